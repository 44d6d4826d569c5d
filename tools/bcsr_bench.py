#!/usr/bin/env python3
"""tools/bcsr_bench.py — the blocked CSR on the device (hip_csr_to_bcsr, hip_bcsr_to_csr), timed.

    python tools/bcsr_bench.py [--reps 10] [--warmup 2] [--workload synth_1m_16] [--shapes 1x1,2x2,4x4,8x8] [--out FILE]

One process, device 0, float32, the matrix resident on the device.  Every time is the distance between two HIP events
recorded on the handle's stream around one blocking entry point (so it contains the call's own host read-backs: the
validation flag and the tile count), outputs freed outside the timed region; 2 warm-ups, median of 10, the arms taking
turns.  Writes one JSON document (default profiles/bcsr_bench.json).  Nothing is gated on speed.

parity gate  first, per shape: to_bcsr -> to_csr(drop_tol = 0) -> hip_csr_sort_rows against the row-sorted matrix through
             hip_csr_diff at abs_tol = rel_tol = 0: rows_len_differ == only_a == only_b == beyond == 0 and the same nnz.
             If it fails the tool fails and writes no times.
to_bcsr      hip_csr_to_bcsr of the matrix per shape, with nnzb and the fill (BCSR::nonzeroDensity) it finds
to_csr       hip_bcsr_to_csr (drop_tol = 1e-9) of that result
d2d          beside them: the three CSR arrays copied device to device on the same stream (no reordering can be faster)
transpose    beside them: hip_csr_transpose of the same matrix, the existing operation of the same build (one radix sort
             plus a scatter); ms_over_transpose is the ratio of the medians
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sparse_matrix_with_flops_amd import hipspgemm as hs  # noqa: E402
from sparse_matrix_with_flops_amd import synth  # noqa: E402

WORKLOADS = {
    "synth_1m_16": lambda: synth.powerlaw_csr(1 << 20, 43, 2)[:3],          # the matrix bench.py times
    "synth_256k_16": lambda: synth.powerlaw_csr(1 << 18, 43, 2)[:3],
}
D2D = 3                                                     # hipMemcpyDeviceToDevice


class Events:
    """two HIP events on one stream: ms(fn) = device-timeline milliseconds from before fn() to after it"""

    def __init__(self, stream):
        try:
            self.hip = C.CDLL("libamdhip64.so")
        except OSError:
            self.hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.stream = C.c_void_p(stream)
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        for e in (self.e0, self.e1):
            self.ok(self.hip.hipEventCreate(C.byref(e)), "hipEventCreate")

    @staticmethod
    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"{what} failed with HIP error {rc}")

    def ms(self, fn):
        self.ok(self.hip.hipEventRecord(self.e0, self.stream), "hipEventRecord")
        out = fn()
        self.ok(self.hip.hipEventRecord(self.e1, self.stream), "hipEventRecord")
        self.ok(self.hip.hipEventSynchronize(self.e1), "hipEventSynchronize")
        t = C.c_float(0)
        self.ok(self.hip.hipEventElapsedTime(C.byref(t), self.e0, self.e1), "hipEventElapsedTime")
        return float(t.value), out

    def copy(self, dst, src, nbytes):
        self.ok(self.hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), nbytes, D2D, self.stream), "hipMemcpyAsync")

    def close(self):
        for e in (self.e0, self.e1):
            self.hip.hipEventDestroy(e)


def med(x):
    return round(float(np.median(x)), 4)


def parity_gate(h, dA, dSorted, r, c):
    b = hs.BCSR(dA, r, c, h)
    back = b.to_csr(0.0, h)
    try:
        hs.sort_rows_device(back, h)
        d = back.diff(dSorted, rel=0.0, abs=0.0, handle=h)
        if back.nnz != dSorted.nnz or d.rows_len_differ or d.only_a or d.only_b or d.beyond:
            raise SystemExit(f"parity gate, r={r} c={c}: the round trip differs from the matrix: {d.as_dict()}")
        return {"nnzb": b.nnzb, "density_percent": round(b.nonzero_density(), 4), "max_abs_err": d.max_abs_err}
    finally:
        back.deviceDispose()
        b.dispose()


def time_shape(h, ev, dA, copy, r, c, reps, warmup):
    b = hs.BCSR(dA, r, c, h)

    def d2d():
        ev.copy(copy[0], dA.rowPtr, 4 * (dA.rows + 1))
        ev.copy(copy[1], dA.colInd, 4 * dA.nnz)
        ev.copy(copy[2], dA.values, 4 * dA.nnz)

    arms = {"to_bcsr": (lambda: hs.BCSR(dA, r, c, h), lambda o: o.dispose()),
            "to_csr": (lambda: b.to_csr(1e-9, h), lambda o: o.deviceDispose()),
            "d2d": (d2d, lambda o: None),
            "transpose": (lambda: dA.transpose(h), lambda o: o.deviceDispose())}
    times = {k: [] for k in arms}
    try:
        for it in range(warmup + reps):
            for name, (fn, free) in arms.items():
                ms, out = ev.ms(fn)
                free(out)
                if it >= warmup:
                    times[name].append(ms)
    finally:
        b.dispose()
    out = {"r": r, "c": c}
    for name in arms:
        out[name + "_ms"] = med(times[name])
        out[name + "_runs_ms"] = [round(x, 4) for x in times[name]]
    for name in ("to_bcsr", "to_csr"):
        out[name + "_ms_over_transpose"] = round(out[name + "_ms"] / out["transpose_ms"], 3)
        out[name + "_ms_over_d2d"] = round(out[name + "_ms"] / out["d2d_ms"], 2)
    return out


def run(name, shapes, reps, warmup):
    rp, ci, v = WORKLOADS[name]()
    m = len(rp) - 1
    hA = hs.CSR.from_arrays(rp, ci, v, m, m)
    h = hs.Handle(0)
    ev = Events(h.stream())
    dA = hA.toGpuCSR()
    dSorted = hA.toGpuCSR()
    copy = [hs.dev_alloc(4 * (m + 1)), hs.dev_alloc(4 * hA.nnz), hs.dev_alloc(4 * hA.nnz)]
    try:
        hs.sort_rows_device(dSorted, h)
        out = {"m": m, "nnz": hA.nnz, "longest_row": int(np.diff(rp).max()), "shapes": {}}
        gates = {f"{r}x{c}": parity_gate(h, dA, dSorted, r, c) for r, c in shapes}       # every gate before any time
        for r, c in shapes:
            res = time_shape(h, ev, dA, copy, r, c, reps, warmup)
            res.update(gates[f"{r}x{c}"])
            out["shapes"][f"{r}x{c}"] = res
        out["parity_rule"] = ("sort_rows(to_csr(to_bcsr(A), drop_tol 0)) against sort_rows(A) through hip_csr_diff at tolerance 0: "
                              "same nnz, rows_len_differ == only_a == only_b == beyond == 0")
    finally:
        for p in copy:
            hs.dev_free(p)
        dSorted.deviceDispose()
        dA.deviceDispose()
        ev.close()
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="synth_1m_16", choices=sorted(WORKLOADS))
    ap.add_argument("--shapes", default="1x1,2x2,4x4,8x8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcsr_bench.json"))
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    if hs.device_count() < 1:
        raise SystemExit("bcsr_bench.py needs a HIP device (there is no CPU fallback)")
    res = {"tool": "bcsr_bench", "timing": "HIP events on the handle's stream around blocking calls, median", "reps": args.reps,
           "warmup": args.warmup, "dtype": "float32", "workloads": {args.workload: run(args.workload, shapes, args.reps, args.warmup)}}
    with open(args.out, "w") as f:                          # only after every gate has passed
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
