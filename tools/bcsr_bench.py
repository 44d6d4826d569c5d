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
import numpy as np

from benchkit import HIP_EVENTS, WORKLOADS, Events, copy_buffers, d2d_arm, finish, hs, load, med, need_device, parser, rounded, \
    round_trip_differs, take_turns


def parity_gate(h, dA, dSorted, r, c):
    b = hs.BCSR(dA, r, c, h)
    back = b.to_csr(0.0, h)
    try:
        hs.sort_rows_device(back, h)
        d = back.diff(dSorted, rel=0.0, abs=0.0, handle=h)
        if round_trip_differs(back, dSorted, d):
            raise SystemExit(f"parity gate, r={r} c={c}: the round trip differs from the matrix: {d.as_dict()}")
        return {"nnzb": b.nnzb, "density_percent": round(b.nonzero_density(), 4), "max_abs_err": d.max_abs_err}
    finally:
        back.deviceDispose()
        b.dispose()


def time_shape(h, ev, dA, copy, r, c, reps, warmup):
    b = hs.BCSR(dA, r, c, h)
    arms = {"to_bcsr": lambda: hs.BCSR(dA, r, c, h), "to_csr": lambda: b.to_csr(1e-9, h), "d2d": d2d_arm(dA, copy, ev),
            "transpose": lambda: dA.transpose(h)}
    try:
        times, _ = take_turns(arms, reps, warmup, timer=ev.ms)
    finally:
        b.dispose()
    out = {"r": r, "c": c}
    for name in arms:
        out[name + "_ms"] = med(times[name])
        out[name + "_runs_ms"] = rounded(times[name])
    for name in ("to_bcsr", "to_csr"):
        out[name + "_ms_over_transpose"] = round(out[name + "_ms"] / out["transpose_ms"], 3)
        out[name + "_ms_over_d2d"] = round(out[name + "_ms"] / out["d2d_ms"], 2)
    return out


def run(name, shapes, reps, warmup):
    hA = load(name)
    h = hs.Handle(0)
    ev = Events(h.stream())
    dA = hA.toGpuCSR()
    dSorted = hA.toGpuCSR()
    copy = copy_buffers(dA)
    try:
        hs.sort_rows_device(dSorted, h)
        out = {"m": hA.rows, "nnz": hA.nnz, "longest_row": int(np.diff(hA.rowPtr).max()), "shapes": {}}
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
    ap = parser(__doc__, "bcsr_bench")
    ap.add_argument("--workload", default="synth_1m_16", choices=sorted(WORKLOADS))
    ap.add_argument("--shapes", default="1x1,2x2,4x4,8x8")
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    need_device("bcsr_bench")
    finish("bcsr_bench", args, {args.workload: run(args.workload, shapes, args.reps, args.warmup)}, timing=HIP_EVENTS,
           dtype="float32")


if __name__ == "__main__":
    main()
