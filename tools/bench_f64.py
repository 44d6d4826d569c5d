#!/usr/bin/env python3
"""tools/bench_f64.py — float32 vs float64 SpGEMM (hip_gpuSpMM vs hip_gpuSpMM_f64) on the bench workloads.

    python tools/bench_f64.py [--reps 7] [--warmup 2] [--workloads synth_1m_16,web_google_surrogate] [--out FILE]

C = A*A with A resident on device 0; every repetition is one call of the entry point, its time is the call's ms_total
from spgemm_stats (HIP events on the handle's stream: classification, symbolic, scan/alloc, numeric).  The two value types
alternate call by call.  One JSON line: per workload the median ms_total of both, their ratio, GFLOP/s = 2*P / t, and the
median per-phase and per-kernel times of a separate pass with every kernel timed (f64 numeric launches are timed into
the slot of their bin: k_num_* names).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sparse_matrix_with_flops_amd import hipspgemm as hs  # noqa: E402
from sparse_matrix_with_flops_amd import synth  # noqa: E402

WORKLOADS = {
    "synth_1m_16": lambda: synth.powerlaw_csr(1 << 20, 43, 2),
    "web_google_surrogate": lambda: synth.webgraph_csr(916428, 46),
}
ALL_KERNELS = (1 << hs.NKERNELS) - 1


def one_call(h, dA):
    dC = hs.gpuSpMMWrapper(dA, dA, h)
    st = h.stats()
    dC.deviceDispose()
    return st


def run(name, reps, warmup):
    rp, ci, v = WORKLOADS[name]()
    m = len(rp) - 1
    out = {"m": m, "nnzA": int(rp[-1])}
    h = hs.Handle(0)
    dev = {}
    for dt in (np.float32, np.float64):
        dev[dt] = hs.CSR.from_arrays(rp, ci, v, m, m, dtype=dt).toGpuCSR()
    try:
        for _ in range(warmup):
            for dt in dev:
                one_call(h, dev[dt])
        times = {np.float32: [], np.float64: []}
        stats = {}
        for _ in range(reps):
            for dt in dev:
                st = one_call(h, dev[dt])
                times[dt].append(st["ms_total"])
                stats[dt] = st
        h.set_kernel_timing(ALL_KERNELS)                    # untimed pass: per-phase and per-kernel times
        prof = {np.float32: [], np.float64: []}
        for _ in range(3):
            for dt in dev:
                prof[dt].append(one_call(h, dev[dt]))
        h.set_kernel_timing(0)
    finally:
        for d in dev.values():
            d.deviceDispose()
        h.close()
    P = stats[np.float32]["total_flops"]
    assert stats[np.float64]["total_flops"] == P and stats[np.float64]["nnzC"] == stats[np.float32]["nnzC"]
    out.update({"P": int(P), "nnzC": int(stats[np.float32]["nnzC"])})
    for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
        med = float(np.median(times[dt]))
        phases = {k: round(float(np.median([s[k] for s in prof[dt]])), 4)
                  for k in ("ms_classify", "ms_symbolic", "ms_scan_alloc", "ms_numeric")}
        kern = {}
        for s in prof[dt]:
            for k, x in s["ms_kernel"].items():
                kern.setdefault(k, []).append(x)
        out[tag] = {"ms_total_median": round(med, 4), "ms_total_runs": [round(x, 4) for x in times[dt]],
                    "GFLOPs": round(2.0 * P / (med * 1e-3) / 1e9, 2), "phases_ms": phases,
                    "kernels_ms": {k: round(float(np.median(x)), 4) for k, x in sorted(kern.items(), key=lambda t: -np.median(t[1]))}}
    out["f64_over_f32"] = round(out["f64"]["ms_total_median"] / out["f32"]["ms_total_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default="synth_1m_16,web_google_surrogate")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if hs.device_count() < 1:
        raise SystemExit("bench_f64.py needs a HIP device (there is no CPU fallback)")
    res = {"tool": "bench_f64", "timing": "median of per-call spgemm_stats.ms_total (HIP events), C=A*A, A resident",
           "reps": args.reps, "workloads": {}}
    for name in args.workloads.split(","):
        res["workloads"][name] = run(name, args.reps, args.warmup)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
