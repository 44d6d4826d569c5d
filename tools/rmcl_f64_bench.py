#!/usr/bin/env python3
"""tools/rmcl_f64_bench.py — R-MCL in double on the device: the loop against the float loop, the fused step against the product.

    python tools/rmcl_f64_bench.py [--reps 7] [--warmup 2] [--iters 10] [--out FILE]

One input, device 0: the R-MCL start matrix of the 500 000-node power-law graph of bench.py's rmcl_500k, as
tools/clusters_bench.py builds it (seed 45, self loops, rows 1/deg), in float32 and in float64 (1/deg computed in double).
Two comparisons, every arm under HIP events on the handle's stream around the blocking call, the arms of a comparison
taking turns in this one process, the median of --reps (at least 7) after --warmup untimed rounds; min and max are kept as
the run-to-run spread:
  loop    --iters iterations: hip_gpuRmclIter_device (float) and hip_gpuRmclIter_device_f64 (double)
  step k  for the operands of the first three iterations of the double loop (Mt after k = 0, 1, 2 iterations):
            fused       hip_rmcl_expand_prune_f64
            product     hip_gpuSpMM_f64 alone (the baseline: the call the fused step shares its walk and tables with)
            two_steps   hip_gpuSpMM_f64 + hip_rmcl_prune_n_f64
          and, in one untimed extra call each with per-kernel timing on, the kernel times of `fused` and `product`; the
          share of the fused step spent in the scan of the kept counts and the pack (call time - classification - symbolic
          pass - scan - numeric launches) is what an unpacked Mt between iterations could save
Parity gate: fused and two_steps keep the same number of entries, or the tool fails and writes no times.
Writes one JSON document (default profiles/rmcl_f64_bench.json).  Nothing is gated on speed.
"""
import os
import sys

import numpy as np

from benchkit import HIP_EVENTS, ROOT, Events, finish, hs, med, need_device, parser, rounded, take_turns

sys.path.insert(0, os.path.join(ROOT, "tests"))


def start_matrices():
    """-> (float32 host CSR, float64 host CSR) of the rmcl_500k start matrix"""
    from helpers import po, synth_csr
    A = synth_csr(500000, 45, 2)
    ri = np.repeat(np.arange(A.rows, dtype=np.int32), np.diff(A.rowPtr))
    M0 = po.rmcl_init(A.rows, A.cols, A.colInd, ri, np.ones_like(A.values))
    deg = np.diff(M0.rowPtr)
    m32 = hs.CSR.from_arrays(M0.rowPtr, M0.colInd, M0.values, M0.rows, M0.cols)
    m64 = hs.CSR.from_arrays(M0.rowPtr, M0.colInd, np.repeat(1.0 / deg, deg), M0.rows, M0.cols, dtype=np.float64)
    return m32, m64


def summary(ms):
    return {"ms": med(ms), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs_ms": rounded(ms)}


def free_raw(out):
    for p in out[:3]:
        hs.dev_free(p)


def main():
    ap = parser(__doc__, "rmcl_f64_bench")
    ap.set_defaults(reps=7, warmup=2)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("rmcl_f64_bench: --reps must be at least 7")
    need_device("rmcl_f64_bench")
    h = hs.Handle(0)
    ev = Events(h.stream())
    m32, m64 = start_matrices()
    d32, d64 = m32.toGpuCSR(), m64.toGpuCSR()
    out = {"rows": m64.rows, "nnz": m64.nnz, "iters": args.iters}

    # ---- the loop, float and double taking turns
    def free_loop(M):
        out["loop_nnz_" + ("double" if M.dtype == np.float64 else "float")] = M.nnz
        M.deviceDispose()

    times, _ = take_turns({"float": lambda: hs.gpuRmclIter_device(args.iters, d32, d32, h),
                           "double": lambda: hs.gpuRmclIter_device(args.iters, d64, d64, h)},
                          args.reps, args.warmup, timer=ev.ms, free=free_loop)
    out["loop"] = {k: summary(v) for k, v in times.items()}
    out["loop"]["double_over_float"] = round(out["loop"]["double"]["ms"] / out["loop"]["float"]["ms"], 3)
    hs.pool_trim(0)

    # ---- the step on the operands of the first three iterations
    def args_of(Mt):
        return (h, d64.rowPtr, d64.colInd, d64.values, d64.nnz, Mt.rowPtr, Mt.colInd, Mt.values, Mt.nnz, d64.rows, d64.cols, Mt.cols)

    def two_steps(Mt):
        ic, jc, vc, nnz = hs.gpu_spmm_raw_f64(*args_of(Mt))
        try:
            return hs.rmcl_prune_raw_f64(h, d64.rows, ic, jc, vc, nnz=nnz)
        finally:
            free_raw((ic, jc, vc))

    steps = []
    Mt = d64
    for k in range(3):
        arms = {"fused": lambda: hs.rmcl_expand_prune_raw_f64(*args_of(Mt)),
                "product": lambda: hs.gpu_spmm_raw_f64(*args_of(Mt)),
                "two_steps": lambda: two_steps(Mt)}
        times, last = take_turns(arms, args.reps, args.warmup, timer=ev.ms, free=free_raw)
        if last["fused"][3] != last["two_steps"][3]:
            raise SystemExit(f"step {k}: fused keeps {last['fused'][3]} entries, two steps {last['two_steps'][3]}")
        rec = {"operand_nnz": Mt.nnz, "nnzC": last["product"][3], "kept": last["fused"][3]}
        rec.update({name: summary(ms) for name, ms in times.items()})
        rec["fused_over_product"] = round(rec["fused"]["ms"] / rec["product"]["ms"], 3)
        rec["fused_over_two_steps"] = round(rec["fused"]["ms"] / rec["two_steps"]["ms"], 3)
        h.set_kernel_timing(0xFFFFFFFF)                       # one untimed call each: where the time goes
        for name in ("fused", "product"):
            ms, res = ev.ms(arms[name])
            free_raw(res)
            st = h.stats()
            rec[name + "_kernels_ms"] = {kn: round(v, 4) for kn, v in st["ms_kernel"].items()}
            rec[name + "_phases_ms"] = {p: round(st[p], 4) for p in ("ms_classify", "ms_symbolic", "ms_scan_alloc", "ms_numeric")}
            rec[name + "_timed_call_ms"] = round(ms, 4)
        h.set_kernel_timing(0)
        ph = rec["fused_phases_ms"]
        rec["fused_pack_and_scan_ms"] = round(rec["fused_timed_call_ms"] - sum(ph.values()), 4)
        rec["fused_pack_and_scan_share"] = round(rec["fused_pack_and_scan_ms"] / rec["fused_timed_call_ms"], 3)
        steps.append(rec)
        nxt = hs.gpuRmclIter_device(1, d64, Mt, h)            # the operand of the next iteration
        if Mt is not d64:
            Mt.deviceDispose()
        Mt = nxt
    if Mt is not d64:
        Mt.deviceDispose()
    out["steps"] = steps
    d32.deviceDispose()
    d64.deviceDispose()
    ev.close()
    finish("rmcl_f64_bench", args, {"rmcl_500k": out}, timing=HIP_EVENTS)


if __name__ == "__main__":
    main()
