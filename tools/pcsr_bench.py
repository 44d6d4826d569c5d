#!/usr/bin/env python3
"""tools/pcsr_bench.py — the column-partitioned product (correctTests/pcsrTest.cc on the device), timed.

    python tools/pcsr_bench.py [--reps 10] [--warmup 2] [--workloads synth_1m_16,web_google_surrogate] [--blocks 1,2,4,8]
                               [--out FILE]

One process, device 0, float32, the matrix resident on the device; the product is A*A with B = A cut into c column
blocks.  Every time is a host clock around one blocking entry point (the calls return after their device work has
completed), outputs freed outside the timed region; 2 warm-ups, median of 10.  Writes one JSON document (default
profiles/pcsr_bench.json).  Nothing is gated on speed.

parity gate  first, per c: the blockwise product, joined and row-sorted on the device, against the row-sorted whole
             product through hip_csr_diff at rel_tol = 1e-6: structure identical (rows_len_differ == only_a == only_b
             == 0) and beyond == 0.  If it fails the tool fails and writes no times.
split, join  hip_csr_split_columns of B and hip_pcsr_join of the c product blocks, each beside the time of
             spgemm_hip_memcpy_d2d of the same three arrays followed by a device synchronise (the ceiling: neither can
             move its entries faster than a copy does).  Reported, not gated.
product      hip_pcsr_spmm over the c blocks against the whole hip_gpuSpMM, the two arms alternating.
per block    a separate pass with the big-row kernels' event timing on: hip_gpuSpMM per block, its spgemm_stats phase
             times, bin_rows (the last bin = rows above 4096 products) and ms_kernel of k_sym_big, k_num_bighash and
             k_num_big (which takes the last bin's rows instead of k_num_bighash when C is narrow enough); the same
             for the whole product.
"""
import numpy as np

from benchkit import copy_buffers, d2d_arm, finish, hs, load, med, need_device, parser, rounded, round_trip_differs, take_turns

PHASES = ("ms_classify", "ms_symbolic", "ms_scan_alloc", "ms_numeric")
K_SYM_BIG, K_NUM_BIG, K_NUM_BIGHASH = 8, 15, 16             # SPGEMM_K_* of include/spgemm_hip.h
BIG_KERNELS = ("k_sym_big", "k_num_big", "k_num_bighash")   # the last bin's numeric kernel is k_num_big when C is narrow


def parity_gate(h, dA, whole_sorted, c):
    pB = hs.PCSR(dA, c, h)
    pC = pB.spmm_left(dA, h)
    joined = pC.join(h)
    try:
        hs.sort_rows_device(joined, h)
        d = joined.diff(whole_sorted, rel=1e-6, abs=0.0, handle=h)
        if round_trip_differs(joined, whole_sorted, d):
            raise SystemExit(f"parity gate, c={c}: the blockwise product differs from the whole product: {d.as_dict()}")
        return {"max_abs_err": d.max_abs_err, "max_rel_err": d.max_rel_err}
    finally:
        joined.deviceDispose()
        pC.deviceDispose()
        pB.deviceDispose()


def stats_of(sts):
    """median phase times, the bins and the big-row kernels of repeated spgemm_stats of one product"""
    last = sts[-1]
    return {"ms_total": med([s["ms_total"] for s in sts]), "phases_ms": {k: med([s[k] for s in sts]) for k in PHASES},
            "bin_rows": last["bin_rows"], "rows_in_last_bin": last["bin_rows"][-1], "P": last["total_flops"], "nnzC": last["nnzC"],
            "ms_kernel": {k: med([s["ms_kernel"].get(k, 0.0) for s in sts]) for k in BIG_KERNELS}}


def per_block(h, dA, mats, reps, warmup):
    """mats: {name: device CSR B}; hip_gpuSpMM(A, B) per entry with the big-row kernels' events on -> {name: stats}"""
    h.set_kernel_timing((1 << K_SYM_BIG) | (1 << K_NUM_BIG) | (1 << K_NUM_BIGHASH))
    runs = {k: [] for k in mats}
    try:
        for it in range(warmup + reps):
            for name, dB in mats.items():
                hs.gpuSpMMWrapper(dA, dB, h).deviceDispose()
                if it >= warmup:
                    runs[name].append(h.stats())
    finally:
        h.set_kernel_timing(0)
    return {name: stats_of(sts) for name, sts in runs.items()}


def one_block_count(h, dA, dC, c, reps, warmup):
    pB = hs.PCSR(dA, c, h)
    pC = pB.spmm_left(dA, h)
    copyB, copyC = copy_buffers(dA), copy_buffers(dC)
    try:
        arms = {
            "split": lambda: hs.PCSR(dA, c, h), "d2d_B": d2d_arm(dA, copyB),
            "join": lambda: pC.join(h), "d2d_C": d2d_arm(dC, copyC),
            "hip_pcsr_spmm": lambda: pB.spmm_left(dA, h), "hip_gpuSpMM": lambda: hs.gpuSpMMWrapper(dA, dA, h),
        }
        t, _ = take_turns(arms, reps, warmup)
        out = {"stride": pB.stride, "block_nnz": [b.nnz for b in pB.blocks], "product_block_nnz": [b.nnz for b in pC.blocks]}
        for name, ceiling in (("split", "d2d_B"), ("join", "d2d_C")):
            out[name] = {"ms": med(t[name]), "d2d_ms": med(t[ceiling]), "ms_over_d2d": round(med(t[name]) / med(t[ceiling]), 2),
                         "runs_ms": rounded(t[name]), "d2d_runs_ms": rounded(t[ceiling])}
        out["product"] = {"hip_pcsr_spmm_ms": med(t["hip_pcsr_spmm"]), "hip_gpuSpMM_ms": med(t["hip_gpuSpMM"]),
                          "blockwise_over_whole": round(med(t["hip_pcsr_spmm"]) / med(t["hip_gpuSpMM"]), 3),
                          "hip_pcsr_spmm_runs_ms": rounded(t["hip_pcsr_spmm"]), "hip_gpuSpMM_runs_ms": rounded(t["hip_gpuSpMM"])}
        mats = {f"block {b}": pB.block(b) for b in range(c)}
        mats["whole"] = dA
        out["per_block"] = per_block(h, dA, mats, reps, warmup)
        blocks = [out["per_block"][f"block {b}"] for b in range(c)]
        out["sum_over_blocks"] = {"rows_in_last_bin": sum(b["rows_in_last_bin"] for b in blocks),
                                  "ms_total": round(sum(b["ms_total"] for b in blocks), 4),
                                  "ms_kernel": {k: round(sum(b["ms_kernel"][k] for b in blocks), 4) for k in BIG_KERNELS}}
        return out
    finally:
        for p in copyB + copyC:
            hs.dev_free(p)
        pC.deviceDispose()
        pB.deviceDispose()


def run(name, counts, reps, warmup):
    hA = load(name)
    h = hs.Handle(0)
    dA = hA.toGpuCSR()
    dC = hs.gpuSpMMWrapper(dA, dA, h)
    try:
        out = {"m": hA.rows, "nnzA": hA.nnz, "nnzC": dC.nnz, "longest_row": int(np.diff(hA.rowPtr).max()), "parity": {}, "blocks": {}}
        hs.sort_rows_device(dC, h)
        for c in counts:                                     # every gate before any time
            out["parity"][str(c)] = parity_gate(h, dA, dC, c)
        out["parity"]["rule"] = "joined and row-sorted against the row-sorted whole product: structure identical, beyond == 0 at rel_tol 1e-6"
        for c in counts:
            out["blocks"][str(c)] = one_block_count(h, dA, dC, c, reps, warmup)
    finally:
        dC.deviceDispose()
        dA.deviceDispose()
        h.close()
    return out


def main():
    ap = parser(__doc__, "pcsr_bench")
    ap.add_argument("--workloads", default="synth_1m_16,web_google_surrogate")
    ap.add_argument("--blocks", default="1,2,4,8")
    args = ap.parse_args()
    need_device("pcsr_bench")
    counts = [int(x) for x in args.blocks.split(",")]
    finish("pcsr_bench", args, {name: run(name, counts, args.reps, args.warmup) for name in args.workloads.split(",")})


if __name__ == "__main__":
    main()
