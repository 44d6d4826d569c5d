#!/usr/bin/env python3
"""tools/topk_bench.py — selection (the k largest entries per row) on the device, alone and inside the R-MCL loop.

    python tools/topk_bench.py [--procs 2] [--reps 7] [--warmup 2] [--loop-reps 3] [--out FILE]

float32, device 0.  The input of part (a) is the first-iteration hip_rmcl_expand_prune output of rmcl_500k (the R-MCL start
matrix of the 500 000-node power-law graph of bench.py's rmcl_500k).  One FRESH process per measurement (this file with
--child), --procs of them.  Every process first passes a parity gate at every k: hip_csr_row_topk is bit-equal (rowPtr,
columns, value bits) to the host route a caller had before, or the tool fails and writes no times.
  (a) selection alone, k = 16, 64, 256; the arms take turns, each between two HIP events on the handle's stream, median:
        topk     hip_csr_row_topk (flags 0) as a whole: validation, lengths, scan, copy and selection kernels
        d2d      the three arrays of the input copied device to device: the floor of any pass over the matrix
        prune    hip_rmcl_prune_n on the same matrix: the nearest existing streaming pass (row rule, scan, compaction)
      beside them the host route a caller had before, under the host clock, ONCE per process (it takes seconds): CSR::toCpuCSR,
      one numpy lexsort over (row, NaN, -value, column, position), the first k of every row, CSR::toGpuCSR.  The download and
      the sort do not depend on k: they are done once and counted into the host time of every k.
      With the rows each path of the selection took (spgemm_hip_debug_topk_paths) and the entries kept.
  (b) the loop: ten iterations of hip_gpuRmclIter_device against hip_gpuRmclIter_device_topk at k = 64, taking turns under
      the host clock around the blocking calls; per iteration the entries after selection (iterNnz) and the rows cut
      (iterCut), and the entries of the uncapped result.
Reported: the median over the processes of each process's median.  Writes one JSON document (default
profiles/topk_bench.json).  Nothing is gated on speed.
"""
import json
import os
import subprocess
import sys

import numpy as np

from benchkit import ROOT, Events, clock, copy_buffers, d2d_arm, finish, hs, med, need_device, parser, release, rounded, take_turns

sys.path.insert(0, os.path.join(ROOT, "tests"))
KS = (16, 64, 256)
LOOP_K, LOOP_ITERS = 64, 10
ARMS = ("topk", "d2d", "prune")


def start_matrix():
    """the R-MCL start matrix of the 500 000-node power-law graph (seed 45), on the host"""
    from helpers import po, synth_csr
    A = synth_csr(500000, 45, 2)
    ri = np.repeat(np.arange(A.rows, dtype=np.int32), np.diff(A.rowPtr))
    M0 = po.rmcl_init(A.rows, A.cols, A.colInd, ri, np.ones_like(A.values))
    return hs.CSR.from_arrays(M0.rowPtr, M0.colInd, M0.values, M0.rows, M0.cols)


def host_ranks(H):
    """one lexsort of a host CSR under the library's order -> (the entries from best to worst row by row, each one's rank
    in its row)"""
    row = np.repeat(np.arange(H.rows, dtype=np.int64), np.diff(H.rowPtr.astype(np.int64)))
    nan = np.isnan(H.values)
    worse = np.where(nan, np.float32(0), -H.values) + np.float32(0)
    order = np.lexsort((np.arange(H.nnz), H.colInd, worse, nan, row))
    return order, np.arange(H.nnz) - H.rowPtr.astype(np.int64)[row[order]]


def host_select(H, order, rank, k):
    """the first k of every row, back in storage order"""
    keep = np.sort(order[rank < k])
    rp = np.zeros(H.rows + 1, np.int64)
    np.cumsum(np.minimum(np.diff(H.rowPtr.astype(np.int64)), k), out=rp[1:])
    return hs.CSR.from_arrays(rp, H.colInd[keep], H.values[keep], H.rows, H.cols)


def host_topk(H, k):
    return host_select(H, *host_ranks(H), k)


def same_bits(dA, dB):
    A, B = dA.toCpuCSR(), dB.toCpuCSR()
    return (A.nnz == B.nnz and np.array_equal(A.rowPtr, B.rowPtr) and np.array_equal(A.colInd, B.colInd) and
            A.values.tobytes() == B.values.tobytes())


def prune_arm(h, dX):
    def run():
        i, j, v, nnz = hs.rmcl_prune_raw(h, dX.rows, dX.rowPtr, dX.colInd, dX.values, dX.nnz)
        return [i, j, v]
    return run


def child(reps, warmup, loop_reps):
    h = hs.Handle(0)
    d0 = start_matrix().toGpuCSR()
    i, j, v, n = hs.rmcl_expand_prune_raw(h, d0.rowPtr, d0.colInd, d0.values, d0.nnz, d0.rowPtr, d0.colInd, d0.values, d0.nnz,
                                          d0.rows, d0.rows, d0.rows)
    dX = hs.CSR(v, j, i, d0.rows, d0.cols, n, True, dtype=np.float32)
    ev = Events(h.stream())
    copy = copy_buffers(dX)
    res = {"m": dX.rows, "nnz_start": d0.nnz, "nnz_input": dX.nnz,
           "longest_row": int(np.diff(hs.d2h(dX.rowPtr, dX.rows + 1, np.int32)).max()), "selection": {}}
    try:
        down_ms, H = clock(dX.toCpuCSR)
        sort_ms, (order, rank) = clock(lambda: host_ranks(H))
        for k in KS:
            rest_ms, want = clock(lambda: host_select(H, order, rank, k).toGpuCSR())
            before = h.topk_paths()
            got = dX.row_topk(k, handle=h)
            after = h.topk_paths()
            same, kept, cut = same_bits(got, want), got.nnz, got.rows_cut
            got.deviceDispose()
            want.deviceDispose()
            if not same:
                raise SystemExit(f"parity gate: hip_csr_row_topk and the host route disagree at k={k}")
            arms = {"topk": lambda: dX.row_topk(k, handle=h), "d2d": d2d_arm(dX, copy, ev), "prune": prune_arm(h, dX)}
            t, _ = take_turns(arms, reps, warmup, timer=ev.ms, free=release)
            res["selection"][str(k)] = {"kept": kept, "rows_cut": cut, "paths": {p: after[p] - before[p] for p in after},
                                        "host_ms": rounded([down_ms + sort_ms + rest_ms]),
                                        "host_parts_ms": rounded([down_ms, sort_ms, rest_ms]),
                                        **{a + "_ms": rounded(t[a]) for a in ARMS}}
        seen = {}

        def uncapped():
            out = hs.gpuRmclIter_device(LOOP_ITERS, d0, d0, h)
            seen["nnz_uncapped"] = out.nnz
            return out

        def capped():
            out, seen["iter_nnz"], seen["iter_cut"] = hs.gpuRmclIterTopK_device(LOOP_ITERS, LOOP_K, d0, d0, h)
            seen["nnz_capped"] = out.nnz
            return out
        t, _ = take_turns({"uncapped": uncapped, "capped": capped}, loop_reps, 1, timer=clock, free=release)
        res["loop"] = {"k": LOOP_K, "iterations": LOOP_ITERS, **seen, "uncapped_ms": rounded(t["uncapped"]),
                       "capped_ms": rounded(t["capped"])}
    finally:
        for p in copy:
            hs.dev_free(p)
        ev.close()
        dX.deviceDispose()
        d0.deviceDispose()
        h.close()
    print(json.dumps(res))


def measure(procs, reps, warmup, loop_reps):
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, __file__, "--child", "--reps", str(reps), "--warmup", str(warmup), "--loop-reps",
                            str(loop_reps)], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("a measuring process failed (the parity gate, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print("k=64: " + ", ".join(f"{a} {med(runs[-1]['selection']['64'][a + '_ms'])} ms" for a in ARMS + ("host",)) +
              f"; loop {med(runs[-1]['loop']['uncapped_ms'])} / {med(runs[-1]['loop']['capped_ms'])} ms", file=sys.stderr, flush=True)
    res = {key: runs[0][key] for key in ("m", "nnz_start", "nnz_input", "longest_row")}
    res["selection"] = {}
    for k in map(str, KS):
        first = runs[0]["selection"][k]
        sel = {key: first[key] for key in ("kept", "rows_cut", "paths")}
        for a in ARMS + ("host",):
            per_proc = [med(p["selection"][k][a + "_ms"]) for p in runs]
            sel[a] = {"ms": med(per_proc), "per_process_ms": per_proc}
        sel["host"]["download_sort_rest_ms"] = first["host_parts_ms"]
        sel["topk_over_d2d"] = round(sel["topk"]["ms"] / sel["d2d"]["ms"], 2)
        sel["topk_over_prune"] = round(sel["topk"]["ms"] / sel["prune"]["ms"], 2)
        sel["host_over_topk"] = round(sel["host"]["ms"] / sel["topk"]["ms"], 1)
        res["selection"][k] = sel
    loop = {key: runs[0]["loop"][key] for key in ("k", "iterations", "iter_nnz", "iter_cut", "nnz_uncapped", "nnz_capped")}
    for a in ("uncapped", "capped"):
        per_proc = [med(p["loop"][a + "_ms"]) for p in runs]
        loop[a] = {"ms": med(per_proc), "per_process_ms": per_proc}
    loop["capped_over_uncapped"] = round(loop["capped"]["ms"] / loop["uncapped"]["ms"], 3)
    res["loop"] = loop
    return res


def main():
    ap = parser(__doc__, "topk_bench")
    ap.set_defaults(reps=7, warmup=2)
    ap.add_argument("--procs", type=int, default=2, help="fresh processes")
    ap.add_argument("--loop-reps", type=int, default=3, help="timed rounds of the two ten-iteration loops")
    ap.add_argument("--child", action="store_true", help="(internal) measure in this process")
    args = ap.parse_args()
    need_device("topk_bench")
    if args.child:
        return child(args.reps, args.warmup, args.loop_reps)
    out = {"rmcl_500k": measure(args.procs, args.reps, args.warmup, args.loop_reps)}
    finish("topk_bench", args, out, timing="selection: HIP events on the handle's stream around each arm, median; loop: host "
           "clock around the blocking calls; median over fresh processes of each process's median", dtype="float32",
           procs=args.procs, parity="hip_csr_row_topk bit-equal to the host route at every k in every process")


if __name__ == "__main__":
    main()
