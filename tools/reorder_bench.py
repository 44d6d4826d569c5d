#!/usr/bin/env python3
"""tools/reorder_bench.py — the device reordering primitives and the reference's ordering experiment, timed.

    python tools/reorder_bench.py [--reps 10] [--warmup 2] [--workloads synth_1m_16,web_google_surrogate] [--out FILE]

One process, device 0, float32, the matrix resident on the device.  Every time is a host clock around one blocking entry
point (the calls return after their device work has completed), outputs freed outside the timed region; 2 warm-ups, median
of 10.  Writes one JSON document (default profiles/reorder_bench.json).

primitives   PM, MP, PMPt with a seeded random P, transpose, rowDescendingOrderPermutation: milliseconds, the
             algorithmic bytes (computed below from the shapes: every input array read once, every output array written
             once), the time of spgemm_hip_memcpy_d2d of the same three arrays followed by a device synchronise that
             waits for them (the ceiling: a permutation or transpose cannot move its entries faster than a copy does) and
             time / ceiling.  Reported, not gated.
transpose    hip_csr_transpose against the route a caller had before it: row ids expanded per entry, hip_coo_to_csr with
gate         rows and columns swapped.  The two arms alternate.  The row ids are expanded once, outside the timed region,
             which favours the old route.  Both results must be bit-equal; the new entry point must not be slower, or the
             tool fails.
permuTest    correctTests/permuTest.cc on the device: hip_gpuSpMM of A*A for three orderings (as generated, PMPt with a
             seeded random P, PMPt with the descending-row-length P), the arms alternating; per ordering the median
             spgemm_stats.ms_total, the per-phase times and bin_rows.  Parity gate first: each permuted product, taken
             back with PtMP and row-sorted, must have the structure hash of the unpermuted product and value checksums
             within 1e-6 relative; if it fails the tool fails and writes no times.
"""
import os
import sys

import numpy as np

from benchkit import ROOT, copy_buffers, d2d_arm, finish, hs, load, med, need_device, parser, release, rounded, take_turns

sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import structure_hash, value_checksums  # noqa: E402

PEAK_HBM_GBPS = 8000.0                                      # MI355X HBM3E peak
PHASES = ("ms_classify", "ms_symbolic", "ms_scan_alloc", "ms_numeric")


def algorithmic_bytes(m, n, nnz):
    """bytes each primitive must move: inputs read once, outputs written once (int32 indices, float32 values)"""
    rowptr_in, rowptr_out, entries = 4 * (m + 1), 4 * (m + 1), 8 * nnz
    return {
        "PM": rowptr_in + 4 * m + rowptr_out + 2 * entries,                   # + rowSrc
        "MP": rowptr_in + 4 * n + rowptr_out + 2 * entries,                   # + colMap (every element once)
        "PMPt": rowptr_in + 4 * m + 4 * n + rowptr_out + 2 * entries,
        "transpose": rowptr_in + entries + 4 * (n + 1) + entries,
        "rowDescendingOrderPermutation": rowptr_in + 4 * m,
    }


def primitives(h, dA, P, Pt, reps, warmup):
    m, n, nnz = dA.rows, dA.cols, dA.nnz
    dP, dPt = hs.h2d(P), hs.h2d(Pt)
    copy = copy_buffers(dA)

    # a device-to-device hipMemcpy may return before the copy has run: the device synchronise makes the arm as blocking
    # as the entry points it is compared with (benchkit.d2d_arm does the same for the three arrays)
    def d2d_rowptr():
        hs.d2d(copy[0], dA.rowPtr, 4 * (m + 1))
        hs.device_synchronize()

    def permute(rowSrc, colMap):
        return lambda: list(hs.csr_permute_raw(h, m, n, nnz, dA.rowPtr, dA.colInd, dA.values, rowSrc, colMap))
    arms = {
        "d2d_csr": d2d_arm(dA, copy), "d2d_rowptr": d2d_rowptr,
        "PM": permute(dP, None), "MP": permute(None, dP), "PMPt": permute(dP, dPt),
        "transpose": lambda: list(hs.csr_transpose_raw(h, m, n, nnz, dA.rowPtr, dA.colInd, dA.values)),
        "rowDescendingOrderPermutation": lambda: [hs.row_descending_permutation_raw(h, m, dA.rowPtr)],
    }
    try:
        t, _ = take_turns(arms, reps, warmup)
    finally:
        release(copy + [dP, dPt])
    nbytes = algorithmic_bytes(m, n, nnz)
    out = {"d2d_csr_ms": med(t["d2d_csr"]), "d2d_rowptr_ms": med(t["d2d_rowptr"]),
           "d2d_csr_runs_ms": rounded(t["d2d_csr"]), "d2d_rowptr_runs_ms": rounded(t["d2d_rowptr"])}
    # a copy reads and writes every byte once: a time below what PEAK_HBM allows has not waited for the copy
    copied = 2 * (4 * (m + 1) + 8 * nnz)
    out["d2d_csr_GBps"] = round(copied / (out["d2d_csr_ms"] * 1e-3) / 1e9, 1)
    if out["d2d_csr_GBps"] > PEAK_HBM_GBPS:
        raise SystemExit(f"d2d ceiling: {out['d2d_csr_GBps']} GB/s is above the HBM peak: the arm did not wait for the copy")
    for name in nbytes:
        ceiling = out["d2d_rowptr_ms"] if name == "rowDescendingOrderPermutation" else out["d2d_csr_ms"]
        ms = med(t[name])
        out[name] = {"ms": ms, "bytes": int(nbytes[name]), "GBps": round(nbytes[name] / (ms * 1e-3) / 1e9, 1),
                     "d2d_ms": ceiling, "ms_over_d2d": round(ms / ceiling, 2), "runs_ms": rounded(t[name])}
    return out


def transpose_gate(h, hA, dA, reps, warmup):
    m, n, nnz = dA.rows, dA.cols, dA.nnz
    row_of = np.repeat(np.arange(m, dtype=np.int32), np.diff(hA.rowPtr))
    dRow = hs.h2d(row_of)                                                     # expanded outside the timed region

    def new():
        return list(hs.csr_transpose_raw(h, m, n, nnz, dA.rowPtr, dA.colInd, dA.values))

    def old():
        return list(hs.coo_to_csr_raw(h, n, m, nnz, dA.colInd, dRow, dA.values, 0)[:3])
    try:
        a, b = new(), old()                                                   # same bits first
        same = all(np.array_equal(hs.d2h(x, cnt, np.int32), hs.d2h(y, cnt, np.int32))
                   for x, y, cnt in zip(a, b, (n + 1, nnz, nnz)))
        release(a + b)
        if not same:
            raise SystemExit("transpose gate: hip_csr_transpose and the hip_coo_to_csr route disagree")
        t, _ = take_turns({"hip_csr_transpose": new, "coo_to_csr_route": old}, reps, warmup)
    finally:
        hs.dev_free(dRow)
    out = {k: {"ms": med(v), "runs_ms": rounded(v)} for k, v in t.items()}
    out["new_over_old"] = round(out["hip_csr_transpose"]["ms"] / out["coo_to_csr_route"]["ms"], 3)
    out["radix_passes"] = {"hip_csr_transpose": -(-max(1, int(n - 1).bit_length()) // 8),
                           "coo_to_csr_route": -(-(max(1, int(n - 1).bit_length()) + int(m - 1).bit_length()) // 8)}
    if out["new_over_old"] > 1.0:
        raise SystemExit(f"transpose gate: hip_csr_transpose takes {out['new_over_old']} x the hip_coo_to_csr route")
    return out


def summary_of(dC, h):
    """row-sorted on the device, then structure hash and the two value checksums"""
    hs.sort_rows_device(dC, h)
    C = dC.toCpuCSR()
    return structure_hash(C.rowPtr, C.colInd), value_checksums(C.colInd, C.values)


def permu_test(h, dA, orders, reps, warmup):
    """orders: {name: P or None}.  Parity gate, then the alternating timed products."""
    mats = {}
    try:
        for name, P in orders.items():
            mats[name] = dA if P is None else dA.PMPt(P, h)
        want = None
        for name, P in orders.items():                       # as generated comes first
            dC = hs.gpuSpMMWrapper(mats[name], mats[name], h)
            if P is not None:
                back = dC.PtMP(P, h)
                dC.deviceDispose()
                dC = back
            got = summary_of(dC, h)
            dC.deviceDispose()
            if want is None:
                want = got
                continue
            if got[0] != want[0]:
                raise SystemExit(f"permuTest parity gate: structure hash of the {name} product differs")
            for x, y in zip(got[1], want[1]):
                if abs(x - y) > 1e-6 * max(abs(x), abs(y)):
                    raise SystemExit(f"permuTest parity gate: checksum of the {name} product {x!r} vs {y!r}")
        runs = {k: [] for k in orders}
        for it in range(warmup + reps):
            for name in orders:
                dC = hs.gpuSpMMWrapper(mats[name], mats[name], h)
                st = h.stats()
                dC.deviceDispose()
                if it >= warmup:
                    runs[name].append(st)
    finally:
        for name, d in mats.items():
            if d is not dA:
                d.deviceDispose()
    out = {"parity": "structure hash equal, checksums within 1e-6 relative"}
    for name, sts in runs.items():
        out[name] = {"ms_total": med([s["ms_total"] for s in sts]), "runs_ms_total": rounded(s["ms_total"] for s in sts),
                     "phases_ms": {k: med([s[k] for s in sts]) for k in PHASES}, "bin_rows": sts[-1]["bin_rows"],
                     "nnzC": sts[-1]["nnzC"], "P": sts[-1]["total_flops"]}
    base = out["as_generated"]["ms_total"]
    for name in orders:
        out[name]["over_as_generated"] = round(out[name]["ms_total"] / base, 3)
    return out


def run(name, reps, warmup):
    hA = load(name)
    m = hA.rows
    h = hs.Handle(0)
    dA = hA.toGpuCSR()
    try:
        P = np.random.default_rng(2024).permutation(m).astype(np.int32)
        Pt = hs.permutation_transpose(P, h)
        Pdesc = dA.rowDescendingOrderPermutation(h)
        lens = np.diff(hA.rowPtr)
        assert np.array_equal(Pdesc, np.argsort(-lens.astype(np.int64), kind="stable"))
        out = {"m": m, "nnzA": hA.nnz, "longest_row": int(lens.max())}
        out["permuTest"] = permu_test(h, dA, {"as_generated": None, "random": P, "descending_length": Pdesc}, reps, warmup)
        out["primitives"] = primitives(h, dA, P, Pt, reps, warmup)
        out["transpose_gate"] = transpose_gate(h, hA, dA, reps, warmup)
    finally:
        dA.deviceDispose()
        h.close()
    return out


def main():
    ap = parser(__doc__, "reorder_bench")
    ap.add_argument("--workloads", default="synth_1m_16,web_google_surrogate")
    args = ap.parse_args()
    need_device("reorder_bench")
    finish("reorder_bench", args, {name: run(name, args.reps, args.warmup) for name in args.workloads.split(",")})


if __name__ == "__main__":
    main()
