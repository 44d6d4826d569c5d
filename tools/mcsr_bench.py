#!/usr/bin/env python3
"""tools/mcsr_bench.py — the mixed CSR on the device (hip_csr_to_mcsr, hip_mcsr_to_csr), timed on a reordered matrix.

    python tools/mcsr_bench.py [--reps 10] [--warmup 2] [--workload synth_1m_16] [--corners 4096,16384,65536]
                               [--shapes 2x2,4x4,8x8] [--out FILE]

One process, device 0, float32.  The matrix is the workload reordered on the device so that its heavy rows and columns
come first: P = hip_csr_row_descending_permutation, then PMPt (hip_csr_permute).  Every time is the distance between two
HIP events recorded on the handle's stream around one blocking entry point (so it contains the call's own host
read-backs), outputs freed outside the timed region; 2 warm-ups, median of 10 with the runs kept, the arms taking turns.
Writes one JSON document (default profiles/mcsr_bench.json).  Nothing is gated on speed or fill.

parity gate  first, per corner and shape: to_mcsr -> to_csr(drop_tol = 0) -> hip_csr_sort_rows against the row-sorted
             matrix through hip_csr_diff at abs_tol = rel_tol = 0: rows_len_differ == only_a == only_b == beyond == 0 and
             the same nnz.  If it fails the tool fails and writes no times.
to_mcsr      hip_csr_to_mcsr with a K x K corner, per K and shape, with what it finds: the share of the entries that went
             into the corner, nnzb, the corner's fill (nonzeroDensity), bytes of tiles plus remainder against the CSR's
to_csr       hip_mcsr_to_csr (drop_tol = 1e-9) of that result
bcsr         beside them, per shape: hip_csr_to_bcsr / hip_bcsr_to_csr of the WHOLE reordered matrix, with its bytes
d2d          beside them: the three CSR arrays copied device to device on the same stream
"""
import numpy as np

from benchkit import HIP_EVENTS, WORKLOADS, Events, copy_buffers, d2d_arm, finish, hs, load, med, need_device, parser, rounded, \
    round_trip_differs, take_turns


def csr_bytes(m, nnz):
    return 4 * (m + 1) + 8 * nnz


def tiles_bytes(bm, nnzb, r, c):
    return 4 * (bm + 1) + 4 * nnzb + 4 * nnzb * r * c


def describe(x, nnz):
    """what one split found, from the host-side counts alone"""
    mixed = tiles_bytes(x.bm, x.nnzb, x.r, x.c) + csr_bytes(x.m, x.remainder.nnz)
    return {"corner_entries": x.nnz, "corner_share_percent": round(100.0 * x.nnz / nnz, 4), "nnzb": x.nnzb,
            "corner_fill_percent": round(x.nonzero_density(), 4), "remainder_nnz": x.remainder.nnz,
            "mixed_bytes": mixed, "csr_bytes": csr_bytes(x.m, nnz), "mixed_over_csr_bytes": round(mixed / csr_bytes(x.m, nnz), 4)}


def parity_gate(h, dA, dSorted, r, c, k):
    x = hs.MCSR(dA, r, c, k, k, h)
    back = x.to_csr(0.0, h)
    try:
        hs.sort_rows_device(back, h)
        d = back.diff(dSorted, rel=0.0, abs=0.0, handle=h)
        if round_trip_differs(back, dSorted, d):
            raise SystemExit(f"parity gate, r={r} c={c} corner {k}: the round trip differs from the matrix: {d.as_dict()}")
        out = describe(x, dA.nnz)
        out["max_abs_err"] = d.max_abs_err
        return out
    finally:
        back.deviceDispose()
        x.dispose()


def time_shape(h, ev, dA, copy, r, c, ks, reps, warmup):
    """all arms of one tile shape in one rotation: the three corners, the whole-matrix BCSR and the copy"""
    held = {k: hs.MCSR(dA, r, c, k, k, h) for k in ks}
    whole = hs.BCSR(dA, r, c, h)
    arms = {}
    for k in ks:
        arms[f"to_mcsr_{k}"] = lambda k=k: hs.MCSR(dA, r, c, k, k, h)
        arms[f"to_csr_{k}"] = lambda k=k: held[k].to_csr(1e-9, h)
    arms["to_bcsr"] = lambda: hs.BCSR(dA, r, c, h)
    arms["bcsr_to_csr"] = lambda: whole.to_csr(1e-9, h)
    arms["d2d"] = d2d_arm(dA, copy, ev)
    try:
        times, _ = take_turns(arms, reps, warmup, timer=ev.ms)
        whole_bytes = tiles_bytes(whole.bm, whole.nnzb, r, c)
        whole_info = {"nnzb": whole.nnzb, "fill_percent": round(whole.nonzero_density(), 4), "bytes": whole_bytes,
                      "bytes_over_csr": round(whole_bytes / csr_bytes(dA.rows, dA.nnz), 4)}
    finally:
        whole.dispose()
        for x in held.values():
            x.dispose()

    def arm(name):
        t = times[name]
        return {"ms": med(t), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "runs_ms": rounded(t)}
    out = {"r": r, "c": c, "whole_matrix_bcsr": dict(whole_info, to_bcsr=arm("to_bcsr"), to_csr=arm("bcsr_to_csr")),
           "d2d": arm("d2d"), "corners": {}}
    for k in ks:
        out["corners"][str(k)] = {"to_mcsr": arm(f"to_mcsr_{k}"), "to_csr": arm(f"to_csr_{k}")}
    return out


def run(name, shapes, ks, reps, warmup):
    hA = load(name)
    m = hA.rows
    h = hs.Handle(0)
    ev = Events(h.stream())
    d0 = hA.toGpuCSR()
    dA = dSorted = None
    copy = copy_buffers(d0)
    try:
        P = d0.rowDescendingOrderPermutation(h)
        dA = d0.PMPt(P, h)                                  # heavy rows and columns first; rows unsorted
        dSorted = d0.PMPt(P, h)
        hs.sort_rows_device(dSorted, h)
        lens = np.diff(hA.rowPtr)[P]
        out = {"m": m, "nnz": hA.nnz, "longest_row": int(lens[0]), "reordering": "P = row_descending_permutation, PMPt",
               "row_length_at": {str(k): int(lens[k - 1]) for k in ks if k <= m}, "shapes": {}}
        gates = {(r, c, k): parity_gate(h, dA, dSorted, r, c, k) for r, c in shapes for k in ks}   # every gate before any time
        for r, c in shapes:
            res = time_shape(h, ev, dA, copy, r, c, ks, reps, warmup)
            for k in ks:
                res["corners"][str(k)].update(gates[(r, c, k)])
            out["shapes"][f"{r}x{c}"] = res
        out["parity_rule"] = ("sort_rows(to_csr(to_mcsr(A), drop_tol 0)) against sort_rows(A) through hip_csr_diff at tolerance 0: "
                              "same nnz, rows_len_differ == only_a == only_b == beyond == 0")
    finally:
        for p in copy:
            hs.dev_free(p)
        for d in (dSorted, dA, d0):
            if d is not None:
                d.deviceDispose()
        ev.close()
        h.close()
    return out


def main():
    ap = parser(__doc__, "mcsr_bench")
    ap.add_argument("--workload", default="synth_1m_16", choices=sorted(WORKLOADS))
    ap.add_argument("--corners", default="4096,16384,65536")
    ap.add_argument("--shapes", default="2x2,4x4,8x8")
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    ks = [int(x) for x in args.corners.split(",")]
    need_device("mcsr_bench")
    finish("mcsr_bench", args, {args.workload: run(args.workload, shapes, ks, args.reps, args.warmup)}, timing=HIP_EVENTS,
           dtype="float32")


if __name__ == "__main__":
    main()
