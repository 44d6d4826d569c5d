#!/usr/bin/env python3
"""tools/edges_f64_bench.py — a double-valued edge-list file to a device CSR: the double loader beside the float one.

    python tools/edges_f64_bench.py [--reps 10] [--warmup 2] [--workload synth_1m_16] [--out FILE]

One process, device 0, through the Python binding.  The workload's edge list is written as text in shuffled order, every
line "from to %.17g" (the value widened to double and printed with 17 significant digits, as a double-valued file is),
behind a "rows nnz" size line; writing it is outside the timed region.
  arm F64   read_edge_file(dtype=float64, DEDUPE): hip_parse_edge_text_f64 + hip_coo_to_csr_f64
  arm F32   read_edge_file(DEDUPE) on the same file: the float entries (17 digits are slow lines there: host strtof)
Parity gate first: the structure of the f64 CSR equals the f32 CSR's through hip_csr_diff on the indices (the f64 values
narrowed are not compared: the two loaders round differently by design), or the tool fails and writes no times.
Then 2 warm-ups and the arms taking turns, median of 10 with the runs kept; wall clock around each call ending in a device
synchronise, plus the phases spgemm_edge_stats reports per arm (the COO phase is wall - ms_total: hip_coo_to_csr and the
file's mapping).  Both arms read the file from the page cache.
Writes one JSON document (default profiles/edges_f64_bench.json).  Nothing is gated on speed.
"""
import os
import tempfile

import numpy as np

from benchkit import WORKLOADS, clock, finish, hs, load, med, need_device, parser, rounded, take_turns

PHASES = ("ms_upload", "ms_split", "ms_parse", "ms_slow", "ms_total")


def write_edge_list(path, A, seed=5):
    """the CSR's entries as "row col %.17g" lines in shuffled order behind a "rows nnz" size line"""
    rng = np.random.default_rng(seed)
    ri = np.repeat(np.arange(A.rows, dtype=np.int64), np.diff(A.rowPtr.astype(np.int64)))
    order = rng.permutation(A.nnz)
    ri, ci, v = ri[order], A.colInd[order], A.values[order].astype(np.float64)
    with open(path, "w") as f:
        f.write(f"# {A.rows} rows, {A.nnz} entries, shuffled\n{A.rows} {A.nnz}\n")
        step = 1 << 20
        for lo in range(0, A.nnz, step):
            f.write("".join(f"{r} {c} {x:.17g}\n" for r, c, x in zip(ri[lo:lo + step].tolist(), ci[lo:lo + step].tolist(),
                                                                      v[lo:lo + step].tolist())))
    return os.path.getsize(path)


def structure_differs(h, a, b):
    """hip_csr_diff on the indices of two device CSRs of different value types: both get the same all-ones float values"""
    if (a.rows, a.cols, a.nnz) != (b.rows, b.cols, b.nnz):
        return True
    ones = hs.h2d(np.ones(max(a.nnz, 1), np.float32))
    try:
        d = hs.csr_diff_raw(h, a.rows, a.cols, a.rowPtr, a.colInd, ones, a.nnz, b.rowPtr, b.colInd, ones, b.nnz, 0.0, 0.0)
    finally:
        hs.dev_free(ones)
    return bool(d.rows_len_differ or d.only_a or d.only_b or d.beyond)


def run(name, reps, warmup):
    A = load(name)
    h = hs.Handle(0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, name + "_f64.snap")
        nbytes = write_edge_list(path, A)
        stats = {"F64": [], "F32": []}

        def arm(key, dtype):
            def call():
                M = hs.read_edge_file(path, True, hs.COO_DEDUPE, h, dtype=dtype)
                hs.device_synchronize()
                stats[key].append(M.edge_stats)
                return M
            return call

        arms = {"F64": arm("F64", np.float64), "F32": arm("F32", np.float32)}
        a, b = arms["F64"](), arms["F32"]()                       # the parity gate, before any timing
        try:
            if structure_differs(h, a, b):
                raise SystemExit("edges_f64_bench: the f64 CSR's structure differs from the f32 CSR's; no times written")
            shape = {"rows": a.rows, "nnz": a.nnz, "lines": a.edge_stats["lines"], "entries": a.edge_stats["entries"]}
        finally:
            a.deviceDispose(); b.deviceDispose()
        for s in stats.values():
            s.clear()
        times, _ = take_turns(arms, reps, warmup, timer=clock)
    h.close()
    out = {"m": A.rows, "nnz_written": A.nnz, "text_bytes": nbytes, "isTrans": True, "coo_flags": "DEDUPE",
           "values": "%.17g of the workload's values widened to double", **shape,
           "parity_rule": "the two device CSRs' indices through hip_csr_diff: same nnz, rows_len_differ == only_a == only_b == 0"}
    for key, t in times.items():
        st = stats[key][warmup:]
        coo = [w - s["ms_total"] for w, s in zip(t, st)]
        out[key] = {"wall_ms": {"ms": med(t), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "runs_ms": rounded(t)},
                    "coo_and_map_ms": {"ms": med(coo), "runs_ms": rounded(coo)},
                    "slow_lines": int(st[-1]["slow_lines"]), "slow_share": st[-1]["slow_lines"] / max(st[-1]["lines"], 1)}
        for p in PHASES:
            x = [float(s[p]) for s in st]
            out[key][p] = {"ms": med(x), "runs_ms": rounded(x)}
    return out


def main():
    ap = parser(__doc__, "edges_f64_bench")
    ap.add_argument("--workload", default="synth_1m_16", choices=sorted(WORKLOADS))
    args = ap.parse_args()
    need_device("edges_f64_bench")
    finish("edges_f64_bench", args, {args.workload: run(args.workload, args.reps, args.warmup)},
           timing="host clock around each call, ending in a device synchronise, median", dtype="float64 beside float32")


if __name__ == "__main__":
    main()
