#!/usr/bin/env python3
"""tools/edges_bench.py — an edge-list file to a device CSR: the host threads' parse against the parse on the device.

    python tools/edges_bench.py [--reps 10] [--warmup 2] [--workload synth_1m_16] [--out FILE]

One process per measurement (the C++ driver tests/cpp/edges_check.x bench), device 0, float32.  The workload's edge list
is written as text in shuffled order -- every third line "from to %.7g", the others "from to" -- with a "rows nnz" size
line; writing it is outside the timed region.
  arm A   COO::readSNAPFile (all host threads: strtol / strtof) + COO::toGpuCSR(DEDUPE): three arrays go up
  arm B   COO::readSNAPFileToGpuCSR(DEDUPE): the text goes up, hip_parse_edge_text + hip_coo_to_csr
Parity gate first: both device CSRs equal through hip_csr_diff at zero tolerances, or the tool fails and writes no times.
Then 2 warm-ups and the arms taking turns, median of 10 with the runs kept; wall clock around each arm ending in a device
synchronise, plus the phases spgemm_edge_stats reports for arm B.  Both arms read the file from the page cache.
Writes one JSON document (default profiles/edges_bench.json).  Nothing is gated on speed.
"""
import json
import os
import subprocess
import tempfile

import numpy as np

from benchkit import ROOT, WORKLOADS, finish, hs, load, med, need_device, parser

CPP = os.path.join(ROOT, "tests", "cpp")


def write_edge_list(path, A, seed=5):
    """the CSR's entries as "row col [value]" lines in shuffled order behind a "rows nnz" size line"""
    rng = np.random.default_rng(seed)
    ri = np.repeat(np.arange(A.rows, dtype=np.int64), np.diff(A.rowPtr.astype(np.int64)))
    order = rng.permutation(A.nnz)
    ri, ci, v = ri[order], A.colInd[order], A.values[order]
    with open(path, "w") as f:
        f.write(f"# {A.rows} rows, {A.nnz} entries, shuffled\n{A.rows} {A.nnz}\n")
        step = 1 << 20
        for lo in range(0, A.nnz, step):
            f.write("".join(f"{r} {c} {x:.7g}\n" if (lo + i) % 3 == 0 else f"{r} {c}\n"
                            for i, (r, c, x) in enumerate(zip(ri[lo:lo + step].tolist(), ci[lo:lo + step].tolist(),
                                                              v[lo:lo + step].tolist()))))
    return os.path.getsize(path)


def run(name, reps, warmup):
    A = load(name)
    subprocess.check_call(["make", "-s", "-f", "edges.mk", "-C", CPP, "edges_check.x"])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, name + ".snap")
        nbytes = write_edge_list(path, A)
        r = subprocess.run([os.path.join(CPP, "edges_check.x"), "bench", path, "1", str(hs.COO_DEDUPE), str(warmup), str(reps)],
                           capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("edges_check.x bench failed (the parity gate, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    out = {"m": A.rows, "nnz_written": A.nnz, "text_bytes": nbytes, "isTrans": True, "coo_flags": "DEDUPE"}
    for key in ("rows", "nnz", "lines", "entries", "slow_lines", "host_threads"):
        out[key] = res[key]
    for key in ("host_arm_ms", "host_arm_read_parse_ms", "device_arm_ms", "ms_upload", "ms_split", "ms_parse", "ms_slow", "ms_total"):
        t = res[key]
        out[key] = {"ms": med(t), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "runs_ms": t}
    out["parity_rule"] = "both device CSRs through hip_csr_diff at tolerance 0: same nnz, rows_len_differ == only_a == only_b == beyond == 0"
    return out


def main():
    ap = parser(__doc__, "edges_bench")
    ap.add_argument("--workload", default="synth_1m_16", choices=sorted(WORKLOADS))
    args = ap.parse_args()
    need_device("edges_bench")
    finish("edges_bench", args, {args.workload: run(args.workload, args.reps, args.warmup)},
           timing="host clock around each arm, ending in a device synchronise, median", dtype="float32")


if __name__ == "__main__":
    main()
