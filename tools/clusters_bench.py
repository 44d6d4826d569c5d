#!/usr/bin/env python3
"""tools/clusters_bench.py — clusters out of an R-MCL result: the download plus a host union-find against the device entries.

    python tools/clusters_bench.py [--procs 3] [--reps 5] [--warmup 2] [--dir /dev/shm] [--out FILE]

Two inputs, float32, device 0:
  rmcl_500k     the R-MCL result after ten device iterations on the 500 000-node graph of bench.py's rmcl_500k (`flow`:
                hip_rmcl_attractors, hip_csr_connected_components on i -> parent[i], hip_labels_to_clusters, and the chain
                hip_rmcl_clusters)
  forest_1m     a random forest of 1 048 576 vertices with scrambled ids, about 1 000 trees, every edge stored once
                (`graph`: hip_csr_connected_components on the pattern, hip_labels_to_clusters)
Each input is made once and handed to the measuring processes as a binary file; making it is outside every timed region.
One FRESH process per measurement (the C++ driver tests/cpp/clusters_check.x bench), --procs of them per input, each with
--warmup untimed rounds and --reps rounds in which the arms take turns, every arm under the host clock around blocking
calls:
  host          what a user does today: CSR::toCpuCSR, then argmax per row (flow only), a union-find, the numbering
  device        each entry on the matrix where it already is
Parity gate in every process: labels and cluster numbers of the two ways are equal, or the tool fails and writes no times.
Reported: the median over the processes of each process's median for every arm, the rounds the components took, and
host / device for the whole way (flow: against hip_rmcl_clusters; graph: against components + labels_to_clusters).
Writes one JSON document (default profiles/clusters_bench.json).  Nothing is gated on speed.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

from benchkit import ROOT, finish, hs, med, need_device, parser

sys.path.insert(0, os.path.join(ROOT, "tests"))
CPP = os.path.join(ROOT, "tests", "cpp")
ARMS = ("host_ms", "attractors_ms", "components_ms", "labels_to_clusters_ms", "rmcl_clusters_ms")


def rmcl_500k():
    """Mt after ten device iterations from the R-MCL start matrix of the 500 000-node power-law graph (seed 45)"""
    from helpers import po, synth_csr
    A = synth_csr(500000, 45, 2)
    ri = np.repeat(np.arange(A.rows, dtype=np.int32), np.diff(A.rowPtr))
    M0 = po.rmcl_init(A.rows, A.cols, A.colInd, ri, np.ones_like(A.values))
    d0 = hs.CSR.from_arrays(M0.rowPtr, M0.colInd, M0.values, M0.rows, M0.cols).toGpuCSR()
    dMt = hs.gpuRmclIter_device(10, d0, d0)
    Mt = dMt.toCpuCSR()
    dMt.deviceDispose()
    d0.deviceDispose()
    return Mt


def forest_1m():
    """every vertex but about one in a thousand hangs under a random vertex below it; ids scrambled; edges stored once"""
    n = 1 << 20
    rng = np.random.default_rng(7)
    up = (rng.random(n) * np.arange(n)).astype(np.int64)
    keep = (rng.random(n) > 0.001) & (np.arange(n) > 0)
    p = rng.permutation(n)
    src, dst = p[np.arange(n)[keep]], p[up[keep]]
    order = np.argsort(src, kind="stable")
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(src, minlength=n), out=rp[1:])
    return hs.CSR.from_arrays(rp, dst[order], np.ones(len(src), np.float32), n, n)


INPUTS = {"rmcl_500k": ("flow", rmcl_500k), "forest_1m": ("graph", forest_1m)}


def dump(M, path):
    with open(path, "wb") as f:
        np.array([M.rows, M.cols, M.nnz], np.int32).tofile(f)
        np.ascontiguousarray(M.rowPtr, np.int32).tofile(f)
        np.ascontiguousarray(M.colInd, np.int32).tofile(f)
        np.ascontiguousarray(M.values, np.float32).tofile(f)


def measure(kind, binpath, procs, reps, warmup):
    runs = []
    for _ in range(procs):
        r = subprocess.run([os.path.join(CPP, "clusters_check.x"), "bench", kind, binpath, str(warmup), str(reps)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("clusters_check.x bench failed (the parity gate, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"{os.path.basename(binpath)}: host {med(runs[-1]['host_ms'])} ms, rounds {runs[-1]['rounds']}", file=sys.stderr,
              flush=True)
    res = {k: runs[0][k] for k in ("rows", "nnz", "clusters", "components")}
    res["rounds"] = sorted({p["rounds"] for p in runs})
    for key in ARMS:
        if runs[0][key]:
            per_proc = [med(p[key]) for p in runs]
            res[key] = {"ms": med(per_proc), "per_process_ms": per_proc, "runs_ms": [p[key] for p in runs]}
    device = res["rmcl_clusters_ms"]["ms"] if kind == "flow" else res["components_ms"]["ms"] + res["labels_to_clusters_ms"]["ms"]
    res["device_whole_way_ms"] = round(device, 4)
    res["host_over_device"] = round(res["host_ms"]["ms"] / device, 2) if device else None
    return res


def main():
    ap = parser(__doc__, "clusters_bench")
    ap.set_defaults(reps=5, warmup=2)
    ap.add_argument("--procs", type=int, default=3, help="fresh processes per input")
    ap.add_argument("--dir", default="/dev/shm", help="where the binary inputs are written")
    ap.add_argument("--workload", action="append", choices=sorted(INPUTS))
    args = ap.parse_args()
    need_device("clusters_bench")
    subprocess.check_call(["make", "-s", "-f", "clusters.mk", "-C", CPP, "clusters_check.x"])
    out = {}
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        for name in args.workload or ["rmcl_500k", "forest_1m"]:
            kind, make = INPUTS[name]
            binpath = os.path.join(d, name + ".bin")
            dump(make(), binpath)
            out[name] = measure(kind, binpath, args.procs, args.reps, args.warmup)
            os.remove(binpath)
    finish("clusters_bench", args, out, timing="host clock around each arm (blocking calls); median over fresh processes of "
           "each process's median", dtype="float32", procs=args.procs)


if __name__ == "__main__":
    main()
