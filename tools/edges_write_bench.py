#!/usr/bin/env python3
"""tools/edges_write_bench.py — a device CSR to an edge-list file: the download plus the host's printf loop against the
text written on the device.

    python tools/edges_write_bench.py [--procs 5] [--reps 2] [--warmup 1] [--dir /dev/shm] [--out FILE]

Two matrices, float32, device 0, both formats (FIXED6 "%d\\t%d\\t%.6lf", ROUNDTRIP "%d %d %.9g"), files under --dir:
  synth_1m_16   the headline matrix (1 048 576 rows, 15.6 M entries)
  rmcl_500k     the R-MCL result after ten device iterations on the 500 000-node graph of bench.py's rmcl_500k
Each matrix is made once and handed to the measuring processes as a binary file; making it is outside every timed region.
One FRESH process per measurement (the C++ driver tests/cpp/edges_write_check.x bench), --procs of them per matrix and
format, each with --warmup untimed rounds and --reps rounds of the two arms taking turns:
  arm A   what the parent commit can do: CSR::toCpuCSR, then one fprintf per entry, single-threaded (the mirror's loop)
  arm B   gpuWriteCSRWrapper = hip_write_edge_file: length pass, scan, write pass, download through the pinned lanes,
          fwrite beside the next slab's formatting
Parity gate in every process: the two files are equal byte for byte, or the tool fails and writes no times.
Reported: the median over the processes of each process's median, for both arms and for arm B's phases
(spgemm_edge_write_stats); the ratio A / B; the slowest phase of B; the format kernels' bytes per second (what they must
read and write: 2 (4 (m + 1) + 8 nnz) for the two passes + 2 nnz length bytes + the text, over ms_length + ms_write) against the 8 TB/s of
HBM, and the download's against the 63 GB/s of the host link.  Writes one JSON document (default
profiles/edges_write_bench.json).  Nothing is gated on speed.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

from benchkit import ROOT, finish, hs, load, med, need_device, parser

sys.path.insert(0, os.path.join(ROOT, "tests"))
CPP = os.path.join(ROOT, "tests", "cpp")
HBM_GBS, LINK_GBS = 8000.0, 63.0
FORMATS = {"FIXED6": 0, "ROUNDTRIP": 1}
PHASES = ("ms_length", "ms_scan", "ms_write", "ms_slow", "ms_download", "ms_file")


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


def dump(M, path):
    with open(path, "wb") as f:
        np.array([M.rows, M.cols, M.nnz], np.int32).tofile(f)
        np.ascontiguousarray(M.rowPtr, np.int32).tofile(f)
        np.ascontiguousarray(M.colInd, np.int32).tofile(f)
        np.ascontiguousarray(M.values, np.float32).tofile(f)


def measure(binpath, out, fmt, procs, reps, warmup):
    runs = []
    for _ in range(procs):
        r = subprocess.run([os.path.join(CPP, "edges_write_check.x"), "bench", binpath, out, str(fmt), str(warmup), str(reps)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("edges_write_check.x bench failed (the parity gate, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"{os.path.basename(binpath)} fmt={fmt}: host {med(runs[-1]['host_arm_ms'])} ms, device {med(runs[-1]['device_arm_ms'])} ms",
              file=sys.stderr, flush=True)
    res = {k: runs[0][k] for k in ("rows", "nnz", "bytes", "slabs", "slow_entries")}
    for key in ("host_arm_ms", "device_arm_ms", "ms_total") + PHASES:
        per_proc = [med(p[key]) for p in runs]
        res[key] = {"ms": med(per_proc), "per_process_ms": per_proc, "runs_ms": [p[key] for p in runs]}
    return derive(res)


def derive(res):
    """the figures computed from the recorded times: ratio, slowest phase, rates"""
    a, b = res["host_arm_ms"]["ms"], res["device_arm_ms"]["ms"]
    res["host_over_device"] = round(a / b, 2) if b else None
    res["slowest_phase"] = max(PHASES, key=lambda k: res[k]["ms"])
    # each of the two passes reads rowPtr, colInd and values; the length bytes are written once and read once; the text is
    # written once
    kernel_bytes = 2 * (4 * (res["rows"] + 1) + 8 * res["nnz"]) + 2 * res["nnz"] + res["bytes"]
    kms = res["ms_length"]["ms"] + res["ms_write"]["ms"]
    res["format_kernels"] = {"bytes": kernel_bytes, "ms": round(kms, 4), "GBs": round(kernel_bytes / kms / 1e6, 1) if kms else None,
                             "share_of_hbm": round(kernel_bytes / kms / 1e6 / HBM_GBS, 4) if kms else None}
    dms = res["ms_download"]["ms"]
    res["download"] = {"bytes": res["bytes"], "ms": dms, "GBs": round(res["bytes"] / dms / 1e6, 1) if dms else None,
                       "share_of_link": round(res["bytes"] / dms / 1e6 / LINK_GBS, 4) if dms else None}
    res["file_write_GBs"] = round(res["bytes"] / res["ms_file"]["ms"] / 1e6, 2) if res["ms_file"]["ms"] else None
    return res


def main():
    ap = parser(__doc__, "edges_write_bench")
    ap.set_defaults(reps=2, warmup=1)
    ap.add_argument("--procs", type=int, default=5, help="fresh processes per matrix and format")
    ap.add_argument("--dir", default="/dev/shm", help="where the files are written")
    ap.add_argument("--workload", action="append", choices=["synth_1m_16", "rmcl_500k"])
    args = ap.parse_args()
    need_device("edges_write_bench")
    subprocess.check_call(["make", "-s", "-f", "edges_write.mk", "-C", CPP, "edges_write_check.x"])
    out = {}
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        for name in args.workload or ["synth_1m_16", "rmcl_500k"]:
            M = rmcl_500k() if name == "rmcl_500k" else load(name)
            binpath = os.path.join(d, name + ".bin")
            dump(M, binpath)
            out[name] = {fname: measure(binpath, os.path.join(d, name + ".txt"), fmt, args.procs, args.reps, args.warmup)
                         for fname, fmt in FORMATS.items()}
            os.remove(binpath)
    finish("edges_write_bench", args, out, timing="host clock around each arm (both end with the file closed); arm B's "
           "kernel phases from HIP events; median over fresh processes of each process's median", dtype="float32",
           procs=args.procs, directory=args.dir, hbm_peak_GBs=HBM_GBS, link_peak_GBs=LINK_GBS)


if __name__ == "__main__":
    main()
