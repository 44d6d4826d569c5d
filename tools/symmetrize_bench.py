#!/usr/bin/env python3
"""tools/symmetrize_bench.py — making a directed graph undirected: the device entries against the host round trip.

    python tools/symmetrize_bench.py [--procs 3] [--reps 5] [--warmup 2] [--workloads synth_1m_16,web_google_surrogate] [--out FILE]

float32, device 0, the matrix resident on the device, rows strictly ascending (as synth makes them).  One FRESH process per
measurement (this file with --child), --procs of them per workload, each with --warmup untimed rounds and --reps rounds in
which the arms take turns, every arm under the host clock around blocking calls, results freed outside the timed region:
  add         hip_csr_add(1, A, 1, A^T) alone, A^T made before the loop
  symmetrize  hip_csr_symmetrize(SUM) as a whole: the validation, hip_csr_transpose, hip_csr_add
  transpose   hip_csr_transpose of the same matrix: the yardstick (the add reads and writes the same order of bytes)
  host        what a user does today: CSR::toCpuCSR, a numpy merge of the entries of A and A^T (one stable sort of the
              2 nnz keys, equal neighbours summed), CSR::toGpuCSR
Parity gate in every process, before anything is timed: the device result equals the host route's, rowPtr, columns and
value bits, or the tool fails and writes no times.  Reported: the median over the processes of each process's median
for every arm, the algorithmic bytes of the add and of the transpose (inputs read once, outputs written once), add /
transpose, and host / symmetrize.  Writes one JSON document (default profiles/symmetrize_bench.json).  Nothing is gated on
speed.
"""
import json
import subprocess
import sys

import numpy as np

from benchkit import WORKLOADS, clock, finish, hs, load, med, need_device, parser, release, rounded, take_turns

ARMS = ("add", "symmetrize", "transpose", "host")


def host_merge(hA):
    """A + A^T of a host CSR by one stable sort of the keys of A's entries and of their mirror images"""
    m = hA.rows
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(hA.rowPtr))
    col = hA.colInd.astype(np.int64)
    keys = np.concatenate([row * m + col, col * m + row])
    vals = np.concatenate([hA.values, hA.values])
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    first = np.ones(len(keys), bool)
    first[1:] = keys[1:] != keys[:-1]
    out = vals[first]
    slot = np.cumsum(first) - 1
    out[slot[~first]] += vals[~first]                       # a key occurs at most twice: rows are strictly ascending
    keys = keys[first]
    rp = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(keys // m, minlength=m), out=rp[1:])
    return hs.CSR.from_arrays(rp, (keys % m).astype(np.int32), out, m, m)


def host_route(dA):
    """what a user does today: download, merge on the host, upload"""
    return host_merge(dA.toCpuCSR()).toGpuCSR()


def same_bits(dX, dY):
    X, Y = dX.toCpuCSR(), dY.toCpuCSR()
    return (X.nnz == Y.nnz and np.array_equal(X.rowPtr, Y.rowPtr) and np.array_equal(X.colInd, Y.colInd) and
            X.values.tobytes() == Y.values.tobytes())


def child(name, reps, warmup):
    hA = load(name)
    h = hs.Handle(0)
    dA = hA.toGpuCSR()
    dT = dA.transpose(h)
    try:
        # the parity gate: the whole entry, and the add alone, against the host route
        want = host_route(dA)
        for what, got in (("hip_csr_symmetrize(SUM)", dA.symmetrize(hs.SYM_SUM, handle=h)), ("hip_csr_add(A, A^T)", dA.add(dT, handle=h))):
            same = same_bits(got, want)
            nnzS = got.nnz
            got.deviceDispose()
            if not same:
                want.deviceDispose()
                raise SystemExit(f"parity gate: {what} and the host route disagree on {name}")
        want.deviceDispose()
        arms = {
            "add": lambda: dA.add(dT, handle=h),
            "symmetrize": lambda: dA.symmetrize(hs.SYM_SUM, handle=h),
            "transpose": lambda: dA.transpose(h),
            "host": lambda: host_route(dA),
        }
        t, _ = take_turns(arms, reps, warmup, timer=clock, free=release)
    finally:
        dT.deviceDispose()
        dA.deviceDispose()
        h.close()
    print(json.dumps({"m": hA.rows, "nnzA": hA.nnz, "nnzS": nnzS, "longest_row": int(np.diff(hA.rowPtr).max()),
                      **{k + "_ms": rounded(v) for k, v in t.items()}}))


def measure(name, procs, reps, warmup):
    runs = []
    for _ in range(procs):
        r = subprocess.run([sys.executable, __file__, "--child", name, "--reps", str(reps), "--warmup", str(warmup)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("a measuring process failed (the parity gate, or an error):\n" + r.stdout[-2000:] + r.stderr[-2000:])
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"{name}: " + ", ".join(f"{k} {med(runs[-1][k + '_ms'])} ms" for k in ARMS), file=sys.stderr, flush=True)
    res = {k: runs[0][k] for k in ("m", "nnzA", "nnzS", "longest_row")}
    for k in ARMS:
        per_proc = [med(p[k + "_ms"]) for p in runs]
        res[k] = {"ms": med(per_proc), "per_process_ms": per_proc, "runs_ms": [p[k + "_ms"] for p in runs]}
    m, nnz, nnzS = res["m"], res["nnzA"], res["nnzS"]
    # inputs read once, outputs written once (int32 indices, float32 values); the add reads A and A^T and writes S
    res["add"]["bytes"] = 2 * (4 * (m + 1) + 8 * nnz) + 4 * (m + 1) + 8 * nnzS
    res["transpose"]["bytes"] = 2 * (4 * (m + 1) + 8 * nnz)
    for k in ("add", "transpose"):
        res[k]["GBps"] = round(res[k]["bytes"] / (res[k]["ms"] * 1e-3) / 1e9, 1)
    res["add_over_transpose"] = round(res["add"]["ms"] / res["transpose"]["ms"], 3)
    res["host_over_symmetrize"] = round(res["host"]["ms"] / res["symmetrize"]["ms"], 2)
    return res


def main():
    ap = parser(__doc__, "symmetrize_bench")
    ap.set_defaults(reps=5, warmup=2)
    ap.add_argument("--procs", type=int, default=3, help="fresh processes per workload")
    ap.add_argument("--workloads", default="synth_1m_16,web_google_surrogate")
    ap.add_argument("--child", choices=sorted(WORKLOADS), help="(internal) measure one workload in this process")
    args = ap.parse_args()
    need_device("symmetrize_bench")
    if args.child:
        return child(args.child, args.reps, args.warmup)
    out = {name: measure(name, args.procs, args.reps, args.warmup) for name in args.workloads.split(",")}
    finish("symmetrize_bench", args, out, timing="host clock around each arm (blocking calls); median over fresh processes of "
           "each process's median", dtype="float32", procs=args.procs,
           parity="device result bit-equal to the host route in every process")


if __name__ == "__main__":
    main()
