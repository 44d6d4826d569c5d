"""COO -> CSR on the device (hip_coo_to_csr) on the edge list of the 1M-row workload in shuffled order, device arrays in
and out, against the CPU restatement of the reference's std::sort path (oracle).

    python tools/coo_bench.py [--reps 10] [--warmup 2] [--no-cpu] [--out FILE]
"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import po
from sparse_matrix_with_flops_amd import hipspgemm as hs, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-cpu", action="store_true", help="skip the one-thread CPU oracle")
ap.add_argument("--out", default=None, help="write the times as JSON")
args = ap.parse_args()

m = 1 << 20
rp, ci, v = synth.powerlaw_csr(m, 43, 2)[:3]
ri = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
perm = np.random.default_rng(1).permutation(len(ci))
ri, ci, v = ri[perm], ci[perm], v[perm]
n = len(ci)
h = hs.Handle(0)
dr, dc, dv = hs.h2d(ri), hs.h2d(ci), hs.h2d(v)
res = {"tool": "coo_bench", "timing": "host clock around blocking calls, median", "reps": args.reps, "warmup": args.warmup,
       "m": m, "entries": n, "calls": {}}
for flags, tag in ((hs.COO_DEDUPE, "sort+dedupe+toCSR"), (hs.COO_SELF_LOOPS | hs.COO_ROW_NORMALISE, "rmclInit")):
    runs = []
    for it in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        ia, ja, av, nn = hs.coo_to_csr_raw(h, m, m, n, dr, dc, dv, flags)
        dt = time.perf_counter() - t0
        for p in (ia, ja, av):
            hs.dev_free(p)
        if it >= args.warmup:
            runs.append(dt * 1e3)
    med = float(np.median(runs))
    res["calls"][tag] = {"ms": round(med, 4), "runs_ms": [round(x, 4) for x in runs], "nnz_out": int(nn)}
    print(f"device {tag:20s} {n} entries -> {nn}: {med:7.2f} ms  ({n/med/1e3:7.1f} M entries/s, {n*12*2/med/1e6:6.1f} GB/s of the 12 B/entry in + out)")
if not args.no_cpu:
    t0 = time.perf_counter()
    W = po.coo_to_csr(m, m, ri, ci, v, dedupe=True)
    cpu = time.perf_counter() - t0
    res["cpu_oracle_ms"] = round(cpu * 1e3, 1)
    print(f"CPU oracle (qsort of tuples, 1 thread) sort+dedupe+toCSR: {cpu*1e3:7.1f} ms ({n/cpu/1e6:5.1f} M entries/s)")
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
