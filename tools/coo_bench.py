"""COO -> CSR on the device (hip_coo_to_csr) on the edge list of the 1M-row workload in shuffled order, device arrays in
and out, against the CPU restatement of the reference's std::sort path (oracle).

    python tools/coo_bench.py [--reps 10] [--warmup 2] [--no-cpu] [--out FILE]
"""
import json, os, sys
import numpy as np
from benchkit import HOST_CLOCK, ROOT, WORKLOADS, clock, hs, med, need_device, parser, release, rounded
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import po

ap = parser(__doc__, "coo_bench")
ap.set_defaults(out=None)                                   # this tool prints; --out FILE also writes the times as JSON
ap.add_argument("--no-cpu", action="store_true", help="skip the one-thread CPU oracle")
args = ap.parse_args()
need_device("coo_bench")

rp, ci, v = WORKLOADS["synth_1m_16"]()
m = len(rp) - 1
ri = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
perm = np.random.default_rng(1).permutation(len(ci))
ri, ci, v = ri[perm], ci[perm], v[perm]
n = len(ci)
h = hs.Handle(0)
dr, dc, dv = hs.h2d(ri), hs.h2d(ci), hs.h2d(v)
res = {"tool": "coo_bench", "timing": HOST_CLOCK, "reps": args.reps, "warmup": args.warmup,
       "m": m, "entries": n, "calls": {}}
for flags, tag in ((hs.COO_DEDUPE, "sort+dedupe+toCSR"), (hs.COO_SELF_LOOPS | hs.COO_ROW_NORMALISE, "rmclInit")):
    runs = []
    for it in range(args.warmup + args.reps):
        ms, (ia, ja, av, nn) = clock(lambda: hs.coo_to_csr_raw(h, m, m, n, dr, dc, dv, flags))
        release([ia, ja, av])
        if it >= args.warmup:
            runs.append(ms)
    mid = float(np.median(runs))
    res["calls"][tag] = {"ms": med(runs), "runs_ms": rounded(runs), "nnz_out": int(nn)}
    print(f"device {tag:20s} {n} entries -> {nn}: {mid:7.2f} ms  ({n/mid/1e3:7.1f} M entries/s, {n*12*2/mid/1e6:6.1f} GB/s of the 12 B/entry in + out)")
if not args.no_cpu:
    cpu_ms, W = clock(lambda: po.coo_to_csr(m, m, ri, ci, v, dedupe=True))
    res["cpu_oracle_ms"] = round(cpu_ms, 1)
    print(f"CPU oracle (qsort of tuples, 1 thread) sort+dedupe+toCSR: {cpu_ms:7.1f} ms ({n/cpu_ms/1e3:5.1f} M entries/s)")
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
