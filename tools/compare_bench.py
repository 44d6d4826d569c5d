#!/usr/bin/env python3
"""tools/compare_bench.py — comparing two device CSRs on the device against the route a caller had before, timed.

    python tools/compare_bench.py [--reps 10] [--warmup 2] [--workloads synth_1m_16,web_google_surrogate] [--out FILE]

One process, device 0, float32.  Per workload C = A * A is computed and row-sorted on the device once; every time is a host
clock around blocking calls, 2 warm-ups, median of 10, the arms taking turns.  Writes one JSON document (default
profiles/compare_bench.json).  Nothing is gated on a time: the record is the deliverable.  The two routes must agree on
what they report before any time is written.

diff         hip_csr_diff(C, C') with rel = 1e-6 against the host route: both matrices downloaded (six arrays) and compared
             with the numpy restatement of the mirror's CSR::isParityEqual (rowPtr and colInd identical, values within
             1e-6 relative), its download and its compare also timed apart.  C' is C with one value in a thousand scaled
             by 1 + 1e-3 ("perturbed") and a bit-identical copy ("equal": the case the end-of-run check meets).
differsStats hip_csr_differsStats(A, C) with the reference's eight percents against the --stats route before it: the new
             matrix downloaded whole (three arrays, what a gpuRmclIter(1) per iteration through the host moves one way)
             and the host loop of CSR::differsStats restated in numpy; the rowPtr-only download is timed as well.
"""
import numpy as np

from benchkit import finish, hs, load, med, need_device, parser, rounded, take_turns

REF_PERCENTS = [-30, -20, -5, 0, 5, 20, 30, 100]


def summary(times):
    return {k: {"ms": med(v), "runs_ms": rounded(v)} for k, v in times.items()}


def host_parity(X, Y, rel):
    """the mirror's CSR::isParityEqual restated in numpy, without its early exit -> (same, entries beyond rel)"""
    if (X.rows, X.cols, X.nnz) != (Y.rows, Y.cols, Y.nnz):
        return False, -1
    if not np.array_equal(X.rowPtr, Y.rowPtr) or not np.array_equal(X.colInd, Y.colInd):
        return False, -1
    x, y = X.values.astype(np.float64), Y.values.astype(np.float64)
    beyond = int(np.count_nonzero(np.abs(x - y) > rel * np.maximum(np.abs(x), np.abs(y))))
    return beyond == 0, beyond


def host_differs_stats(arp, brp, percents):
    """CSR::differsStats (float QValue) over two host row pointers, vectorised"""
    n = len(percents)
    a, b = np.diff(arp).astype(np.int64), np.diff(brp).astype(np.int64)
    pc = np.asarray(percents, np.float32)
    counts = np.zeros(n + 4, np.int64)
    appeared, both_zero, equal = (a == 0) & (b > 0), (a == 0) & (b == 0), (a != 0) & (a == b)
    counts[n + 1], counts[n + 2], counts[n + 3] = appeared.sum(), both_zero.sum(), equal.sum()
    rest = ~(appeared | both_zero | equal)
    ratio = (b[rest] - a[rest]).astype(np.float32) / a[rest].astype(np.float32)
    below = ratio[:, None] < pc[None, :] if n else np.zeros((len(ratio), 0), bool)
    slot = np.where(below.any(axis=1), below.argmax(axis=1), n) if n else np.zeros(len(ratio), np.int64)
    counts[:n + 1] += np.bincount(slot, minlength=n + 1)
    return [int(x) for x in counts]


def diff_arms(h, dC, dOther, rel, reps, warmup):
    def device():
        return dC.diff(dOther, rel=rel, abs=0.0, handle=h)

    def download():
        return dC.toCpuCSR(), dOther.toCpuCSR()

    def host():
        return host_parity(*download(), rel)
    pair = download()
    # the arms' results are reports and host objects: nothing to free, the last of each is compared below
    times, last = take_turns({"hip_csr_diff": device, "download_and_host_compare": host, "download_only": download,
                              "host_compare_only": lambda: host_parity(pair[0], pair[1], rel)}, reps, warmup, free=None)
    d, (same, beyond) = last["hip_csr_diff"], last["download_and_host_compare"]
    device_same = d.rows_len_differ == 0 and d.only_a == 0 and d.only_b == 0 and d.beyond == 0
    if device_same != same:
        raise SystemExit(f"the two routes disagree: device beyond={d.beyond}, host beyond={beyond}")
    out = summary(times)
    out["report"] = d.as_dict()
    out["host_beyond_symmetric_rule"] = beyond
    out["device_over_host_route"] = round(out["hip_csr_diff"]["ms"] / out["download_and_host_compare"]["ms"], 4)
    return out


def run(name, reps, warmup):
    hA = load(name)
    m = hA.rows
    h = hs.Handle(0)
    dA = hA.toGpuCSR()
    made = [dA]
    try:
        dC = hs.gpuSpMMWrapper(dA, dA, h)
        made.append(dC)
        hs.sort_rows_device(dC, h)
        C = dC.toCpuCSR()
        rng = np.random.default_rng(7)
        vals = C.values.copy()
        hit = rng.random(C.nnz) < 1e-3
        vals[hit] = (vals[hit].astype(np.float64) * (1.0 + 1e-3)).astype(np.float32)
        dEqual = hs.CSR(hs.h2d(C.values), hs.h2d(C.colInd), hs.h2d(C.rowPtr), m, m, C.nnz, True)
        made.append(dEqual)
        dPert = hs.CSR(hs.h2d(vals), hs.h2d(C.colInd), hs.h2d(C.rowPtr), m, m, C.nnz, True)
        made.append(dPert)
        out = {"m": m, "nnzA": hA.nnz, "nnzC": C.nnz, "longest_row_of_C": int(np.diff(C.rowPtr).max()),
               "perturbed_entries": int(np.count_nonzero(vals != C.values))}
        out["diff_equal"] = diff_arms(h, dC, dEqual, 1e-6, reps, warmup)
        out["diff_perturbed"] = diff_arms(h, dC, dPert, 1e-6, reps, warmup)

        def stats_device():
            return dA.differsStats(dC, REF_PERCENTS, h)

        def stats_whole():
            new = dC.toCpuCSR()
            return host_differs_stats(hA.rowPtr, new.rowPtr, REF_PERCENTS)

        def stats_rowptr():
            return host_differs_stats(hA.rowPtr, hs.d2h(dC.rowPtr, m + 1, np.int32), REF_PERCENTS)
        times, last = take_turns({"hip_csr_differsStats": stats_device, "download_matrix_and_host_loop": stats_whole,
                                  "download_rowptr_and_host_loop": stats_rowptr}, reps, warmup, free=None)
        if not (last["hip_csr_differsStats"] == last["download_matrix_and_host_loop"] == last["download_rowptr_and_host_loop"]):
            raise SystemExit(f"differsStats: the routes disagree: {last}")
        out["differsStats"] = summary(times)
        out["differsStats"]["counts"] = last["hip_csr_differsStats"]
        out["differsStats"]["device_over_host_route"] = round(
            out["differsStats"]["hip_csr_differsStats"]["ms"] / out["differsStats"]["download_matrix_and_host_loop"]["ms"], 4)
    finally:
        for d in made:
            d.deviceDispose()
        h.close()
    return out


def main():
    ap = parser(__doc__, "compare_bench")
    ap.add_argument("--workloads", default="synth_1m_16,web_google_surrogate")
    args = ap.parse_args()
    need_device("compare_bench")
    finish("compare_bench", args, {name: run(name, args.reps, args.warmup) for name in args.workloads.split(",")})   # the routes agreed


if __name__ == "__main__":
    main()
