#!/usr/bin/env python3
"""tools/dense_bench.py — the dense matrix on the device (hip_csr_to_dense, hip_dense_to_csr, hip_dense_gemm), timed.

    python tools/dense_bench.py [--reps 10] [--warmup 2] [--workload synth_1m_16] [--side 16384] [--gemm 4096] [--out FILE]

One process, device 0, float32 and float64.  Every time is the distance between two HIP events recorded on the handle's
stream around one blocking entry point (so it contains the call's own host read-backs: the validation flag, the scan
total), outputs freed outside the timed region; 2 warm-ups, median of 10, the arms taking turns.  Writes one JSON document
(default profiles/dense_bench.json).  Nothing is gated on speed.

parity gate  first, per value type.  Conversions: to_csr(to_dense(A), KEEP_ABS, tol 0) against A (row-sorted, no repeated
             column) through hip_csr_diff at abs_tol = rel_tol = 0: same nnz, rows_len_differ == only_a == only_b ==
             beyond == 0.  Product: I * B for an asymmetric 1024 x 1024 B must be B, and a 512 x 512 x 256 product of
             multiples of 2^-6 (every partial sum exact) must equal numpy's float64 product, both bit for bit.  If a gate
             fails the tool fails and writes no times.
to_dense     hip_csr_to_dense of the first `side` rows and columns of the workload into a resident side x side buffer
to_csr       hip_dense_to_csr (KEEP_ABS, tol 0) of that buffer
d2d          beside them: the dense buffer copied device to device on the same stream (the yardstick: one read and one
             write of every cell; to_dense writes every cell once, to_csr reads every cell twice)
gemm         hip_dense_gemm at `gemm`^3, uniform [-1, 1) operands, in TFLOP/s (2 * gemm^3 flop)
"""
import numpy as np

from benchkit import HIP_EVENTS, WORKLOADS, Events, finish, hs, load, med, need_device, parser, rounded, round_trip_differs, \
    take_turns

DTYPES = {"float32": np.float32, "float64": np.float64}


def corner(hA, side, dtype):
    """the first `side` rows and columns of host CSR hA, rows sorted, the first of a repeated column kept"""
    side = min(side, hA.rows)
    end = int(hA.rowPtr[side])
    rows = np.repeat(np.arange(side), np.diff(hA.rowPtr[:side + 1]))
    cols, vals = hA.colInd[:end], hA.values[:end]
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    keep = cols < side
    keep[1:] &= (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=side))])
    return hs.CSR.from_arrays(rp, cols[keep], vals[keep].astype(dtype), side, side, dtype=dtype)


def product_gate(h, dtype):
    n = 1024
    B = (np.arange(n, dtype=np.float64)[:, None] * n + np.arange(n)).astype(dtype)
    rng = np.random.default_rng(7)
    X, Y = (rng.integers(-256, 257, (512, 256)) / 64.0).astype(dtype), (rng.integers(-256, 257, (256, 512)) / 64.0).astype(dtype)
    for name, L, R, want in (("I * B", np.eye(n, dtype=dtype), B, B),
                             ("exact 512x512x256", X, Y, (X.astype(np.float64) @ Y.astype(np.float64) + 0.0).astype(dtype))):
        dL, dR = hs.DenseMatrix.from_host(L), hs.DenseMatrix.from_host(R)
        dP = dL.matmul(dR, h)
        try:
            if dP.download().tobytes() != want.tobytes():
                raise SystemExit(f"parity gate, {np.dtype(dtype).name} product {name}: the bits differ")
        finally:
            for d in (dL, dR, dP):
                d.dispose()


def conversions(h, ev, hA, side, dtype, reps, warmup):
    A = corner(hA, side, dtype)
    dA = A.toGpuCSR()
    item = np.dtype(dtype).itemsize
    nbytes = A.rows * A.cols * item
    buf, copy = hs.dev_alloc(nbytes), hs.dev_alloc(nbytes)
    try:
        hs.csr_to_dense_raw(h, A.rows, A.cols, dA.nnz, dA.rowPtr, dA.colInd, dA.values, buf, A.cols, dtype)
        ic, jc, cv, nnz = hs.dense_to_csr_raw(h, A.rows, A.cols, buf, A.cols, hs.DENSE_KEEP_ABS, 0.0, dtype)
        back = hs.CSR(cv, jc, ic, A.rows, A.cols, nnz, True, dtype=dtype)
        try:
            d = back.diff(dA, rel=0.0, abs=0.0, handle=h)
            if round_trip_differs(back, dA, d):
                raise SystemExit(f"parity gate, {np.dtype(dtype).name}: the round trip differs from the matrix: {d.as_dict()}")
        finally:
            back.deviceDispose()

        def to_csr():
            return list(hs.dense_to_csr_raw(h, A.rows, A.cols, buf, A.cols, hs.DENSE_KEEP_ABS, 0.0, dtype)[:3])
        arms = {"to_dense": lambda: hs.csr_to_dense_raw(h, A.rows, A.cols, dA.nnz, dA.rowPtr, dA.colInd, dA.values, buf, A.cols, dtype),
                "to_csr": to_csr, "d2d": lambda: ev.copy(copy, buf, nbytes)}
        times, _ = take_turns(arms, reps, warmup, timer=ev.ms)
    finally:
        hs.dev_free(buf)
        hs.dev_free(copy)
        dA.deviceDispose()
    out = {"side": A.rows, "nnz": A.nnz, "dense_bytes": nbytes}
    for name in arms:
        out[name + "_ms"] = med(times[name])
        out[name + "_runs_ms"] = rounded(times[name])
    for name in ("to_dense", "to_csr"):
        out[name + "_ms_over_d2d"] = round(out[name + "_ms"] / out["d2d_ms"], 3)
    out["d2d_GBps"] = round(2 * nbytes / out["d2d_ms"] / 1e6, 1)
    return out


def gemms(h, ev, n, reps, warmup):
    rng = np.random.default_rng(4096)
    mats = {}
    for name, dtype in DTYPES.items():
        L, R = (rng.random((n, n)) * 2 - 1).astype(dtype), (rng.random((n, n)) * 2 - 1).astype(dtype)
        mats[name] = (hs.DenseMatrix.from_host(L), hs.DenseMatrix.from_host(R), hs.DenseMatrix.zeros(n, n, dtype))
    arms = {name: (lambda a=a, b=b, c=c, dtype=DTYPES[name]: hs.dense_gemm_raw(h, n, n, n, a.values, n, b.values, n, c.values, n, dtype))
            for name, (a, b, c) in mats.items()}
    try:
        times, _ = take_turns(arms, reps, warmup, timer=ev.ms)
    finally:
        for trio in mats.values():
            for d in trio:
                d.dispose()
    out = {"m": n, "n": n, "k": n}
    for name in arms:
        out[name + "_ms"] = med(times[name])
        out[name + "_runs_ms"] = rounded(times[name])
        out[name + "_tflops"] = round(2.0 * n ** 3 / out[name + "_ms"] / 1e9, 2)
    return out


def run(name, side, gemm, reps, warmup):
    hA = load(name)
    h = hs.Handle(0)
    ev = Events(h.stream())
    try:
        for dtype in DTYPES.values():                              # every gate before any time
            product_gate(h, dtype)
        out = {"conversions": {n: conversions(h, ev, hA, side, dt, reps, warmup) for n, dt in DTYPES.items()}}
        out["gemm"] = gemms(h, ev, gemm, reps, warmup)
        out["parity_rule"] = ("to_csr(to_dense(A), KEEP_ABS, 0) against A through hip_csr_diff at tolerance 0; I * B == B and an "
                              "exact-sum product == numpy's float64 product, bit for bit")
    finally:
        ev.close()
        h.close()
    return out


def main():
    ap = parser(__doc__, "dense_bench")
    ap.add_argument("--workload", default="synth_1m_16", choices=sorted(WORKLOADS))
    ap.add_argument("--side", type=int, default=16384)
    ap.add_argument("--gemm", type=int, default=4096)
    args = ap.parse_args()
    need_device("dense_bench")
    finish("dense_bench", args, {args.workload: run(args.workload, args.side, args.gemm, args.reps, args.warmup)}, timing=HIP_EVENTS,
           dtype="float32, float64")


if __name__ == "__main__":
    main()
