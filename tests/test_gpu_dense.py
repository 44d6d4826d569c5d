"""GPU (-m gpu): the dense matrix -- hip_csr_to_dense, hip_dense_to_csr, hip_dense_gemm and their _f64 twins.  The two
conversions move values and compute nothing, so they are compared on bits with the restatement tests/dense_ref.py (pinned
by hand in tests/test_dense_abi.py); float64 values carry bits beyond float32 (x + 2^-40), so a pass through float would
show.  The product is compared bit for bit where every partial sum is exact, and against the bound of a length-k chain
otherwise; the float fmaf-chain claim is tests/cpp/dense_check.cc part (c)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import dense_ref as dr
import reorder_ref as rr
from dense_ref import BK, BM, BN, CP_TILE, RS_TILE, SEG
from devcsr import built_gpu, handle  # noqa: F401
from devcsr import _plain, _special, assert_bits, one_long_row, take, typed, typed_plain, with_nnz
from helpers import DATA, GOLDEN, ROOT, po, random_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
ERR_OVERFLOW, ERR_INPUT = 3, 5
RULES = [(dr.KEEP_REFERENCE, 0.0), (dr.KEEP_REFERENCE, 1e-8), (dr.KEEP_ABS, 0.0), (dr.KEEP_ABS, 1e-8)]
PAD = 3


# ---- device buffers with a leading dimension ---------------------------------------------------------------------------
def sentinel(dtype):
    return np.dtype(dtype).type(-77.25)


def padded(D, ld, fill):
    """host image of a rows x ld buffer: D in [:, :cols], `fill` in the padding"""
    out = np.full((D.shape[0], ld), fill, D.dtype)
    out[:, :D.shape[1]] = D
    return out


def fetch(ptr, rows, ld, dtype):
    return hs.d2h(ptr, rows * ld, dtype).reshape(rows, ld)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def dense_of(handle, dM, ld, dtype):
    """hip_csr_to_dense into a sentinel-filled rows x ld buffer -> the whole buffer on the host"""
    buf = hs.h2d(np.full((dM.rows, ld), sentinel(dtype), dtype))
    try:
        hs.csr_to_dense_raw(handle, dM.rows, dM.cols, dM.nnz, dM.rowPtr, dM.colInd, dM.values, buf, ld, dtype)
        return fetch(buf, dM.rows, ld, dtype)
    finally:
        hs.dev_free(buf)


def csr_of(handle, D, ld, rule, tol):
    """hip_dense_to_csr of the host array D, uploaded with leading dimension ld (NaN in the padding: it must not be read
    as a cell, the reference rule would keep it)"""
    buf = hs.h2d(padded(D, ld, np.nan))
    try:
        ic, jc, cv, nnz = hs.dense_to_csr_raw(handle, D.shape[0], D.shape[1], buf, ld, rule, tol, D.dtype)
        return take(hs.CSR(cv, jc, ic, D.shape[0], D.shape[1], nnz, True, dtype=D.dtype))
    finally:
        hs.dev_free(buf)


# ---- inputs (made once, never modified) --------------------------------------------------------------------------------
def _cases():
    out = {"0x0": rr.Host(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 0, 0),
           "5x7 empty": rr.Host(np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 7),
           "1000x257": _plain(random_csr(1000, 257, 0.02, 1, sorted_rows=False)),
           "257x1000": _plain(random_csr(257, 1000, 0.02, 2, sorted_rows=False)),
           "long row": one_long_row()}
    for nnz in sorted({CP_TILE - 1, CP_TILE, CP_TILE + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1}):
        out[f"nnz {nnz}"] = with_nnz(61, 97, nnz, nnz)
        out[f"nnz {nnz} sorted"] = _dedupe(rr.sort_rows(out[f"nnz {nnz}"]))      # the direct scatter at the same sizes
    return out


def _dedupe(S):
    """a row-sorted matrix without its repeated columns (the first of each run stays)"""
    rows = np.repeat(np.arange(S.rows), np.diff(S.rowPtr))
    keep = np.ones(S.nnz, bool)
    keep[1:] = (rows[1:] != rows[:-1]) | (S.colInd[1:] != S.colInd[:-1])
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=S.rows))])
    return rr.Host(rp, S.colInd[keep], S.values[keep], S.rows, S.cols)


CASES = _cases()
REPEATS = ["long row"] + [f"nnz {x}" for x in (CP_TILE + 1, RS_TILE + 1)]
WANT_DENSE = {}


def want_dense(name, dtype):
    """the restatement's dense form of a case, computed once per (case, dtype)"""
    key = (name, np.dtype(dtype).name)
    if key not in WANT_DENSE:
        WANT_DENSE[key] = dr.to_dense(typed(CASES[name], dtype))
    return WANT_DENSE[key]


# shapes of the dense -> CSR walk: one row of many segments, one cell per row, rows one below / at / one above a segment,
# rows that end inside a 64-cell step, a ragged last segment
DENSE_SHAPES = [(1, 3 * SEG + 1), (3 * SEG + 1, 1), (3, SEG - 1), (3, SEG), (3, SEG + 1), (5000, 3), (300, 63), (300, 64),
                (300, 65), (7, 2 * SEG + 5), (2, SEG // 2 + 1)]


def dense_input(rows, cols, dtype, seed):
    """about a third of the cells hold a value: plain ones of both signs (with bits beyond float32 in float64), the special
    values, and tiny ones around the tolerance"""
    rng = np.random.default_rng(seed)
    D = np.zeros((rows, cols), dtype)
    mask = rng.random((rows, cols)) < 0.3
    v = (rng.random(int(mask.sum())) + 0.25) * rng.choice([-1.0, 1.0], int(mask.sum()))
    if np.dtype(dtype) == np.float64:
        v = v + 2.0 ** -40
    D[mask] = v.astype(dtype)
    flat = D.reshape(-1)
    sp = list(_special(dtype).values()) + [np.dtype(dtype).type(1e-8), np.nextafter(np.dtype(dtype).type(1e-8), np.dtype(dtype).type(1)),
                                           np.dtype(dtype).type(-1e-8)]
    where = rng.integers(0, flat.size, size=min(flat.size, 4 * len(sp)))
    for q, at in enumerate(where):
        flat[at] = sp[q % len(sp)]
    flat[0], flat[-1] = np.dtype(dtype).type(2.5), np.dtype(dtype).type(3.5)     # the first and the last cell are kept
    return D


# ---- conversions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_csr_to_dense_and_back_match_the_restatement(handle, name, dtype):
    M = typed(CASES[name], dtype)
    want = want_dense(name, dtype)
    dM = M.toGpuCSR()
    try:
        for ld in (M.cols, M.cols + PAD):
            got = dense_of(handle, dM, ld, dtype)
            assert same_bytes(got[:, :M.cols], want), f"{name} ld={ld}: dense cells"
            assert np.all(got[:, M.cols:] == sentinel(dtype)), f"{name} ld={ld}: padding was written"
            for rule, tol in RULES:
                assert_bits(csr_of(handle, want, ld, rule, tol), dr.to_csr(want, rule, tol), f"{name} ld={ld} rule={rule} tol={tol}")
    finally:
        dM.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dense_to_csr_at_the_segment_edges(handle, shape, dtype):
    D = dense_input(shape[0], shape[1], dtype, shape[0] + shape[1])
    for ld in (shape[1], shape[1] + PAD):
        for rule, tol in RULES:
            assert_bits(csr_of(handle, D, ld, rule, tol), dr.to_csr(D, rule, tol), f"{shape} ld={ld} rule={rule} tol={tol}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", REPEATS)
def test_repeated_columns_give_the_same_bytes_twice_and_the_last_wins(handle, name, dtype):
    M = typed(CASES[name], dtype)
    rows = np.repeat(np.arange(M.rows), np.diff(M.rowPtr))
    cell = rows.astype(np.int64) * M.cols + M.colInd
    assert len(np.unique(cell)) < M.nnz, "the case repeats a column"
    last = {int(c): i for i, c in enumerate(cell)}               # the last entry in storage order of every cell
    want = np.zeros(M.rows * M.cols, dtype)
    want[list(last)] = M.values[list(last.values())]
    dM = M.toGpuCSR()
    try:
        runs = [dense_of(handle, dM, M.cols + PAD, dtype) for _ in range(2)]
        assert runs[0].tobytes() == runs[1].tobytes(), name
        assert same_bytes(runs[0][:, :M.cols], want.reshape(M.rows, M.cols)), name
    finally:
        dM.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_keep_their_bits(handle, dtype):
    sp = _special(dtype)
    t = np.dtype(dtype).type
    vals = np.array(list(sp.values()) + [t(-1), t(1e-8), np.nextafter(t(1e-8), t(1)), t(2)], dtype)
    n = len(vals)
    M = hs.CSR.from_arrays([0, n, n, 2 * n], list(range(n))[::-1] + list(range(n)), np.concatenate([vals, vals]), 3, n + 2, dtype=dtype)
    dM = M.toGpuCSR()
    try:
        got = dense_of(handle, dM, M.cols, dtype)
        assert same_bytes(got, dr.to_dense(M))
        assert got[0, :n].tobytes() == vals[::-1].tobytes() and got[2, :n].tobytes() == vals.tobytes()      # moved, bit for bit
        assert not np.signbit(got[1]).any() and not got[1].any()                                           # untouched cells are +0.0
        ref = csr_of(handle, got, M.cols, dr.KEEP_REFERENCE, 1e-8)
        assert_bits(ref, dr.to_csr(got, dr.KEEP_REFERENCE, 1e-8), "reference rule")
        kept = set(ref.values[ref.rowPtr[2]:].view(np.uint32 if np.dtype(dtype) == np.float32 else np.uint64).tolist())
        bits = lambda x: int(np.array([x], dtype).view(np.uint32 if np.dtype(dtype) == np.float32 else np.uint64)[0])  # noqa: E731
        assert bits(sp["nan"]) in kept and bits(t(-1)) not in kept and bits(np.nextafter(t(1e-8), t(1))) in kept
        assert (bits(t(1e-8)) in kept) == (np.dtype(dtype) == np.float64)        # float(1e-8) is below the double 1e-8
        ab = csr_of(handle, got, M.cols, dr.KEEP_ABS, 0.0)
        assert_bits(ab, dr.to_csr(got, dr.KEEP_ABS, 0.0), "abs rule")
        kept = set(ab.values[ab.rowPtr[2]:].view(np.uint32 if np.dtype(dtype) == np.float32 else np.uint64).tolist())
        assert bits(sp["nan"]) not in kept and bits(t(-1)) in kept and bits(sp["denormal"]) in kept and bits(sp["-0"]) not in kept
    finally:
        dM.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["1000x257", "257x1000"])
def test_round_trip_of_a_sorted_matrix_is_the_matrix(handle, name, dtype):
    S = typed(rr.sort_rows(CASES[name]), dtype)
    dS = S.toGpuCSR()
    d = hs.DenseMatrix(dS, handle)
    try:
        for rule, tol in ((dr.KEEP_ABS, 0.0), (dr.KEEP_ABS, 1e-8)):
            assert_bits(take(d.to_csr(rule, tol, handle)), S, f"{name}: to_csr(to_dense(A))")
    finally:
        d.dispose()
        dS.deviceDispose()


# ---- bad input ---------------------------------------------------------------------------------------------------------
def test_bad_input_is_an_error_not_a_fault(handle):
    L = hs.lib()
    M = typed(CASES["1000x257"], np.float32)
    m, n, ld = M.rows, M.cols, M.cols + PAD
    dM = M.toGpuCSR()
    image = np.full((m, ld), sentinel(np.float32), np.float32)
    buf = hs.h2d(image)
    ups = []

    def call(IA, JA):
        rc = L.hip_csr_to_dense(handle.ptr, m, n, M.nnz, C.c_void_p(IA), C.c_void_p(JA), C.c_void_p(dM.values), C.c_void_p(buf), ld)
        return rc, L.spgemm_hip_last_error()

    def refused(IA, JA, word, what):
        hs.pool_trim(handle.device)
        rc, msg = call(IA, JA)
        assert rc == ERR_INPUT and word in msg, (what, rc, msg)
        balance = hs.pool_cached_bytes(handle.device)
        assert call(IA, JA)[0] == ERR_INPUT, what
        assert hs.pool_cached_bytes(handle.device) == balance, what                  # nothing stays allocated
        assert fetch(buf, m, ld, np.float32).tobytes() == image.tobytes(), what + ": the target was written"
        got = dense_of(handle, dM, n, np.float32)                                    # the handle is usable
        assert same_bytes(got, want_dense("1000x257", np.float32)), "valid call after " + what

    try:
        falling = M.rowPtr.copy()
        falling[500] = falling[499] - 1 if falling[499] > 0 else falling[501] + 1
        ups.append(hs.h2d(falling))
        refused(ups[0], dM.colInd, b"rowPtr", "a decreasing rowPtr")
        for bad, what in ((n, "a column equal to n"), (-1, "a column of -1")):
            cols = M.colInd.copy()
            cols[7] = bad
            ups.append(hs.h2d(cols))
            refused(dM.rowPtr, ups[-1], b"column", what)
    finally:
        for p in ups + [buf]:
            hs.dev_free(p)
        dM.deviceDispose()


def test_pool_does_not_grow(handle):
    dM = typed(CASES["long row"], np.float64).toGpuCSR()

    def rounds(k):
        for _ in range(k):
            d = hs.DenseMatrix(dM, handle)
            d.to_csr(handle=handle).deviceDispose()
            d.dispose()
    try:
        rounds(10)
        before = hs.pool_cached_bytes(handle.device)
        rounds(5)
        assert hs.pool_cached_bytes(handle.device) == before
    finally:
        dM.deviceDispose()


# ---- offsets beyond 2^31 -----------------------------------------------------------------------------------------------
def test_offsets_beyond_2_to_31_and_the_overflow_of_the_count(handle):
    """46341 x 46341 floats: 2 147 488 281 cells, 8.6 GB; the dense buffer never comes to the host.  The all-kept image is
    made by one 64 MiB upload of 0x3f bytes (every float 0.747...) doubled with device copies."""
    import torch
    side = 46341
    cells = side * side
    assert cells > 2 ** 31
    free = torch.cuda.mem_get_info()[0]
    if free < 12 * 2 ** 30:
        pytest.skip(f"needs 12 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    rng = np.random.default_rng(46341)
    rows = np.sort(np.concatenate([[0], rng.integers(0, side - 1, 990), np.full(12, side - 1)]))
    cols = np.concatenate([[0], rng.integers(0, side, len(rows) - 13), side - 1 - 300 * np.arange(12)[::-1]])
    A = _dedupe(rr.sort_rows(rr.Host(np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=side))]), cols,
                                     (rng.random(len(rows)) + 0.25).astype(np.float32), side, side)))
    assert A.colInd[0] == 0 and A.rowPtr[1] >= 1 and A.colInd[-1] == side - 1 and A.rowPtr[-1] - A.rowPtr[-2] == 12
    assert (side - 1) * side + int(A.colInd[-12]) > 2 ** 31      # the 12 entries of the last row lie beyond 2^31
    dA = typed_plain(A, np.float32).toGpuCSR()
    buf = hs.dev_alloc(cells * 4)
    try:
        hs.csr_to_dense_raw(handle, side, side, dA.nnz, dA.rowPtr, dA.colInd, dA.values, buf, side, np.float32)
        ic, jc, cv, nnz = hs.dense_to_csr_raw(handle, side, side, buf, side, dr.KEEP_ABS, 0.0, np.float32)
        assert_bits(take(hs.CSR(cv, jc, ic, side, side, nnz, True, dtype=np.float32)), typed_plain(A, np.float32), "round trip")
        chunk = 64 * 2 ** 20
        seed = hs.h2d(np.full(chunk, 0x3f, np.uint8))
        hs.d2d(buf, seed, chunk)
        hs.dev_free(seed)
        done = chunk
        while done < cells * 4:
            step = min(done, cells * 4 - done)
            hs.d2d(buf + done, buf, step)
            done += step
        hs.device_synchronize()                                   # the copies are not on the handle's stream
        outs = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        cnt = C.c_int(9)
        rc = hs.lib().hip_dense_to_csr(handle.ptr, side, side, C.c_void_p(buf), side, dr.KEEP_REFERENCE, 1e-8,
                                       *[C.byref(x) for x in outs], C.byref(cnt))
        assert rc == ERR_OVERFLOW and [x.value for x in outs] == [None, None, None] and cnt.value == 0, (rc, hs.lib().spgemm_hip_last_error())
    finally:
        hs.dev_free(buf)
        dA.deviceDispose()
        hs.pool_trim(handle.device)


# ---- the product -------------------------------------------------------------------------------------------------------
def product(handle, A, B, pad, dtype):
    """hip_dense_gemm of host arrays; pad > 0: every leading dimension is wider, A's and B's padding holds NaN (it must not
    be read), C's a sentinel (it must survive) -> C[m x n]"""
    m, k = A.shape
    n = B.shape[1]
    lda, ldb, ldc = k + pad, n + pad, n + pad
    image = np.full((m, ldc), sentinel(dtype), dtype)
    dA, dB, dC = hs.h2d(padded(A, lda, np.nan)), hs.h2d(padded(B, ldb, np.nan)), hs.h2d(image)
    try:
        hs.dense_gemm_raw(handle, m, n, k, dA, lda, dB, ldb, dC, ldc, dtype)
        got = fetch(dC, m, ldc, dtype)
        assert np.all(got[:, n:] == sentinel(dtype)), "C's padding was written"
        return got[:, :n]
    finally:
        for p in (dA, dB, dC):
            hs.dev_free(p)


def exact_operands(m, n, k, dtype, seed):
    """multiples of 2^-6 in [-4, 4]: with k <= 256 every partial sum is a multiple of 2^-12 below 2^12, exact in float"""
    rng = np.random.default_rng(seed)
    return ((rng.integers(-256, 257, (m, k)) / 64.0).astype(dtype), (rng.integers(-256, 257, (k, n)) / 64.0).astype(dtype))


EXACT_SHAPES = [(1, 1, 1), (31, 33, 2), (33, 31, 3), (17, 15, 5), (BM - 1, BN + 1, BK + 1), (BM + 1, BN - 1, 2 * BK - 1),
                (2 * BM + 1, 2 * BN + 1, 1), (5, 7, 0), (BM + 2, BN + 2, 256)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_product_of_exact_inputs_is_exact(handle, shape, dtype):
    m, n, k = shape
    assert k <= 256
    A, B = exact_operands(m, n, k, dtype, m * 7 + n * 3 + k)
    want = (A.astype(np.float64) @ B.astype(np.float64) + 0.0).astype(dtype)     # + 0.0: a sum of zeros is +0.0
    assert np.array_equal(want.astype(np.float64), A.astype(np.float64) @ B.astype(np.float64))
    for pad in (0, PAD):
        assert same_bytes(product(handle, A, B, pad, dtype), want), f"{shape} pad={pad}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_times_an_asymmetric_matrix_is_that_matrix(handle, dtype):
    k, n = BM + 5, BN + 37
    assert k * n < 2 ** 24
    B = (np.arange(k, dtype=np.float64)[:, None] * n + np.arange(n)).astype(dtype)
    for pad in (0, PAD):
        assert same_bytes(product(handle, np.eye(k, dtype=dtype), B, pad, dtype), B), f"pad={pad}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(70, 67, 131), (BM + 3, BN + 5, 4 * BK + 1)], ids=lambda s: "x".join(map(str, s)))
def test_product_of_general_inputs_is_within_the_chain_bound(handle, shape, dtype):
    """|got - ref| <= k * u * (|A| |B|)[i][j], the bound of a length-k chain of fused multiply-adds; u = 2^-24 / 2^-53"""
    m, n, k = shape
    rng = np.random.default_rng(k)
    A, B = (rng.random((m, k)) * 2 - 1).astype(dtype), (rng.random((k, n)) * 2 - 1).astype(dtype)
    wide = np.float64 if np.dtype(dtype) == np.float32 else np.longdouble
    ref = A.astype(wide) @ B.astype(wide)
    bound = k * (2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53) * (np.abs(A).astype(wide) @ np.abs(B).astype(wide))
    for pad in (0, PAD):
        err = np.abs(product(handle, A, B, pad, dtype).astype(wide) - ref)
        print(f"{shape} {np.dtype(dtype).name} pad={pad}: max err / bound = {float(np.max(err / bound)):.4f}")
        assert np.all(err <= bound), f"{shape} pad={pad}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_product_agrees_with_the_spgemm(handle, dtype):
    side = 300
    R = random_csr(side, side, 0.03, 300, sorted_rows=False, signed=False)
    rng = np.random.default_rng(300)
    A0 = rr.Host(R.rowPtr, R.colInd, (rng.integers(1, 257, R.nnz) / 64.0).astype(np.float32), side, side)
    # on the CPU: every sum of A * A is exact in float, so any order of summation gives the same bits
    D64 = dr.to_dense(A0).astype(np.float64)
    P64 = D64 @ D64
    assert np.array_equal(P64.astype(np.float32).astype(np.float64), P64)
    oracle = rr.sort_rows(po.omp_spmm(po.CSRHost(A0.rowPtr, A0.colInd, A0.values, side, side),
                                      po.CSRHost(A0.rowPtr, A0.colInd, A0.values, side, side)))
    assert rr.same_bits(_plain(oracle), dr.to_csr(P64.astype(np.float32), dr.KEEP_ABS, 0.0))
    dA = typed_plain(A0, dtype).toGpuCSR()
    dC = hs.gpuSpMMWrapper(dA, dA, handle)
    hs.sort_rows_device(dC, handle)
    d = hs.DenseMatrix(dA, handle)
    p = d.matmul(d, handle)
    dE = p.to_csr(dr.KEEP_ABS, 0.0, handle)
    try:
        raw = hs.csr_diff_raw_f64 if np.dtype(dtype) == np.float64 else hs.csr_diff_raw
        r = raw(handle, side, side, dC.rowPtr, dC.colInd, dC.values, dC.nnz, dE.rowPtr, dE.colInd, dE.values, dE.nnz, 0.0, 0.0)
        assert (r.rows_len_differ, r.only_a, r.only_b, r.beyond) == (0, 0, 0, 0), r.as_dict()
        assert_bits(dE.toCpuCSR(), dr.to_csr(P64.astype(dtype), dr.KEEP_ABS, 0.0), "dense product as a CSR")
    finally:
        for x in (dE, dC, dA):
            x.deviceDispose()
        p.dispose()
        d.dispose()


# ---- the mirrors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_python_class_on_the_known_answer(handle, dtype):
    with open(os.path.join(GOLDEN, "dense_kat.json")) as f:
        k = json.load(f)
    D = np.array(k["dense"], dtype).reshape(k["rows"], k["cols"])
    d = hs.DenseMatrix.from_host(D)
    dA = d.to_csr(handle=handle)
    back = hs.DenseMatrix(dA, handle)
    z = hs.DenseMatrix.zeros(3, 4, dtype)
    sq = d.matmul(hs.DenseMatrix.from_host(D.T.copy()), handle)
    try:
        assert (d.rows, d.cols, d.ld, d.dtype) == (5, 6, 6, np.dtype(dtype)) and same_bytes(d.download(), D)
        A = dA.toCpuCSR()
        assert A.rowPtr.tolist() == k["expected"]["rowPtr"] and A.colInd.tolist() == k["expected"]["colInd"]
        assert A.values.tolist() == k["expected"]["values"] and A.values.dtype == np.dtype(dtype)
        assert same_bytes(back.download(), D)
        assert same_bytes(z.download(), np.zeros((3, 4), dtype))
        assert (sq.rows, sq.cols) == (5, 5) and same_bytes(sq.download(), (D.astype(np.float64) @ D.T.astype(np.float64)).astype(dtype))
    finally:
        dA.deviceDispose()
        for x in (d, back, z, sq):
            x.dispose()


def test_cpp_mirror_runs_the_dense_scenarios():
    """tests/cpp/dense_check.cc: the known answer, the dense-somp scenario on own_graph.snap, the float fmaf chain"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-B", "-C", cpp, "-f", "dense.mk", "dense_check.x"])
    out = subprocess.run([os.path.join(cpp, "dense_check.x"), os.path.join(DATA, "own_graph.snap")], capture_output=True, text=True,
                         timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    for check in ("shape", "rowPtr", "colInd", "values", "dense again", "host form", "host dense again"):
        assert f"kat {check}: ok" in lines, check
    assert "Same" in lines and "Diffs" not in lines
    assert "fmaf chain: 0 of 4690 elements differ" in lines
    assert "Pass" in lines and "FAILED" not in out.stdout
