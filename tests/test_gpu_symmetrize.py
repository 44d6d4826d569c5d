"""GPU: sparse add, diagonal scaling, degree counts / factors and the three symmetrisations of a directed graph, against
the numpy restatement (symmetrize_ref), in float32 and float64.  Float64 values carry + 2^-40 so a pass through float
would show."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import clusters_ref as cr
import symmetrize_ref as sr
from reorder_ref import Host
from devcsr import built_gpu, handle  # noqa: F401
from devcsr import assert_bits, take
from helpers import DATA, ROOT, po
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
ERR_INPUT = 5
ADD_TILE = 1024         # work items (entries of A, then of B) per block of the two passes of the add (symmetrize_device.hpp)
T = ADD_TILE
COEFFICIENTS = [(1.0, 1.0), (1.0, -1.0), (0.5, 2.0), (1.0, 0.0), (0.0, 0.0)]
RMCL_INIT = hs.COO_SELF_LOOPS | hs.COO_ROW_NORMALISE


# ---- inputs (made once per name, never modified) ---------------------------------------------------------------------
def _values(rng, n, dtype, signed=True):
    """float32 numbers (of either sign); float64 gets bits beyond float32"""
    v = (rng.random(n) + 0.25) * (rng.choice([-1.0, 1.0], size=n) if signed else 1.0)
    v = v.astype(np.float32).astype(np.float64)
    return (v + 2.0 ** -40 if np.dtype(dtype) == np.float64 else v).astype(dtype)


def from_flat(pos, values, rows, cols):
    """sorted distinct flat positions row * cols + col -> CSR with strictly ascending rows"""
    pos = np.asarray(pos, np.int64)
    rp = np.zeros(rows + 1, np.int32)
    if rows:
        np.cumsum(np.bincount(pos // max(cols, 1), minlength=rows), out=rp[1:])
    return Host(rp, pos % max(cols, 1), values, rows, cols)


def pair(rows, cols, nnzA, nnzB, common, seed, dtype):
    """-> (A, B) with strictly ascending rows, exactly nnzA / nnzB entries, `common` positions shared"""
    rng = np.random.default_rng(seed)
    cells = rows * cols
    picked = rng.choice(cells, size=nnzA + nnzB - common, replace=False) if cells else np.zeros(0, np.int64)
    posA, posB = np.sort(picked[:nnzA]), np.sort(picked[nnzA - common:])
    return from_flat(posA, _values(rng, nnzA, dtype), rows, cols), from_flat(posB, _values(rng, nnzB, dtype), rows, cols)


def long_row_pair(dtype):
    """300 x 40 000, the construction of the comparison's long row: row 17 holds 20 000 strictly ascending columns in A
    and, in B, half of those plus 10 000 others; every other row is empty"""
    rng = np.random.default_rng(17)
    cols = rng.permutation(40000)
    ca, extra = np.sort(cols[:20000]), cols[20000:30000]
    va = (rng.random(20000) + 0.25).astype(np.float32).astype(np.float64)
    if np.dtype(dtype) == np.float64:
        va = va + 2.0 ** -40
    half = np.sort(rng.choice(20000, size=10000, replace=False))
    scale = np.where(rng.integers(0, 4, size=10000) == 0, 1.0 + 1e-3, 1.0)
    cb = np.concatenate([ca[half], extra])
    vb = np.concatenate([va[half] * scale, (rng.random(10000) + 0.25).astype(np.float32).astype(np.float64)])
    order = np.argsort(cb)
    rp = np.zeros(301, np.int32)
    rp[18:] = 20000
    return Host(rp, ca, va.astype(dtype), 300, 40000), Host(rp, cb[order], vb[order].astype(dtype), 300, 40000)


def _rows_to_csr(rows, cols, dtype, seed):
    """rows: list of column lists (ascending)"""
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c in r], np.int32)
    return Host(rp, ci, _values(rng, len(ci), dtype), len(rows), cols)


def edge_pair(dtype):
    """rows whose only common column is the first (row 0) or the last (row 1) of the row, in both operands or in one
    (rows 2, 3); a row present in A only (4), in B only (5), in neither (6); one common column and nothing else (7)"""
    a = [[2, 5, 9, 30], [1, 4, 8, 40], [3, 10, 11], [0, 6, 12], [7, 8, 9], [], [], [13]]
    b = [[2, 6, 10, 31], [0, 3, 7, 40], [3, 20, 21, 22], [1, 2, 12], [], [5, 6], [], [13]]
    return _rows_to_csr(a, 41, dtype, 31), _rows_to_csr(b, 41, dtype, 32)


def identical_pair(dtype):
    A, _ = pair(61, 97, 400, 0, 0, 21, dtype)
    return A, Host(A.rowPtr, A.colInd, A.values.copy(), A.rows, A.cols)


SHAPES = {
    "0x0": lambda dt: pair(0, 0, 0, 0, 0, 1, dt),
    "5x7 both empty": lambda dt: pair(5, 7, 0, 0, 0, 2, dt),
    "A empty": lambda dt: pair(61, 97, 0, 300, 0, 3, dt),
    "B empty": lambda dt: pair(61, 97, 300, 0, 0, 4, dt),
    # nnzA + nnzB = T - 1, T, T + 1: the last block of the walk
    "total T-1": lambda dt: pair(61, 97, 520, T - 1 - 520, 200, 5, dt),
    "total T": lambda dt: pair(61, 97, 520, T - 520, 200, 6, dt),
    "total T+1": lambda dt: pair(61, 97, 520, T + 1 - 520, 200, 7, dt),
    # nnzB = T - 1, T, T + 1: the scan of onlyB and the B items on a block edge
    "nnzB T-1": lambda dt: pair(61, 97, 700, T - 1, 300, 8, dt),
    "nnzB T": lambda dt: pair(61, 97, 700, T, 300, 9, dt),
    "nnzB T+1": lambda dt: pair(61, 97, 700, T + 1, 300, 10, dt),
    "same pattern": lambda dt: pair(61, 97, 400, 400, 400, 11, dt),
    "identical": identical_pair,
    "disjoint": lambda dt: pair(61, 97, 400, 450, 0, 12, dt),
    "row edges": edge_pair,
    "long row": long_row_pair,
}


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    return SHAPES[name](dtype)


@functools.lru_cache(maxsize=None)
def want_add(name, dtype, alpha, beta):
    A, B = case(name, dtype)
    return sr.add(A, B, alpha, beta)


def to_dev(M):
    return hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols, dtype=M.values.dtype).toGpuCSR()


def strictly_ascending(M):
    rp = np.asarray(M.rowPtr, np.int64)
    inner = np.ones(M.nnz, bool)
    inner[rp[:-1][rp[:-1] < M.nnz]] = False                        # the first entry of every non-empty row
    return bool(np.all(np.diff(np.asarray(M.colInd, np.int64))[inner[1:]] > 0)) if M.nnz > 1 else True


def test_the_shapes_are_what_they_claim():
    for dt in DTYPES:
        for name in SHAPES:
            A, B = case(name, dt)
            assert strictly_ascending(A) and strictly_ascending(B), name
            assert A.values.dtype == B.values.dtype == np.dtype(dt)
        for k, d in (("T-1", -1), ("T", 0), ("T+1", 1)):
            A, B = case("total " + k, dt)
            assert A.nnz + B.nnz == T + d
            assert case("nnzB " + k, dt)[1].nnz == T + d
        A, B = case("same pattern", dt)
        assert np.array_equal(A.colInd, B.colInd) and np.array_equal(A.rowPtr, B.rowPtr)
        A, B = case("disjoint", dt)
        assert not (sr.pattern(A) & sr.pattern(B)).any()
        A, B = case("long row", dt)
        assert A.rowPtr[18] - A.rowPtr[17] == 20000 and np.count_nonzero(np.isin(B.colInd, A.colInd)) == 10000
        A, B = case("row edges", dt)
        common = sr.pattern(A) & sr.pattern(B)
        assert [np.flatnonzero(common[r]).tolist() for r in range(8)] == [[2], [40], [3], [12], [], [], [], [13]]
    if np.dtype(np.float64) in map(np.dtype, DTYPES):
        v = case("total T", np.float64)[0].values
        assert np.any(v.astype(np.float32).astype(np.float64) != v)


# ---- hip_csr_add -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_add_matches_the_restatement_bit_for_bit(handle, name, dtype):
    A, B = case(name, dtype)
    dA, dB = to_dev(A), to_dev(B)
    try:
        for alpha, beta in COEFFICIENTS:
            got = take(dA.add(dB, alpha, beta, handle))
            want = want_add(name, dtype, alpha, beta)
            assert got.nnz == want.nnz
            assert_bits(got, want, f"{name} {np.dtype(dtype)} alpha={alpha} beta={beta}")
    finally:
        dA.deviceDispose()
        dB.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_minus_a_keeps_every_entry_at_zero(handle, dtype):
    A, B = case("identical", dtype)
    got = hs.CSR.from_arrays(A.rowPtr, A.colInd, A.values, A.rows, A.cols, dtype=dtype).add(
        hs.CSR.from_arrays(B.rowPtr, B.colInd, B.values, B.rows, B.cols, dtype=dtype), 1.0, -1.0, handle)   # host CSRs
    assert not got.on_device and got.nnz == A.nnz and np.array_equal(got.colInd, A.colInd)
    assert np.array_equal(got.rowPtr, A.rowPtr) and got.values.dtype == np.dtype(dtype) and np.all(got.values == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_add_with_an_inf_and_a_nan(handle, dtype):
    A, B = case("total T+1", dtype)
    va, vb = A.values.copy(), B.values.copy()
    ka, kb = (np.repeat(np.arange(M.rows, dtype=np.int64), np.diff(M.rowPtr)) * M.cols + M.colInd for M in (A, B))
    common = np.flatnonzero(np.isin(ka, kb))
    va[common[0]] = np.inf                                         # inf on a common column
    va[common[1]] = np.nan                                         # NaN on a common column
    vb[np.flatnonzero(~np.isin(kb, ka))[0]] = -np.inf              # -inf on a column only B holds
    A2, B2 = Host(A.rowPtr, A.colInd, va, A.rows, A.cols), Host(B.rowPtr, B.colInd, vb, B.rows, B.cols)
    want = sr.add(A2, B2, 0.5, 2.0)
    dA, dB = to_dev(A2), to_dev(B2)
    try:
        got = take(dA.add(dB, 0.5, 2.0, handle))
    finally:
        dA.deviceDispose()
        dB.deviceDispose()
    assert np.array_equal(got.rowPtr, want.rowPtr) and np.array_equal(got.colInd, want.colInd)
    assert np.isnan(want.values).sum() >= 1 and np.isinf(want.values).sum() >= 2
    assert np.array_equal(np.isnan(got.values), np.isnan(want.values))
    assert np.array_equal(np.isinf(got.values), np.isinf(want.values))
    plain = np.isfinite(want.values)
    assert got.values[plain].tobytes() == want.values[plain].tobytes()
    assert np.array_equal(np.sign(got.values[~plain & ~np.isnan(want.values)]), np.sign(want.values[~plain & ~np.isnan(want.values)]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["total T+1", "long row"])
def test_two_calls_return_the_same_bytes(handle, name, dtype):
    A, B = case(name, dtype)
    dA, dB = to_dev(A), to_dev(B)
    try:
        first, second = take(dA.add(dB, 0.5, 2.0, handle)), take(dA.add(dB, 0.5, 2.0, handle))
    finally:
        dA.deviceDispose()
        dB.deviceDispose()
    assert_bits(second, first, name)


def _raw_add(handle, dtype, m, n, A, B):
    """(rc, outputs) of the C entry itself on host triples (rowPtr, colInd, values) uploaded as they are"""
    ups = [hs.h2d(np.ascontiguousarray(x, dt)) for M in (A, B) for x, dt in zip(M, (np.int32, np.int32, dtype))]
    try:
        out = hs._CsrOut()
        fn, _ = hs._typed("hip_csr_add", dtype)
        rc = fn(handle.ptr, m, n, 1.0, *hs._ptrs(*ups[:3]), len(A[1]), 1.0, *hs._ptrs(*ups[3:]), len(B[1]), *out.refs())
        return rc, out.values()
    finally:
        for p in ups:
            hs.dev_free(p)


BAD = {
    "two equal columns": ([0, 3, 4], [1, 1, 2, 0]),
    "a descending row": ([0, 3, 4], [0, 2, 1, 0]),
    "a column equal to n": ([0, 3, 4], [0, 1, 5, 0]),
    "a decreasing rowPtr": ([0, 3, 2, 4], [0, 1, 2, 0]),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("what", list(BAD))
def test_bad_input_is_an_error_not_a_fault(handle, what, side, dtype):
    rp, ci = BAD[what]
    m, n = len(rp) - 1, 5
    good_rp = np.zeros(m + 1, np.int32)
    good_rp[1:] = np.arange(1, m + 1)
    good = (good_rp, np.zeros(m, np.int32), np.ones(m, dtype))
    bad = (np.array(rp, np.int32), np.array(ci, np.int32), np.ones(len(ci), dtype))
    rc, outs = _raw_add(handle, dtype, m, n, *((bad, good) if side == "A" else (good, bad)))
    assert rc == ERR_INPUT, (rc, hs.lib().spgemm_hip_last_error())
    assert outs == (None, None, None, 0) and hs.lib().spgemm_hip_last_error()
    rc, outs = _raw_add(handle, dtype, m, n, good, good)          # the handle is still usable
    assert rc == 0 and outs[3] == m
    for p in outs[:3]:
        hs.dev_free(p)


# ---- hip_csr_scale / hip_csr_col_counts / hip_degree_factors -----------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["nnzB T+1", "long row"])
def test_scale_matches_the_restatement(handle, name, dtype):
    A = case(name, dtype)[0]
    rng = np.random.default_rng(41)
    rs, cs = _values(rng, A.rows, dtype), _values(rng, A.cols, dtype)
    dA = to_dev(A)
    drs, dcs = hs.h2d(rs), hs.h2d(cs)
    out = hs.dev_alloc(A.values.itemsize * max(A.nnz, 1))
    try:
        for hr, hc, pr, pc in ((rs, cs, drs, dcs), (rs, None, drs, None), (None, cs, None, dcs), (None, None, None, None)):
            hs.csr_scale_raw(handle, A.rows, A.cols, A.nnz, dA.rowPtr, dA.colInd, dA.values, pr, pc, out, dtype=dtype)
            got, want = hs.d2h(out, A.nnz, dtype), sr.scale(A, hr, hc)
            assert got.tobytes() == want.tobytes(), (name, hr is None, hc is None)
        hs.csr_scale_raw(handle, A.rows, A.cols, A.nnz, dA.rowPtr, dA.colInd, dA.values, drs, dcs, dA.values, dtype=dtype)
        assert hs.d2h(dA.values, A.nnz, dtype).tobytes() == sr.scale(A, rs, cs).tobytes(), "in place"
        assert np.array_equal(hs.d2h(dA.colInd, A.nnz, np.int32), A.colInd)
    finally:
        for p in (drs, dcs, out):
            hs.dev_free(p)
        dA.deviceDispose()


def test_scale_refuses_a_column_outside_the_scale(handle):
    rp, ci, v = np.array([0, 2], np.int32), np.array([0, 3], np.int32), np.ones(2, np.float32)
    ups = [hs.h2d(x) for x in (rp, ci, v, np.ones(3, np.float32))]
    try:
        with pytest.raises(hs.SpgemmError, match="status 5"):
            hs.csr_scale_raw(handle, 1, 3, 2, *ups[:3], None, ups[3], ups[2])
        assert np.array_equal(hs.d2h(ups[2], 2, np.float32), v)
        hs.csr_scale_raw(handle, 1, 3, 2, *ups[:3], None, None, ups[2])          # no column scale: the column indexes nothing
    finally:
        for p in ups:
            hs.dev_free(p)


def test_col_counts_with_an_unnamed_and_a_hot_column(handle):
    # 20 000 rows x 5 columns: column 1 in every row, column 0 in every 7th, column 4 in every 3rd; nobody names 2 and 3
    rows = [([0] if r % 7 == 0 else []) + [1] + ([4] if r % 3 == 0 else []) for r in range(20000)]
    A = _rows_to_csr(rows, 5, np.float32, 51)
    want = sr.col_counts(A)
    assert want.tolist() == [2858, 20000, 0, 0, 6667]
    dci, count = hs.h2d(A.colInd), hs.h2d(np.full(5, -1, np.int32))
    try:
        hs.csr_col_counts_raw(handle, 5, A.nnz, dci, count)
        assert np.array_equal(hs.d2h(count, 5, np.int32), want)
        with pytest.raises(hs.SpgemmError, match="status 5"):
            hs.csr_col_counts_raw(handle, 4, A.nnz, dci, count)                   # column 4 is outside [0, 4)
        assert np.array_equal(hs.d2h(count, 5, np.int32), want)                    # untouched
    finally:
        hs.dev_free(dci)
        hs.dev_free(count)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_degree_factors(handle, dtype):
    counts = np.concatenate([np.arange(0, 1200), [20000, 65537, 10 ** 6, 2 ** 31 - 1]]).astype(np.int32)
    dc, out = hs.h2d(counts), hs.dev_alloc(np.dtype(dtype).itemsize * len(counts))
    try:
        for e in (0.5, 0.25, 1.0, 0.0):
            hs.degree_factors_raw(handle, len(counts), dc, e, out, dtype=dtype)
            got = hs.d2h(out, len(counts), dtype)
            assert got[0] == 0 and got[1] == 1
            want = np.power(counts[1:].astype(dtype), np.dtype(dtype).type(-e))
            ulps = np.abs(got[1:].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
            print(f"{np.dtype(dtype)} exponent {e}: largest distance {ulps.max():.2f} ulp")
            assert ulps.max() <= 4.0, (e, int(counts[1:][ulps.argmax()]))
    finally:
        hs.dev_free(dc)
        hs.dev_free(out)


# ---- hip_csr_symmetrize ------------------------------------------------------------------------------------------------
def hub_graph(dtype):
    """257 nodes, directed, positive values.  Row 0 is the hub: 60 out-links, to nodes 1..60, each of which has exactly
    10 in-links (the hub and 9 of the nodes 61..256), so row 0 of A * A^T is made of 600 products.  The nodes 61..256
    also link among themselves (about 4 per row, a diagonal entry here and there, some edges in both directions)."""
    rng = np.random.default_rng(257)
    m = 257
    P = np.zeros((m, m), bool)
    P[0, 1:61] = True
    for c in range(1, 61):
        P[rng.choice(np.arange(61, m), size=9, replace=False), c] = True
    tail = rng.random((m - 61, m - 61)) < 4.0 / (m - 61)
    P[61:, 61:] |= tail
    P[100, 100] = P[101, 101] = True                                # diagonal entries
    P[70, 80] = P[80, 70] = True                                    # an edge stored in both directions
    D = np.zeros((m, m), np.float64)
    r, c = np.nonzero(P)
    D[r, c] = _values(rng, len(r), dtype, signed=False)
    return sr.from_dense(D.astype(dtype), P)


def own_graph(dtype):
    A = po.load(os.path.join(DATA, "own_graph.snap"), isTrans=False, mode=0)
    v = A.values.astype(np.float64) + (2.0 ** -40 if np.dtype(dtype) == np.float64 else 0.0)
    return Host(A.rowPtr, A.colInd, v.astype(dtype), A.rows, A.cols)


GRAPHS = {"hub 257": hub_graph, "own_graph.snap": own_graph}


@functools.lru_cache(maxsize=None)
def graph(name, dtype):
    return GRAPHS[name](dtype)


def test_the_hub_row_has_600_products():
    A = graph("hub 257", np.float32)
    indeg = sr.col_counts(A)
    assert A.rowPtr[1] - A.rowPtr[0] == 60 and int(indeg[A.colInd[:60]].sum()) == 600
    assert strictly_ascending(A) and np.all(A.values > 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_sum_mode_is_a_plus_at_bit_for_bit(handle, name, dtype):
    A = graph(name, dtype)
    dA = to_dev(A)
    try:
        dS = dA.symmetrize(hs.SYM_SUM, handle=handle)
        try:
            dT = dS.transpose(handle)
            S, St = dS.toCpuCSR(), take(dT)
        finally:
            dS.deviceDispose()
    finally:
        dA.deviceDispose()
    assert_bits(S, sr.sym_sum(A), name)
    assert_bits(St, S, name + ": its own transpose")
    dense, a = sr.to_dense(S), sr.to_dense(A)
    assert np.array_equal(np.diag(dense), 2 * np.diag(a))         # a diagonal entry is doubled
    if name == "hub 257":
        assert a[100, 100] != 0 and a[70, 80] != 0 and a[80, 70] != 0
        assert dense[70, 80] == a[70, 80] + a[80, 70] == dense[80, 70]      # both directions: summed


def test_sum_mode_of_a_host_csr_and_of_nothing(handle):
    A = graph("own_graph.snap", np.float32)
    S = hs.CSR.from_arrays(A.rowPtr, A.colInd, A.values, A.rows, A.cols).symmetrize(handle=handle)
    assert not S.on_device
    assert_bits(S, sr.sym_sum(A), "host CSR")
    E = hs.CSR.from_arrays(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 0, 0).symmetrize(handle=handle)
    assert E.nnz == 0 and E.rows == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_symmetrize_refuses_an_unsorted_row(handle, dtype):
    rp, ci = np.array([0, 2, 3, 3], np.int32), np.array([2, 1, 0], np.int32)
    dA = hs.CSR.from_arrays(rp, ci, np.ones(3, dtype), 3, 3, dtype=dtype).toGpuCSR()
    try:
        for mode in (hs.SYM_SUM, hs.SYM_BIBLIOMETRIC, hs.SYM_DEGREE_DISCOUNTED):
            with pytest.raises(hs.SpgemmError, match="status 5"):
                dA.symmetrize(mode, handle=handle)
    finally:
        dA.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("mode", ["bibliometric", "degree discounted"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_product_modes_against_the_dense_evaluation(handle, name, mode, dtype):
    """The structure is exact; the values are held to |got - want| <= (K + 16) * u * want with u = 2^-24 (float32) or
    2^-53 (float64) and K the longest row of the scaled operand (rows of Y and columns of Z: the longest row or column of
    A).  Why: every input is positive, so nothing cancels and relative errors only add up (first order in u).
      an entry of S is  sum over k of y_ik * y_jk  +  sum over k of z_ki * z_kj, at most K terms in each sum;
      y_ik = (fo_i * a_ik) * fih_k: two factors and two multiplications.  A factor is pow() evaluated in double and
        rounded to the value type: at most 1 u in float32 (0.5 u from the rounding, pow's own error is 2^-29 of that),
        at most 2 u in float64 (pow within 1 ulp, the exponent -e/2 exact, the count exact).  So y_ik carries at most
        2 * 2 + 2 = 6 u, and a product y_ik * y_jk at most 6 + 6 + 1 = 13 u;
      a sum of n positive terms added in any order carries at most (n - 1) u on top of its terms' own error: K - 1;
      the final add of the two products: 1 u.
      13 + (K - 1) + 1 = K + 13 <= K + 16.
    The dense float64 evaluation it is compared with carries its own rounding, about 2^-53 * (K + 8) at worst: nothing
    beside u in float32.  In float64 it is of the size of the bound itself, so there the assertion holds the two
    evaluations to (K + 16) u of each other, which is what the bound says, not to 2 (K + 16) u.
    The bibliometric mode has no factors: 1 + (K - 1) + 1 + 1 = K + 2.  The same bound is asserted for both."""
    A = graph(name, dtype)
    dA = to_dev(A)
    try:
        dS = dA.symmetrize(hs.SYM_BIBLIOMETRIC if mode == "bibliometric" else hs.SYM_DEGREE_DISCOUNTED, 0.5, 0.5, handle)
        try:
            St = take(dS.transpose(handle))
            S = dS.toCpuCSR()
        finally:
            dS.deviceDispose()
    finally:
        dA.deviceDispose()
    want = sr.sym_bibliometric(A) if mode == "bibliometric" else sr.sym_degree_discounted(A, 0.5, 0.5)
    assert S.values.dtype == np.dtype(dtype)
    assert np.array_equal(S.rowPtr, want.rowPtr) and np.array_equal(S.colInd, want.colInd), "structure"
    assert np.array_equal(St.rowPtr, S.rowPtr) and np.array_equal(St.colInd, S.colInd), "the pattern is symmetric"
    K = int(max(np.diff(A.rowPtr).max(), sr.col_counts(A).max()))
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    err = np.abs(S.values.astype(np.float64) - want.values) / want.values
    print(f"{name} {mode} {np.dtype(dtype)}: K={K} nnz={S.nnz} largest error {err.max() / u:.2f} u, bound {K + 16} u")
    assert np.all(want.values > 0) and err.max() <= (K + 16) * u


# ---- through the chain -------------------------------------------------------------------------------------------------
def test_directed_file_to_clusters_on_the_device(handle):
    path = os.path.join(DATA, "own_graph.snap")
    # device: parse, symmetrise, rmclInit's flags, two iterations, clusters
    dA = hs.read_edge_file(path, isTrans=False, flags=hs.COO_DEDUPE, handle=handle)
    try:
        dS = dA.symmetrize(hs.SYM_SUM, handle=handle)
    finally:
        dA.deviceDispose()
    S = take(dS)
    ri = np.repeat(np.arange(S.rows, dtype=np.int32), np.diff(S.rowPtr))
    dMt = hs.coo_to_csr(S.rows, S.cols, ri, S.colInd, S.values, RMCL_INIT, handle)
    try:
        dOut = hs.gpuRmclIter_device(2, dMt, dMt, handle)
    finally:
        dMt.deviceDispose()
    try:
        cl = hs.rmcl_clusters(dOut, handle)
        try:
            got = (cl.k,) + cl.to_host()
        finally:
            cl.dispose()
    finally:
        dOut.deviceDispose()
    # host: the restatement's A + A^T, the oracle's rmclInit and R-MCL, the clusters' restatement
    A = po.load(path, isTrans=False, mode=0)
    hS = sr.sym_sum(Host(A.rowPtr, A.colInd, A.values, A.rows, A.cols))
    assert_bits(S, hS, "A + A^T")
    hri = np.repeat(np.arange(hS.rows, dtype=np.int32), np.diff(hS.rowPtr))
    Mt = po.rmcl_init(hS.rows, hS.cols, hri, hS.colInd, hS.values)
    out = po.rmcl_iters(Mt, Mt, 2)
    k, cluster, ptr, members, _, _ = cr.rmcl_clusters(out.rowPtr, out.colInd, out.values)
    assert got[0] == k
    assert np.array_equal(got[1], cluster) and np.array_equal(got[2], ptr) and np.array_equal(got[3], members)


def test_cpp_mirror_prints_same():
    """tests/cpp/symmetrize_check.cc: own_graph.snap through gpuSymmetrize(SUM) against a host two-pointer A + A^T, then
    rmclInit's flags, gpuRmclIterDevice and gpuRmclClusters on the symmetrised graph"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "symmetrize.mk", "symmetrize_check.x"])
    out = subprocess.run([os.path.join(cpp, "symmetrize_check.x"), os.path.join(DATA, "own_graph.snap")], capture_output=True,
                         text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "Same" in lines and "Diffs" not in lines
