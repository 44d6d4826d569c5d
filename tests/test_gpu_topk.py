"""GPU (-m gpu): hip_csr_row_topk / _f64 against the numpy restatement tests/topk_ref.py (pinned by hand in
tests/test_topk_abi.py).  Every selection comparison is bit for bit; only the normalised values of the rows that were cut
have a tolerance, worked out where it is used.  After each case the path counters say which kernel took the rows."""
import numpy as np
import pytest

from devcsr import built_gpu, handle  # noqa: F401
from devcsr import _special, assert_bits, one_long_row, take, typed, with_nnz
from reorder_ref import Host
from sparse_matrix_with_flops_amd import hipspgemm as hs
import topk_ref as tr

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
INT_MAX = 2 ** 31 - 1
N = 300                                                     # columns of the hand-built matrices


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _assemble(rows, dtype, n=N):
    """rows: list of (columns, values) -> Host"""
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c, _ in rows])
    ci = np.concatenate([np.asarray(c, np.int32) for c, _ in rows]) if rows else np.zeros(0, np.int32)
    v = np.concatenate([np.asarray(x, dtype) for _, x in rows]) if rows else np.zeros(0, dtype)
    return Host(rp, ci, v, len(rows), n)


def _tied_row(length, rng, dtype):
    """random columns (repeats) and values from 50 levels: ties on the value, and on the pair, wherever the cut falls"""
    return rng.integers(0, N, size=length), (rng.integers(0, 50, size=length) / 64 + 0.25).astype(dtype)


def _among(row, k, rng, dtype):
    """the row among empty rows and rows too short to be cut"""
    short = [_tied_row(n, rng, dtype) for n in (min(k, 3), 1, min(k, 2))]
    none = ([], [])
    return [none, short[0], row, none, none, short[1], short[2]]


def _path_of(length, k, dtype):
    wave, block = hs.row_topk_limits(dtype)
    return "copied" if length <= k else "wave" if length <= wave else "block" if length <= block else "stream"


# ---- the call --------------------------------------------------------------------------------------------------------
def _run(M, k, handle, normalise=False):
    """-> (result on the host, rows cut, what the call added to the path counters)"""
    d = hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols, dtype=M.values.dtype).toGpuCSR()
    try:
        before = handle.topk_paths()
        out = d.row_topk(k, normalise=normalise, handle=handle)
        after = handle.topk_paths()
    finally:
        d.deviceDispose()
    return take(out), out.rows_cut, {p: after[p] - before[p] for p in after}


def _expected_paths(M, k, dtype):
    want = {"copied": 0, "wave": 0, "block": 0, "stream": 0}
    for n in np.diff(M.rowPtr):
        want[_path_of(int(n), k, dtype)] += 1
    return want


def _check(M, k, handle, what):
    dtype = M.values.dtype
    got, cut, paths = _run(M, k, handle)
    want, want_cut = tr.of(M, k)
    assert_bits(got, want, what)
    assert cut == want_cut, what
    assert paths == _expected_paths(M, k, dtype), what
    return paths


# ---- row lengths around every edge -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_lengths_around_every_edge(handle, dtype, k):
    wave, block = hs.row_topk_limits(dtype)
    rng = np.random.default_rng(1000 + k)
    for length in [k, k + 1, 63, 64, 65, wave, wave + 1, block, block + 1]:
        M = _assemble(_among(_tied_row(length, rng, dtype), k, rng, dtype), dtype)
        paths = _check(M, k, handle, f"len={length} k={k}")
        assert paths[_path_of(length, k, dtype)] >= 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_but_one_entry_kept(handle, dtype):
    wave, block = hs.row_topk_limits(dtype)
    rng = np.random.default_rng(7)
    for length in [2, 64, 65, 66, wave, wave + 1, block, block + 1]:
        k = length - 1
        M = _assemble(_among(_tied_row(length, rng, dtype), k, rng, dtype), dtype)
        paths = _check(M, k, handle, f"len={length} k=len-1")
        assert paths[_path_of(length, k, dtype)] == 1 and paths["copied"] == M.rows - 1


# ---- ties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_equal_rows_in_every_column_order(handle, dtype):
    """an rmclInit row: every value 1/len, so the columns alone decide, whatever order they are stored in"""
    wave, block = hs.row_topk_limits(dtype)
    rng = np.random.default_rng(11)
    rows = []
    for length in (100, wave + 900, block + 500):
        cols = rng.permutation(20000)[:length]                       # distinct
        v = np.full(length, dtype(1) / dtype(length), dtype)
        rows += [(np.sort(cols), v), (np.sort(cols)[::-1], v), (rng.permutation(cols), v)]
    M = _assemble(rows, dtype, n=20000)
    for k in (1, 16, 99):
        paths = _check(M, k, handle, f"all equal, k={k}")
        assert (paths["wave"], paths["block"], paths["stream"]) == (3, 3, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeated_pairs_straddle_the_cut(handle, dtype):
    """four columns and two values: whole groups of identical (value, column) pairs lie across the cut, so the position
    decides; one_long_row is the stream path's row with repeated columns"""
    wave, block = hs.row_topk_limits(dtype)
    rng = np.random.default_rng(13)
    rows = [(rng.integers(0, 4, size=n), rng.choice([0.25, 0.5], size=n)) for n in (40, 70, wave, wave + 7, block + 9)]
    M = _assemble(rows, dtype)
    for k in (3, 17, 33):
        _check(M, k, handle, f"repeated pairs, k={k}")
    long = typed(one_long_row(), dtype)
    for k in (1, 64, 7000):
        paths = _check(long, k, handle, f"one long row, k={k}")
        assert paths["stream"] == 1 and paths["copied"] == long.rows - 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_values_one_step_apart(handle, dtype):
    """neighbouring floats (one ulp apart) / doubles 2^-40 apart, which a float cannot tell apart: no two may be mistaken"""
    wave, block = hs.row_topk_limits(dtype)
    rng = np.random.default_rng(17)
    rows = []
    for length in (50, 700, wave + 50, block + 50):
        steps = rng.permutation(length)
        if np.dtype(dtype) == np.float32:
            v = (np.float32(0.5).view(np.uint32) + steps.astype(np.uint32)).view(np.float32)
        else:
            v = 0.5 + steps * 2.0 ** -40
        rows.append((rng.integers(0, N, size=length), v))
    M = _assemble(rows, dtype)
    assert np.dtype(dtype) == np.float32 or len(np.unique(M.values.astype(np.float32))) < 20
    for k in (1, 10, 49):
        _check(M, k, handle, f"one step apart, k={k}")


# ---- special values --------------------------------------------------------------------------------------------------
def _special_row(length, numbers, rng, dtype):
    """`numbers` entries are numbers (among them both infinities, both zeros, a denormal), the others NaNs of both sign bits
    with payloads"""
    sp = _special(dtype)
    bits = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    neg_nan = (np.array([sp["nan"]], dtype).view(bits) | bits(1 << (8 * np.dtype(dtype).itemsize - 1))).view(dtype)[0]
    assert np.isnan(neg_nan) and np.signbit(neg_nan)
    v = (rng.integers(-20, 20, size=length) / 16).astype(dtype)
    fixed = [np.inf, -np.inf, -0.0, 0.0, sp["denormal"], -sp["denormal"], sp["1e-9"], sp["above"]]
    where = rng.permutation(length)
    for p, x in zip(where[:numbers], fixed):
        v[p] = x
    for j, p in enumerate(where[numbers:]):
        v[p] = neg_nan if j % 2 else sp["nan"]
    return rng.integers(0, N, size=length), v


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values(handle, dtype):
    wave, block = hs.row_topk_limits(dtype)
    rng = np.random.default_rng(19)
    rows = []
    for length in (12, 200, wave + 30, block + 30):
        rows.append(_special_row(length, 8, rng, dtype))                  # fewer numbers than any k below but 1 and 5
        rows.append(_special_row(length, length - 3, rng, dtype))         # all but three are numbers
    M = _assemble(rows, dtype)
    for k in (1, 5, 9, 11):
        got, _, _ = _run(M, k, handle)
        _check(M, k, handle, f"special values, k={k}")
        first = got.values[:got.rowPtr[1]]
        assert k < 9 or np.isnan(first).sum() == k - 8                    # row 0 has 8 numbers: NaNs fill the rest


# ---- degenerate shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_rows_no_entries(handle, dtype):
    for M in (_assemble([], dtype), _assemble([([], [])] * 5, dtype)):
        got, cut, paths = _run(M, 3, handle)
        assert_bits(got, tr.of(M, 3)[0], "empty")
        assert cut == 0 and paths == {"copied": M.rows, "wave": 0, "block": 0, "stream": 0}


@pytest.mark.parametrize("dtype", DTYPES)
def test_k_beyond_every_row_is_a_copy(handle, dtype):
    rng = np.random.default_rng(23)
    long = _assemble([_special_row(n, max(n - 4, 0), rng, dtype) for n in (0, 9, 70, 1500, 9000, 1)], dtype)
    short = _assemble([_special_row(n, max(n - 4, 0), rng, dtype) for n in (0, 9, 70, N, 1)], dtype)   # no row longer than n
    for M, k in ((long, 9000), (long, INT_MAX), (short, N + 1), (short, N), (short, INT_MAX)):
        for normalise in (False, True):
            got, cut, paths = _run(M, k, handle, normalise)
            assert_bits(got, M, f"k={k}")
            assert cut == 0 and paths == {"copied": M.rows, "wave": 0, "block": 0, "stream": 0}


@pytest.mark.parametrize("dtype", DTYPES)
def test_k_1_is_the_attractor(handle, dtype):
    M = typed(with_nnz(2000, 2000, 60000, 5), dtype)
    d = M.toGpuCSR()
    try:
        parent = hs.rmcl_attractors(d, handle=handle)
        want = hs.d2h(parent, M.rows, np.int32)
        hs.dev_free(parent)
        got = take(d.row_topk(1, handle=handle))
    finally:
        d.deviceDispose()
    lens = np.diff(M.rowPtr)
    assert np.array_equal(np.diff(got.rowPtr), np.minimum(lens, 1))
    assert np.array_equal(got.colInd, want[lens > 0])


# ---- normalise -------------------------------------------------------------------------------------------------------
def _assert_normalised(got, M, k, what):
    """pattern, rowPtr and the rows that were not cut: the reference's bits.  Rows that were cut: float within 2 ulp of
    fl32(v / fl32(fsum)) (the device's double sum of k floats is within k * 2^-53 of the exact sum, so it rounds to the float
    fsum rounds to or to its neighbour; a divisor one ulp off moves the quotient by at most one ulp before its own
    rounding); double within (k + 1) * 2^-53 * want (k - 1 additions of non-negative terms in any tree, one division)."""
    want, _ = tr.of(M, k, normalise=True)
    assert np.array_equal(got.rowPtr, want.rowPtr) and np.array_equal(got.colInd, want.colInd), what
    was_cut = np.repeat(np.diff(M.rowPtr) > k, np.diff(want.rowPtr))
    g, w = got.values, want.values
    assert g.dtype == w.dtype
    assert g[~was_cut].tobytes() == w[~was_cut].tobytes(), f"{what}: rows that were not cut"
    if g.dtype == np.float32:
        ulps = np.abs(g[was_cut].view(np.int32).astype(np.int64) - w[was_cut].view(np.int32).astype(np.int64))
        assert ulps.max(initial=0) <= 2, (what, int(ulps.max()))
    else:
        err = np.abs(g[was_cut] - w[was_cut])
        assert np.all(err <= (k + 1) * 2.0 ** -53 * w[was_cut]), (what, float(err.max()))
    return was_cut


@pytest.mark.parametrize("dtype", DTYPES)
def test_normalise_divides_only_the_rows_that_were_cut(handle, dtype):
    wave, block = hs.row_topk_limits(dtype)
    rng = np.random.default_rng(29)
    lengths = [0, 5, 8, 9, 100, 40, wave, wave + 1, 3, block, block + 1]
    M = _assemble([(rng.integers(0, N, size=n), rng.random(n) + 2.0 ** -20) for n in lengths], dtype)
    for k in (8, 40):
        got, cut, paths = _run(M, k, handle, normalise=True)
        was_cut = _assert_normalised(got, M, k, f"normalise k={k}")
        assert cut == sum(n > k for n in lengths) and paths == _expected_paths(M, k, dtype)
        assert paths["wave"] and paths["block"] and paths["stream"] and was_cut.any() and not was_cut.all()
        sums = np.add.reduceat(got.values.astype(np.float64), got.rowPtr[:-1][np.diff(got.rowPtr) > 0])
        cut_rows = (np.diff(M.rowPtr) > k)[np.diff(got.rowPtr) > 0]
        assert np.allclose(sums[cut_rows], 1.0, rtol=0, atol=k * 2.0 ** -23)
        again, _, _ = _run(M, k, handle, normalise=True)
        assert again.values.tobytes() == got.values.tobytes() and np.array_equal(again.colInd, got.colInd)


# ---- a random matrix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 40])
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_matrix(handle, dtype, k):
    M = typed(with_nnz(2000, 2000, 60000, 3), dtype)
    paths = _check(M, k, handle, f"random k={k}")
    assert paths["wave"] > 0 and (k == 8 or paths["copied"] > 0)      # mean row length 30: k = 8 cuts every row
    got, cut, _ = _run(M, k, handle, normalise=True)
    _assert_normalised(got, M, k, f"random normalised k={k}")
    assert cut == int((np.diff(M.rowPtr) > k).sum())
