"""GPU (-m gpu): every numeric kernel at its table and window edges, compared BIT FOR BIT.

The inputs come from tests/edge_cases.py: rows that sit exactly on both sides of every bin, layout slot and size-class
boundary, in three walk shapes and four column regimes (all distinct / one column / half repeated / cancelling to 0.0), at
the widths where the big-row kernels change (rank | hash kernel, one | two symbolic windows), with columns on the bitmap
word, group and window seams; single rows on the capacity edges of the rank, hash and double tables; and strided column
progressions.  All values are small integers, so every float32 and float64 partial sum is exact in any order
(edge_cases' docstring has the bound) and the comparison needs no tolerance: rowPtr equal, per-row-sorted colInd equal,
values equal as bit patterns, and stats() must report the products, entries and bin populations the case intends -- which
proves that the rows ran where they were aimed.  tests/test_edge_cases_ref.py checks the expectation itself on the CPU.
"""
import numpy as np
import pytest

import edge_cases as ec
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()
    assert hs.device_count() >= 1, "GPU tests need a HIP device (no CPU fallback exists)"


def handle_with(monkeypatch, **env):
    """a handle created under SPGEMM_* settings (a handle reads them when it is made)"""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    h = hs.Handle(0)
    for k in env:
        monkeypatch.delenv(k)
    return h


class OnDevice:
    """A and B of a case uploaded once per value type"""

    def __init__(self, case):
        self.case = case
        self._d = {}

    def get(self, dtype):
        if dtype not in self._d:
            c = self.case
            up = lambda M: hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values.astype(dtype), M.rows, M.cols, dtype=dtype).toGpuCSR()
            self._d[dtype] = (up(c.A), up(c.B))
        return self._d[dtype]

    def dispose(self):
        for dA, dB in self._d.values():
            dA.deviceDispose()
            dB.deviceDispose()
        self._d = {}


def assert_exact(got, case, dtype, what):
    """rowPtr, sorted colInd and the BITS of the values equal the exact expectation"""
    assert got.rows == case.A.rows and got.cols == case.n
    rp = np.asarray(got.rowPtr)
    if not np.array_equal(rp, case.rowPtr):
        bad = int(np.nonzero(np.diff(rp) != np.diff(case.rowPtr))[0][0])
        raise AssertionError(f"{what}: row {bad} {case.recipes[bad][:4]} has {np.diff(rp)[bad]} entries, expected {np.diff(case.rowPtr)[bad]}")
    row_of = np.repeat(np.arange(got.rows, dtype=np.int64), np.diff(rp.astype(np.int64)))
    order = np.lexsort((np.asarray(got.colInd), row_of))
    gc, gv = np.asarray(got.colInd)[order], np.asarray(got.values)[order]
    assert gv.dtype == dtype
    if not np.array_equal(gc, case.colInd):
        bad = int(row_of[np.nonzero(gc != case.colInd)[0][0]])
        raise AssertionError(f"{what}: columns of row {bad} {case.recipes[bad][:4]} differ")
    bits = np.uint32 if dtype == np.float32 else np.uint64
    wv = case.values.astype(dtype)
    same = gv.view(bits) == wv.view(bits)
    if not same.all():
        i = int(np.nonzero(~same)[0][0])
        bad = int(row_of[i])
        raise AssertionError(f"{what}: {int((~same).sum())} values differ, first in row {bad} {case.recipes[bad][:4]} col {gc[i]}: "
                             f"{gv[i]!r} vs {wv[i]!r}")


def assert_stats(h, case, what):
    st, want = h.stats(), ec.expected_stats(case)
    got = {k: st[k] for k in want}
    assert got == want, f"{what}: stats {got} vs intended {want}"


def one_shot(h, dev, dtype, what, stats=True):
    dA, dB = dev.get(dtype)
    dC = hs.gpuSpMMWrapper(dA, dB, h)
    try:
        got = dC.toCpuCSR()
    finally:
        dC.deviceDispose()
    assert_exact(got, dev.case, dtype, what)
    if stats:
        assert_stats(h, dev.case, what)
    return got


def two_phase(h, dev, what):
    """hip_spgemm_symbolic + hip_spgemm_numeric into caller-owned buffers"""
    c = dev.case
    dA, dB = dev.get(np.float32)
    args = (dA.rowPtr, dA.colInd, dA.values, c.A.nnz, dB.rowPtr, dB.colInd, dB.values, c.B.nnz, c.A.rows, c.A.cols, c.n)
    IC = hs.dev_alloc(4 * (c.A.rows + 1))
    JC = VC = 0
    try:
        nnz = hs.spgemm_symbolic_raw(h, dA.rowPtr, dA.colInd, c.A.nnz, dB.rowPtr, dB.colInd, c.B.nnz, c.A.rows, c.A.cols, c.n, IC)
        assert nnz == len(c.colInd), f"{what}: symbolic phase counts {nnz} entries, expected {len(c.colInd)}"
        JC, VC = hs.dev_alloc(4 * nnz), hs.dev_alloc(4 * nnz)
        hs.spgemm_numeric_raw(h, *args, IC, JC, VC)
        got = hs.CSR(VC, JC, IC, c.A.rows, c.n, nnz, True, dtype=np.float32).toCpuCSR()
    finally:
        for p in (IC, JC, VC):
            hs.dev_free(p)
    assert_exact(got, c, np.float32, what)
    assert_stats(h, c, what)


# ---- the edge grid: every bin / slot / size-class edge x shape x regime, at every width where the kernels change ----------
@pytest.fixture(scope="module", params=ec.GRID_N, ids=lambda n: f"n{n}")
def grid(request):
    dev = OnDevice(ec.edge_grid(request.param))
    yield dev
    dev.dispose()


def test_grid_one_shot_twice_on_one_handle(grid):
    """hip_gpuSpMM on a fresh handle, then again: with n <= BIG_WC the second call's rank kernel reloads the bitmaps the
    symbolic pass saved (the first call had no room for them and rebuilt them)."""
    h = hs.Handle(0)
    try:
        first = one_shot(h, grid, np.float32, f"{grid.case.name}, first call")
        second = one_shot(h, grid, np.float32, f"{grid.case.name}, second call")
    finally:
        h.close()
    assert np.array_equal(first.rowPtr, second.rowPtr)


def test_grid_two_phase_into_caller_buffers(grid):
    h = hs.Handle(0)
    try:
        two_phase(h, grid, f"{grid.case.name}, symbolic + numeric")
    finally:
        h.close()


def test_grid_f64(grid):
    h = hs.Handle(0)
    try:
        one_shot(h, grid, np.float64, f"{grid.case.name}, f64")
    finally:
        h.close()


@pytest.fixture(scope="module")
def narrow_grid():
    dev = OnDevice(ec.edge_grid(ec.GRID_N[0]))
    yield dev
    dev.dispose()


@pytest.mark.parametrize("path", [1, 2])
def test_grid_opt_in_paths(monkeypatch, narrow_grid, path):
    """the wave-per-batch kernels (SPGEMM_PATH=1: two passes, 2: one pass) take the rows of the low bins; twice, as the
    one-pass form sizes C from the previous call"""
    h = handle_with(monkeypatch, SPGEMM_PATH=path)
    try:
        for call in (1, 2):
            one_shot(h, narrow_grid, np.float32, f"{narrow_grid.case.name}, SPGEMM_PATH={path}, call {call}")
    finally:
        h.close()


# ---- single rows on the capacity edges of the tables -----------------------------------------------------------------------
@pytest.fixture(scope="module", params=["rank", "hash"])
def capacity(request):
    dev = OnDevice(ec.capacity_rank_case() if request.param == "rank" else ec.capacity_hash_case())
    yield dev
    dev.dispose()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_capacity_rows(capacity, dtype):
    h = hs.Handle(0)
    try:
        one_shot(h, capacity, dtype, f"{capacity.case.name}, {np.dtype(dtype).name}")
    finally:
        h.close()


def test_capacity_rows_with_undersized_parking_regions(monkeypatch, capacity):
    """SPGEMM_BHMARGIN=60: every parking region of a multi-pass row is too small, the row is redone with a walk per pass"""
    h = handle_with(monkeypatch, SPGEMM_BHMARGIN=60)
    try:
        one_shot(h, capacity, np.float32, f"{capacity.case.name}, SPGEMM_BHMARGIN=60")
    finally:
        h.close()


# ---- strided columns -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", sorted({s for s, _ in ec.strided_patterns()}))
def test_strided_columns(stride):
    """One row with the columns i*stride: arithmetic progressions resonate with a multiplicative class hash (every column
    i*5599 falls into ONE class of the hash kernel's first attempt); the product has to come out all the same, in both
    value types.  The widest rows (up to 1.5e9 columns) walk some 1400 symbolic windows."""
    h = hs.Handle(0)
    try:
        for s, W in ec.strided_patterns():
            if s != stride:
                continue
            dev = OnDevice(ec.strided_case(s, W))
            try:
                for dtype in (np.float32, np.float64):
                    one_shot(h, dev, dtype, f"{dev.case.name}, {np.dtype(dtype).name}")
            finally:
                dev.dispose()
    finally:
        h.close()
