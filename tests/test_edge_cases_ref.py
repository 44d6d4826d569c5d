"""CPU: keeps tests/edge_cases.py honest.  Every recipe yields exactly the products and distinct columns it intends, the
restated bin_of / slot_of put the row where the case wants it, and the exact int64 expectation equals the oracle's
sequential_CSR_SpMM restatement bit for bit (float32 sums of these integers are exact in any order, see edge_cases)."""
import numpy as np
import pytest

import edge_cases as ec
from helpers import canonical_arrays, po


def check_case(case, oracle=True):
    F, D = case.intended[:, 0], case.intended[:, 1]
    assert np.array_equal(po.row_flops(case.A, case.B), F)
    assert np.array_equal(np.diff(case.rowPtr), D)
    assert F.max() <= ec.MAX_PRODUCTS
    # ascending and distinct inside every row
    rows = np.repeat(np.arange(case.A.rows), np.diff(case.rowPtr))
    key = rows.astype(np.int64) * case.n + case.colInd
    assert np.all(np.diff(key) > 0)
    if oracle:
        want = po.sequential_spmm(case.A, case.B)
        assert np.array_equal(want.rowPtr, case.rowPtr)
        wc, wv = canonical_arrays(want.rowPtr, want.colInd, want.values)
        assert np.array_equal(wc, case.colInd)
        assert np.array_equal(wv.view(np.uint32), case.values.astype(np.float32).view(np.uint32))
        assert np.array_equal(wv.astype(np.int64), case.values)


def test_restated_boundaries():
    assert [ec.bin_of(f) for f in ec.BIN_EDGES] == [0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8]
    assert [ec.slot_of(f) for f in ec.SLOT_EDGES] == [5, 6, 7, 8, 8, 9]
    assert [ec.bin_of(f) for f in ec.SLOT_EDGES] == [5, 5, 6, 6, 6, 7]
    assert [ec.slot_of(f) for f in ec.CLASS_EDGES] == [15, 14, 14, 13, 13, 12, 12, 11, 11, 10]
    assert ec.slot_of(4097) == 15 and ec.slot_of(ec.MAX_PRODUCTS) == 10 and ec.slot_of(4096) == 9
    assert all(ec.bin_of(f) == 8 for f in ec.CLASS_EDGES)
    # both sides of every edge are in the grid
    for hi in ec.BIN_UPPER + (ec.H1A_MAX, ec.H4A_MAX) + tuple(2 ** k - 1 for k in range(13, 18)):
        assert hi in ec.GRID_F and hi + 1 in ec.GRID_F
        assert ec.slot_of(hi) != ec.slot_of(hi + 1)


@pytest.mark.parametrize("n", ec.GRID_N)
def test_edge_grid(n):
    case = ec.edge_grid(n)
    assert case.A.rows == len(ec.GRID_F) * len(ec.SHAPES) * len(ec.REGIMES)
    for (F, D), rc in zip(case.intended, case.recipes):
        assert F == rc.F and D == ec.default_distinct(rc.F, rc.regime, n)
    # shapes: entries of A per row
    nA = np.diff(case.A.rowPtr)
    for i, rc in enumerate(case.recipes):
        assert nA[i] == {"one_long": 1, "unit_rows": rc.F, "rows16": (rc.F + 15) // 16}[rc.shape]
    # the regimes do what they say: "cancel" rows of even length are all zeros and keep their entries, the others none
    vals_of = lambda i: case.values[case.rowPtr[i]:case.rowPtr[i + 1]]
    cols_of = lambda i: case.colInd[case.rowPtr[i]:case.rowPtr[i + 1]]
    seams = ec.seam_columns(n)
    for i, rc in enumerate(case.recipes):
        v = vals_of(i)
        if rc.regime == "cancel" and rc.F % 2 == 0:
            assert len(v) == case.intended[i, 1] and not v.any()
        if rc.regime == "cancel" and rc.F % 2 == 1:
            assert np.count_nonzero(v) == 1
        if rc.regime == "distinct" and rc.F <= n:
            assert len(v) == rc.F and v.all()
        if case.intended[i, 1] >= len(seams):
            assert np.all(np.isin(seams, cols_of(i))), "a multi-column row leaves out a seam column"
    one = [cols_of(i)[0] for i, rc in enumerate(case.recipes) if rc.regime == "one_col" and rc.F]
    assert set(one) == set(seams.tolist())               # the single-column rows cover every seam between them
    st = ec.expected_stats(case)
    assert sum(st["bin_rows"]) == case.A.rows and all(st["bin_rows"][b] > 0 for b in range(ec.NBINS))
    assert {ec.slot_of(int(f)) for f in case.intended[:, 0]} == set(range(ec.NSLOTS))
    check_case(case)


def test_capacity_rows():
    r, h = ec.capacity_rank_case(), ec.capacity_hash_case()
    assert r.n <= ec.BIG_WC < h.n
    assert [int(d) for d in r.intended[:, 1]] == list(ec.CAP_RANK_D)
    assert [int(d) for d in h.intended[:, 1]] == list(ec.CAP_HASH_D) + [25000]
    passes = lambda d, cap: -(-d // cap)
    assert [passes(d, ec.BIG_CAP) for d in ec.CAP_RANK_D[:4]] == [1, 2, 2, 3]
    assert [passes(d, ec.BH_CAP) for d in ec.CAP_HASH_D[:5]] == [1, 2, 2, 3, ec.BH_MAXCLS + 1]
    # the last row: few enough classes to park, but more parked products than the buffer holds
    F, D = (int(x) for x in h.intended[-1])
    npass = passes(D, ec.BH_CAP)
    stride = min(F, F * ec.BH_MARGIN // (100 * npass) + 256)
    assert 1 < npass <= ec.BH_MAXCLS and (npass - 1) * stride > ec.BH_SPILL
    # ... while the rows before it park within it
    for D in ec.CAP_HASH_D[1:4]:
        npass = passes(D, ec.BH_CAP)
        assert (npass - 1) * min(D, D * ec.BH_MARGIN // (100 * npass) + 256) <= ec.BH_SPILL
    check_case(r)
    check_case(h)


def test_strided_rows():
    pats = ec.strided_patterns()
    assert len(pats) == 29 and (509, 300000) in pats and (5599, 23000) in pats
    assert (65536, 45000) not in pats and (65537, 45000) not in pats
    for s, W in pats:
        assert W * s < 2 ** 31
    for s, W in [(1, 17000), (5599, 23000), (509, 300000)]:
        case = ec.strided_case(s, W)
        assert case.n == W * s and np.array_equal(case.colInd, np.arange(W) * s)
        check_case(case, oracle=case.n <= 16_000_000)      # (the oracle keeps dense arrays of n entries)
