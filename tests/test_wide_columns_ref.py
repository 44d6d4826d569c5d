"""CPU: the reference of the wide-column GPU tests (tests/wide_columns.py) is right on its own.

At N_REF = 3 * 2^20 + 5 columns, which the C oracle can still hold, the product of A with a relabelled B equals the
relabelled product of A with B for every case and every map: rowPtr, sorted columns and value bits.  Every map is strictly
increasing and stays inside [0, n) at every width the GPU tests use, and every generated row has the product count and the
number of distinct columns its case claims."""
import numpy as np
import pytest

import wide_columns as wc

CASES = {"bins": wc.case_bins, "big": wc.case_big, "mid": wc.case_mid,
         "bins-f64": lambda: wc.case_bins(np.float64), "big-f64": lambda: wc.case_big(np.float64),
         "wide-f64": wc.case_wide_f64}
CASES.update({f"sym-{n}": (lambda n=n: wc.case_sym(n)) for n in wc.W + (wc.N_REF,)})
_MADE = {}


def _case(name):
    if name not in _MADE:
        _MADE[name] = CASES[name]()
    return _MADE[name]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("n", wc.W + (wc.N_REF,))
@pytest.mark.parametrize("name", wc.MAPS)
def test_maps_are_strictly_increasing_and_inside(name, n):
    f = wc.phi(name, wc.N0, n)
    assert f.dtype == np.int64 and len(f) == wc.N0
    assert f[0] >= 0 and f[-1] <= n - 1 and (np.diff(f) >= 1).all()
    if name == "top":
        assert f[0] == n - wc.N0 and f[-1] == n - 1
    if name == "spread":
        assert f[0] == 0 and f[-1] == n - 1 and len(np.unique(f // wc.WC)) == (n + wc.WC - 1) // wc.WC     # every window
    if name == "edges":
        E, p = wc.edge_columns(n), wc.edge_positions(wc.N0, n)
        assert np.array_equal(f[p], E) and E[-1] == n - 1
        for w in wc.EDGE_WINDOWS:
            for c in (w * wc.WC - 1, w * wc.WC):
                assert (c in E) == (c < n)


def test_the_widths():
    assert wc.W == (2 ** 30 + 1, 2 ** 31 - 2 ** 20, 2 ** 31 - 2 ** 20 + 1, 2 ** 31 - 1)
    assert wc.N_REF == 3 * 2 ** 20 + 5 and wc.N0 <= 200000


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_are_what_the_case_claims(name):
    """products from the operands, distinct columns from the reference product"""
    case = _case(name)
    assert np.array_equal(wc.row_products(case.A, case.B), case.products), name
    assert np.array_equal(np.diff(np.asarray(case.want().rowPtr, np.int64)), case.claims[:, 1]), name
    assert (np.diff(np.asarray(case.B.rowPtr)) <= wc.L).all() and case.B.cols == wc.N0
    cols = np.asarray(case.B.colInd)
    assert cols.min() == 0 and cols.max() == wc.N0 - 1            # so that `spread` and `edges` reach column 0 and n - 1
    v = np.asarray(case.B.values, np.float64)
    if wc.is_double(case.B):
        k = v * 2.0 ** 30
        assert (k == np.floor(k)).all() and (k % 2 == 1).all() and (k < 2 ** 12).all()
    else:
        assert set(np.unique(v)) <= {1.0, 2.0, 3.0, 4.0}


def test_the_cases_cover_what_they_are_for():
    assert wc.bin_rows(_case("bins").products) == [2, 2, 4, 4, 4, 4, 4, 4, 2]
    big = _case("big")
    assert (big.products > 4096).all() and len(big.products) <= 4
    assert big.claims[:, 1].max() > wc.BH_CAP and (70 in big.claims[:, 1]) and (4097 in big.products)
    mid = _case("mid")
    assert ((mid.products > 512) & (mid.products <= 4096)).all()
    assert _case("wide-f64").claims[0, 1] > 163840
    for n in wc.W:
        sym = _case(f"sym-{n}")
        rp = np.asarray(sym.A.rowPtr)
        used = np.unique(np.concatenate([sym.B.colInd[sym.B.rowPtr[e]:sym.B.rowPtr[e + 1]] for e in sym.A.colInd[rp[0]:rp[1]]]))
        assert np.array_equal(wc.phi("edges", wc.N0, n)[used], wc.edge_columns(n)) and sym.products[0] > 4096


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("map_name", wc.MAPS)
def test_relabelling_commutes_with_the_product(name, map_name):
    case = _case(name)
    f = wc.phi(map_name, wc.N0, wc.N_REF)
    got = wc.product(case.A, wc.relabel(case.B, f, wc.N_REF))
    want = wc.relabel(case.want(), f, wc.N_REF)
    assert got.cols == want.cols == wc.N_REF
    g, w = wc.sorted_bits(got), wc.sorted_bits(want)
    assert g[0] == w[0], f"{name} {map_name}: rowPtr"
    assert g[1] == w[1], f"{name} {map_name}: columns"
    assert g[3] == w[3] and g[2] == w[2], f"{name} {map_name}: value bits"
