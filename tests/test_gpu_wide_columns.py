"""GPU (-m gpu): every column-keyed kernel at column indices up to 2^31 - 2.

The product cases are built over 200 000 compact columns (tests/wide_columns.py), multiplied there by the CPU reference
once, and B is relabelled by a strictly increasing map onto up to 2^31 - 1 columns: the device result must equal the
relabelled reference in rowPtr, per-row sorted columns and value BITS (every sum of a case is exact, so there is no
tolerance anywhere in this module).  tests/test_wide_columns_ref.py proves the relabelling identity on the CPU for these
very cases.  Beside the result every test asserts the route: the handle's bin counts, the direct / fallback rows of the
big-row kernels, the path counters of the mid-row kernels.

Widths: 2^30 + 1; 2^31 - 2^20, the last whose symbolic windows end below 2^31; 2^31 - 2^20 + 1; 2^31 - 1.  A big row
(more than 4096 products) costs one bitmap window per 2^20 columns in the symbolic pass, 2048 of them at the widest:
the cases hold at most four such rows.
"""
import numpy as np
import pytest

import topk_ref as tr
import wide_columns as wc
from devcsr import assert_bits, bigrow_twice, env_handle, same_bits, take
from reorder_ref import Host
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu

NMAX = wc.W[-1]                 # 2^31 - 1: columns up to 2^31 - 2
INT_MAX = 2 ** 31 - 1
DTYPES = [np.float32, np.float64]
ERR_INPUT = "status 5"          # SPGEMM_ERR_INPUT in the message of hs.SpgemmError


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()
    assert hs.device_count() >= 1, "GPU tests need a HIP device (no CPU fallback exists)"


# ---- cases, maps and relabelled references: made once, never modified ------------------------------------------------------
_CASES, _PHI, _WIDE = {}, {}, {}
_MAKERS = {"bins": wc.case_bins, "big": wc.case_big, "mid": wc.case_mid, "wide-f64": wc.case_wide_f64,
           "bins-f64": lambda: wc.case_bins(np.float64), "big-f64": lambda: wc.case_big(np.float64)}


def _case(name):
    if name not in _CASES:
        _CASES[name] = wc.case_sym(int(name[4:])) if name.startswith("sym-") else _MAKERS[name]()
    return _CASES[name]


def _phi(map_name, n):
    if (map_name, n) not in _PHI:
        _PHI[map_name, n] = wc.phi(map_name, wc.N0, n)
    return _PHI[map_name, n]


def _wide(name, map_name, n):
    """-> (the case, B on n columns, the reference on n columns)"""
    key = (name, map_name, n)
    if key not in _WIDE:
        case, f = _case(name), _phi(map_name, n)
        _WIDE[key] = (case, wc.relabel(case.B, f, n), wc.relabel(case.want(), f, n))
    return _WIDE[key]


def _dev(M):
    return hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols, dtype=np.asarray(M.values).dtype).toGpuCSR()


def _mul(h, A, B):
    dA, dB = _dev(A), _dev(B)
    try:
        return take(hs.gpuSpMMWrapper(dA, dB, h))
    finally:
        dA.deviceDispose()
        dB.deviceDispose()


def _same(got, want, what):
    """rowPtr, per-row sorted columns, value bits; either value type"""
    assert (got.rows, got.cols) == (want.rows, want.cols), f"{what}: shape"
    if not wc.is_double(want):
        return same_bits(got, want, what)
    g, w = wc.sorted_bits(got), wc.sorted_bits(want)
    assert g[0] == w[0], f"{what}: rowPtr differs"
    assert g[1] == w[1], f"{what}: columns differ"
    assert g[3] == w[3] == "float64" and g[2] == w[2], f"{what}: value bits differ"


# ---- a. every bin; e. the same in double ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", wc.W)
@pytest.mark.parametrize("map_name", wc.MAPS)
@pytest.mark.parametrize("name", ["bins", "bins-f64"])
def test_every_bin(name, map_name, n):
    """rows of 0 ... 4097 products, each all-distinct and half-repeated; the handle reports the bins they were built for"""
    case, B, want = _wide(name, map_name, n)
    h = env_handle()
    try:
        got = _mul(h, case.A, B)
        st = h.stats()
    finally:
        h.close()
    assert st["bin_rows"] == wc.bin_rows(case.products) == [2, 2, 4, 4, 4, 4, 4, 4, 2], st
    print(f"{name} {map_name} n={n}: symbolic {st['ms_symbolic']:.3f} ms, call {st['ms_total']:.3f} ms")
    assert st["total_flops"] == int(case.products.sum()) and st["nnzC"] == want.nnz, st
    _same(got, want, f"{name} {map_name} n={n}")


# ---- b. big rows, float: the hash kernel with classes and parking, then the direct kernel with the re-hit log -------------------
def _bigrow_cap():
    h = env_handle()
    try:
        return h.bigrow_paths()["cap"]
    finally:
        h.close()


@pytest.mark.parametrize("n", wc.W)
@pytest.mark.parametrize("map_name", wc.MAPS)
def test_big_rows_hash_then_direct(map_name, n):
    """first call on a fresh handle: every big row in k_num_bighash (12 288 distinct columns: two classes, parked products);
    second call: the rows with at most cap re-hits in k_num_bigdirect, the 4200-on-70 row stays with the hash kernel"""
    case, B, want = _wide("big", map_name, n)
    direct = int((case.rehits <= _bigrow_cap()).sum())
    assert 1 <= direct < len(case.products)
    bigrow_twice(case.A, B, f"big {map_name} n={n}", direct=direct, want=want)


@pytest.mark.parametrize("n", wc.W)
@pytest.mark.parametrize("map_name", wc.MAPS)
def test_big_rows_double(map_name, n):
    """e: the same rows through hip_gpuSpMM_f64, twice on one handle (LDS table, multi-pass LDS table)"""
    case, B, want = _wide("big-f64", map_name, n)
    h = env_handle()
    try:
        for call in ("first", "second"):
            got = _mul(h, case.A, B)
            st = h.stats()
            print(f"big-f64 {map_name} n={n} ({call} call): symbolic {st['ms_symbolic']:.3f} ms, call {st['ms_total']:.3f} ms")
            assert st["bin_rows"][8] == len(case.products)
            _same(got, want, f"big-f64 {map_name} n={n} ({call} call)")
    finally:
        h.close()


def test_widest_row_double():
    """e: 163 904 distinct columns in one row, spread over all 2048 windows: the device-memory table of the double path"""
    case, B, want = _wide("wide-f64", "spread", NMAX)
    h = env_handle()
    try:
        got = _mul(h, case.A, B)
        st = h.stats()
        print(f"wide-f64: symbolic {st['ms_symbolic']:.3f} ms, call {st['ms_total']:.3f} ms")
        assert st["bin_rows"][8] == 1
    finally:
        h.close()
    _same(got, want, "wide-f64")


# ---- c. mid rows (513-4096 products), float -----------------------------------------------------------------------------------
WCAP = 448                      # re-hits the wave-per-row kernel takes
MD_SLOTS = {0: 1024, 1: 1024, 2: 2048, 3: 2048}         # SPGEMM_MD_CFG -> table slots of k_num_middirect; the cap is 7/8
MID_ENVS = {"default": {}, "wave": {"SPGEMM_MD_WAVE": 1},
            "pair": {"SPGEMM_SYM_PAIR": 1, "SPGEMM_SP_MINROWS": 0}, "no-pair": {"SPGEMM_SYM_PAIR": 0, "SPGEMM_SP_MINROWS": 0}}
MID_ENVS.update({f"cfg{c}": {"SPGEMM_MD_CFG": c, "SPGEMM_MD_WAVE": 0} for c in MD_SLOTS})


@pytest.mark.parametrize("env_name", sorted(MID_ENVS))
@pytest.mark.parametrize("map_name", ["top", "edges"])
def test_mid_rows_every_route(map_name, env_name):
    """three products on a fresh handle: the first has no log and keeps the hash kernels; the second and the third take the
    wave kernel (at most 448 re-hits, bin 6), the four-wave kernel (at most cap) or the hash kernel of their bin, as planned
    from the planted re-hits; with SPGEMM_SYM_PAIR the rows of bin 6 are logged by k_sym_midpair, else by k_sym_hash"""
    env = MID_ENVS[env_name]
    case, B, want = _wide("mid", map_name, NMAX)
    f, planted = case.products, case.rehits
    b6 = (f > 512) & (f <= 2048)
    nmid, n6 = len(f), int(b6.sum())
    cap = MD_SLOTS[env.get("SPGEMM_MD_CFG", 0)] // 8 * 7
    waves = b6 & (planted <= WCAP) if env.get("SPGEMM_MD_WAVE", 1) else np.zeros_like(b6)
    direct = planted <= cap
    plan = (int(waves.sum()), int((b6 & direct & ~waves).sum()), int((~direct).sum()))
    assert plan[2] >= 1 and plan[1] >= 2 and (plan[0] >= 3 or not env.get("SPGEMM_MD_WAVE", 1)), plan
    h = env_handle(SPGEMM_MD_MINROWS=1, SPGEMM_MW_MINROWS=1, **env)
    try:
        for call in ("first", "second", "third"):
            what = f"mid {map_name} {env_name} ({call} call)"
            got = _mul(h, case.A, B)
            p = h.midrow_paths()
            _same(got, want, what)
            assert p["rows"] == nmid and p["cap"] == cap, f"{what}: {p}"
            if "SPGEMM_SYM_PAIR" in env:
                sp = h.midrow_sym_paths()
                assert sp == ({"pair": n6, "multiwave": 0} if env["SPGEMM_SYM_PAIR"] else {"pair": 0, "multiwave": n6}), f"{what}: {sp}"
            if call == "first":
                assert (p["direct"], p["wave"], p["multiwave"], p["fallback"]) == (0, 0, 0, nmid), f"{what}: {p}"
                continue
            assert (p["wave"], p["multiwave"], p["fallback"]) == plan and p["direct"] == nmid - plan[2], f"{what}: {p}"
            assert p["logged"] == int(planted[direct].sum()), f"{what}: {p}"
    finally:
        h.close()


# ---- d. the symbolic pass alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", wc.W)
@pytest.mark.parametrize("map_name", ["spread", "edges"])
def test_symbolic_alone(map_name, n):
    """hip_spgemm_symbolic: IC row by row and nnz; row 0 holds exactly the window-edge columns of `edges` at this width"""
    case, B, want = _wide(f"sym-{n}", map_name, n)
    A = case.A
    dA, dB = _dev(A), _dev(B)
    ic = hs.dev_alloc(4 * (A.rows + 1))
    h = env_handle()
    try:
        nnz = hs.spgemm_symbolic_raw(h, dA.rowPtr, dA.colInd, A.nnz, dB.rowPtr, dB.colInd, B.nnz, A.rows, A.cols, n, ic)
        got = hs.d2h(ic, A.rows + 1, np.int32)
        st = h.stats()
    finally:
        h.close()
        hs.dev_free(ic)
        dA.deviceDispose()
        dB.deviceDispose()
    print(f"symbolic alone {map_name} n={n}: symbolic {st['ms_symbolic']:.3f} ms, call {st['ms_total']:.3f} ms")
    lens = np.diff(got.astype(np.int64))
    assert lens[0] == len(wc.edge_columns(n)) == case.claims[0, 1], f"edge row: {lens[0]}"
    assert np.array_equal(lens, case.claims[:, 1]), np.flatnonzero(lens != case.claims[:, 1])
    assert np.array_equal(got, np.asarray(want.rowPtr, np.int32)) and nnz == want.nnz
    assert st["bin_rows"] == wc.bin_rows(case.products) and st["bin_rows"][8] == 3, st


# ---- f. the row tools ----------------------------------------------------------------------------------------------------------
HALVES = np.array([0, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 2], np.int64)       # both sides of bit 30, and the two ends


def _columns(count, seed):
    """`count` distinct columns below 2^31 - 1 from both halves of bit 30, shuffled; 2^31 - 2, 0, 2^30 and 2^30 - 1 are among
    them, in this order of preference when the row is shorter than four"""
    rng = np.random.default_rng(seed)
    fixed = HALVES[[3, 0, 2, 1]][:min(count, 4)]
    pool = np.unique(rng.integers(0, INT_MAX - 1, size=2 * count + 8))
    pool = rng.permutation(pool[~np.isin(pool, HALVES)])[:count - len(fixed)]
    keep = np.r_[fixed, pool].astype(np.int64)
    assert len(keep) == count
    return rng.permutation(keep)


def _values(count, dtype, seed):
    v = np.random.default_rng(seed).integers(1, 1 << 20, size=count).astype(dtype)
    return v + dtype(2.0 ** -30) if np.dtype(dtype) == np.float64 else v


@pytest.mark.parametrize("dtype", DTYPES)
def test_sort_rows(dtype):
    """rows of 2, 4096 (the bitonic kernel's longest) and 4097 entries (the radix kernel, four passes over 31 key bits)"""
    lens = [2, 0, 4096, 4097, 1]
    cols = [_columns(k, 60 + i) for i, k in enumerate(lens)]
    rp = np.r_[0, np.cumsum(lens)]
    M = Host(rp, np.concatenate(cols), _values(int(rp[-1]), dtype, 61), len(lens), NMAX)
    assert (M.colInd[rp[3]:rp[4]] >= 2 ** 30).any() and (M.colInd[rp[3]:rp[4]] < 2 ** 30).any() and 2 ** 31 - 2 in M.colInd[rp[3]:rp[4]]
    order = np.concatenate([rp[i] + np.argsort(c, kind="stable") for i, c in enumerate(cols)])
    d = _dev(M)
    hs.sort_rows_device(d)
    assert_bits(take(d), Host(rp, M.colInd[order], M.values[order], M.rows, NMAX), f"sort {np.dtype(dtype)}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_coo_to_csr(dtype):
    """50 rows, 2^31 - 1 columns: a key of 6 + 31 bits; duplicates summed under COO_DEDUPE (integers: exact in any order)"""
    rng = np.random.default_rng(62)
    rows, count = 50, 3000
    ri, ci = rng.integers(0, rows, size=count), HALVES[rng.integers(0, 4, size=count)]
    v = rng.integers(1, 9, size=count).astype(dtype)
    key = ri * (1 << 31) + ci
    ukey, inv = np.unique(key, return_inverse=True)
    sums = np.zeros(len(ukey), dtype)
    np.add.at(sums, inv, v)
    rp = np.r_[0, np.cumsum(np.bincount(ukey >> 31, minlength=rows))]
    assert len(ukey) < count and len(ukey) > 150
    got = take(hs.coo_to_csr(rows, NMAX, ri, ci, v, hs.COO_DEDUPE, dtype=dtype))
    assert_bits(got, Host(rp, ukey & (2 ** 31 - 1), sums, rows, NMAX), f"coo {np.dtype(dtype)}")
    with pytest.raises(hs.SpgemmError, match=ERR_INPUT):                    # a column equal to cols = INT_MAX: no launch
        hs.coo_to_csr(rows, INT_MAX, ri[:4], np.array([0, 1, INT_MAX, 2]), v[:4], hs.COO_DEDUPE, dtype=dtype)


def _topk_paths(M, k, dtype):
    wave, block = hs.row_topk_limits(dtype)
    want = {"copied": 0, "wave": 0, "block": 0, "stream": 0}
    for length in np.diff(M.rowPtr):
        want["copied" if length <= k else "wave" if length <= wave else "block" if length <= block else "stream"] += 1
    return want


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_topk_ties_on_the_widest_columns(dtype):
    """value ties at columns 2^31 - 2, 2^30 and 0 in a row of the wave, the block and the stream path: the smaller column
    wins, and the entry at 2^31 - 2 (ck = INT_MAX - column = 1, the smallest non-zero key) is still counted: with k one
    below the row length it is the one entry dropped, with a larger value it is the one entry kept by k = 1"""
    wave, block = hs.row_topk_limits(dtype)
    lens = [70, wave, wave + 1, block, block + 1]
    h = env_handle()
    try:
        for variant in ("all tied", "last column largest"):
            rows = []
            for i, length in enumerate(lens):
                c = _columns(length, 70 + i)
                v = np.full(length, 0.75, dtype)
                if variant != "all tied":
                    v[c == 2 ** 31 - 2] = 1.5
                    v[c == 0] = 0.25
                rows.append((c, v))
            rp = np.r_[0, np.cumsum(lens)]
            M = Host(rp, np.concatenate([c for c, _ in rows]), np.concatenate([v for _, v in rows]), len(lens), NMAX)
            for k in (1, 2, 3, 69):
                d = _dev(M)
                try:
                    before = h.topk_paths()
                    out = d.row_topk(k, handle=h)
                    after = h.topk_paths()
                finally:
                    d.deviceDispose()
                want, want_cut = tr.of(M, k)
                got = take(out)
                what = f"topk {np.dtype(dtype)} {variant} k={k}"
                assert_bits(got, want, what)
                assert out.rows_cut == want_cut == len(lens), what
                assert {p: after[p] - before[p] for p in after} == _topk_paths(M, k, dtype), what
                first = got.colInd[got.rowPtr[:-1]] if k == 1 else None
                if k == 1:
                    assert (first == (0 if variant == "all tied" else 2 ** 31 - 2)).all(), what
                if k == 69:
                    assert (2 ** 31 - 2 in got.colInd[:69]) == (variant != "all tied"), what
        with pytest.raises(hs.SpgemmError, match=ERR_INPUT):                # a column equal to cols = INT_MAX: no launch
            d = _dev(Host([0, 3], [0, INT_MAX, 5], np.ones(3, dtype), 1, INT_MAX))
            try:
                d.row_topk(1, handle=h)
            finally:
                d.deviceDispose()
    finally:
        h.close()


def _sorted_host(M):
    rp = np.asarray(M.rowPtr, np.int64)
    order = np.lexsort((np.asarray(M.colInd, np.int64), np.repeat(np.arange(M.rows), np.diff(rp))))
    return Host(M.rowPtr, np.asarray(M.colInd)[order], np.asarray(M.values)[order], M.rows, M.cols)


def _operands(dtype):
    """two row-sorted compact matrices that share most of their pattern: the big rows' product, and the same with every
    third entry gone and other values"""
    X = _sorted_host(_case("big" if np.dtype(dtype) == np.float32 else "big-f64").want())
    keep = np.arange(X.nnz) % 3 != 1
    rp = np.r_[0, np.cumsum(np.add.reduceat(keep.astype(np.int64), X.rowPtr[:-1]))]
    Y = Host(rp, X.colInd[keep], (X.values[keep] * 0.5).astype(dtype), X.rows, X.cols)
    return X, Y


@pytest.mark.parametrize("map_name", wc.MAPS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_and_diff(dtype, map_name):
    """hip_csr_add and hip_csr_diff on two relabelled operands against the relabelled result / the report of the compact call"""
    X, Y = _operands(dtype)
    f = _phi(map_name, NMAX)
    h = env_handle()
    try:
        outs = []
        for A, B in ((X, Y), (wc.relabel(X, f, NMAX), wc.relabel(Y, f, NMAX))):
            dA, dB = _dev(A), _dev(B)
            try:
                outs.append((take(dA.add(dB, 2.0, -3.0, handle=h)), dA.diff(dB, handle=h).as_dict()))
            finally:
                dA.deviceDispose()
                dB.deviceDispose()
    finally:
        h.close()
    (csum, cdiff), (wsum, wdiff) = outs
    assert csum.nnz == X.nnz and cdiff["only_a"] == X.nnz - Y.nnz > 0 and cdiff["only_b"] == 0
    assert_bits(wsum, wc.relabel(Host(csum.rowPtr, csum.colInd, csum.values, csum.rows, csum.cols), f, NMAX), f"add {map_name}")
    assert wdiff == cdiff, (wdiff, cdiff)


@pytest.mark.parametrize("c", [2, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_split_columns_and_join(dtype, c):
    """hip_csr_split_columns / hip_pcsr_join at 2^31 - 1 columns: the entries per block, the local column of the last
    column in the last block, and the round trip"""
    X = wc.relabel(_operands(dtype)[0], _phi("spread", NMAX), NMAX)
    stride = (NMAX + c - 1) // c
    h = env_handle()
    d = _dev(X)
    try:
        P = hs.PCSR(d, c, handle=h)
        try:
            assert P.stride == stride
            assert np.array_equal(np.diff(P.blockPtr), np.bincount(X.colInd.astype(np.int64) // stride, minlength=c))
            last = P.block(c - 1).toCpuCSR()
            mine = X.colInd.astype(np.int64) // stride == c - 1
            assert last.nnz == int(mine.sum()) > 0 and last.colInd.max() == NMAX - 1 - (c - 1) * stride
            assert np.array_equal(np.sort(last.colInd.astype(np.int64) + (c - 1) * stride), np.sort(X.colInd[mine].astype(np.int64)))
            assert_bits(take(P.join(handle=h)), X, f"join c={c}")
        finally:
            P.deviceDispose()
    finally:
        d.deviceDispose()
    bad = _dev(Host([0, 3], [0, 5, INT_MAX], np.ones(3, dtype), 1, INT_MAX))
    try:
        with pytest.raises(hs.SpgemmError, match=ERR_INPUT):                # a column equal to cols = INT_MAX: no launch
            hs.PCSR(bad, c, handle=h)
    finally:
        bad.deviceDispose()
        h.close()
