"""GPU (-m gpu): rows of 513-4096 products (bins 6 and 7), where the symbolic pass logs the re-hit columns and the direct
kernel (k_num_middirect) keeps only those in a small table, against the hash kernels of the two bins it falls back to.

B is built from disjoint rows, so the re-hits of every row of A are planted exactly: a copy of a B row the row already uses
adds as many re-hits as it has columns, a one-column B row adds one.  The planted count is checked on the CPU (products minus
the oracle's row length) before anything is asserted about it.  Values are small integers (any summation order is exact);
the result is compared with the CPU oracle after a per-row sort: rowPtr, columns and value BITS.  A handle sizes the log at
the end of its first call with such rows, so `run()` multiplies twice on a fresh handle: the first call takes the hash
kernels for every row, the second the planned split (Handle.midrow_paths() says which ran, and how much was logged).
"""
import numpy as np
import pytest

from devcsr import env_handle, to_hs
from devcsr import int_csr as _csr
from devcsr import row_flops as _flops
from devcsr import same_bits as _same
from helpers import po
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu

N_LO = 200000                   # below the 262 144 columns of the rank kernel
N_HI = 262208                   # above: the big rows take the hash / direct big-row kernels
S = 1024                        # table slots of the default geometry; the cap is 7/8 of them
T = 256                         # ... and its smallest table (4 waves)


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()
    assert hs.device_count() >= 1, "GPU tests need a HIP device (no CPU fallback exists)"


def _handle(**env):
    """a fresh handle; the SPGEMM_* knobs are read when it is created.  SPGEMM_MD_MINROWS=1 unless the caller says otherwise: a
    bin with fewer rows than four per CU keeps the hash kernel by default, and these cases are a handful of rows"""
    env.setdefault("SPGEMM_MD_MINROWS", 1)
    return env_handle(**env)


def _cap(**env):
    h = _handle(**env)
    try:
        return h.midrow_paths()["cap"]
    finally:
        h.close()


class Bld:
    """B rows over n columns: 64 disjoint rows of 64 columns (the walk's long entries), 512 disjoint rows of 8 (flattened
    entries, several 64-entry groups per row of A), and on demand prefixes, copies and one-column rows of them.  A row of A
    is the sorted list of the B rows it uses; rows of A share B rows freely, only repeats inside one row plant re-hits."""

    def __init__(self, n, seed, reserve=()):
        rng = np.random.default_rng(seed)
        perm = rng.permutation(n)
        perm = perm[~np.isin(perm, np.asarray(reserve, np.int64))][:8192]
        self.n = n
        self.brows = [np.sort(perm[i * 64:(i + 1) * 64]) for i in range(64)]
        self.brows += [np.sort(perm[4096 + i * 8:4096 + (i + 1) * 8]) for i in range(512)]
        self.base = {64: list(range(64)), 8: list(range(64, 576))}
        self.made = {}
        self.arows = []
        self.rehits = []

    def _new(self, key, cols):
        if key not in self.made:
            self.made[key] = len(self.brows)
            self.brows.append(np.asarray(cols, np.int64))
        return self.made[key]

    def part(self, L, products, rehits, onecol=False):
        """B rows of length L giving `products` products with exactly `rehits` re-hits"""
        base = self.base[L]
        distinct = products - rehits
        assert distinct >= 1 and distinct <= L * len(base)
        nfull, rem = divmod(distinct, L)
        ent = base[:nfull]
        if rem:
            ent = ent + [self._new(("prefix", L, nfull, rem), self.brows[base[nfull]][:rem])]
        first = self.brows[ent[0]]
        full, rest = (0, rehits) if (onecol or nfull == 0) else divmod(rehits, L)
        ent = ent + [self._new(("copy", ent[0], k), first) for k in range(full)]
        cols = [int(first[0 if onecol else k % len(first)]) for k in range(rest)]
        ent = ent + [self._new(("single", c, k), [c]) for k, c in enumerate(cols)]
        return ent

    def row(self, *parts, rehits):
        ent = sorted(e for p in parts for e in p)
        assert len(set(ent)) == len(ent)
        self.arows.append(np.asarray(ent, np.int64))
        self.rehits.append(rehits)

    def add(self, L, products, rehits, **kw):
        self.row(self.part(L, products, rehits, **kw), rehits=rehits)

    def finish(self, seed, pad_rows=0, lo=1, hi=4):
        B = _csr(self.brows, self.n, seed, lo, hi)
        A = _csr(self.arows + [np.zeros(0, np.int64)] * pad_rows, len(self.brows), seed + 1, lo, hi)
        return A, B, np.asarray(self.rehits + [0] * pad_rows, np.int64)


def _mul(h, A, B):
    dA, dB = to_hs(A).toGpuCSR(), to_hs(B).toGpuCSR()
    dC = hs.gpuSpMMWrapper(dA, dB, h)
    got = dC.toCpuCSR()
    for d in (dC, dA, dB):
        d.deviceDispose()
    return got, h.midrow_paths()


_ORACLE = {}


def _plan(case, A, B, planted):
    """the oracle's product (computed once per case), the rows of bins 6-7, and the planted re-hits checked against it"""
    if case not in _ORACLE:
        want = po.sequential_spmm(A, B)
        f = _flops(A, B)
        mid = (f > 512) & (f <= 4096)
        assert np.array_equal((f - np.diff(np.asarray(want.rowPtr, np.int64)))[mid], planted[mid]), f"{case}: planted re-hits"
        _ORACLE[case] = (want, mid)
    return _ORACLE[case]


def run(case, A, B, planted, split=True, zero_signs=True, **env):
    """Case 7 for every input: on a fresh handle the first call has no log (0 direct rows), the second takes the planned
    split: rows with at most cap re-hits direct, the others the hash kernel.  split=False: the old path, 0 direct rows;
    split=None: not determined by the input.  Both calls equal the oracle.  Returns (second result, its paths, the handle)."""
    want, mid = _plan(case, A, B, planted)
    nmid = int(mid.sum())
    h = _handle(**env)
    try:
        got1, p1 = _mul(h, A, B)
        _same(got1, want, case + " (first call)", zero_signs)
        assert (p1["rows"], p1["direct"], p1["fallback"], p1["logged"]) == (nmid, 0, nmid, 0), f"{case}: first call {p1}"
        got2, p2 = _mul(h, A, B)
        _same(got2, want, case + " (second call)", zero_signs)
        assert p2["rows"] == nmid and p2["direct"] + p2["fallback"] == nmid, f"{case}: second call {p2}"
        if split is not None:
            takes = mid & (planted <= p2["cap"]) if split else np.zeros_like(mid)
            assert p2["direct"] == int(takes.sum()), f"{case}: second call {p2}"
            assert p2["logged"] == int(planted[takes].sum()), f"{case}: logged {p2}"     # case 12: products - nnz of the direct rows
    except BaseException:
        h.close()
        raise
    return got2, p2, h


def check(case, A, B, planted, **kw):
    run(case, A, B, planted, **kw)[2].close()


# ---- the inputs ---------------------------------------------------------------------------------------------------------
def case_walk_paths(n):
    """1: long entries only, flattened entries only (2 and 6 groups of 64 entries, two chunks of a 4-wave block), both"""
    b = Bld(n, 1)
    b.add(64, 600, 30)
    b.add(8, 600, 30)
    b.add(8, 3000, 100)
    b.row(b.part(64, 700, 20), b.part(8, 800, 25), rehits=45)
    b.row(b.part(64, 2000, 130), b.part(8, 1500, 7), rehits=137)
    return b.finish(2)


def case_edges(n):
    """2: the ends of the two bins and of the two layout slots of bin 6; no re-hit (expanded), one, a few dozen"""
    b = Bld(n, 3)
    for products in (513, 1024, 1025, 2048, 2049, 4096):
        for r in (0, 1, 40):
            b.add(64, products, r)
            b.add(8, products, r)
    return b.finish(4)


def case_table_sizes(n):
    """3: re-hits around the points where table_size<4> changes: 4 r against the smallest table, every power of two up to
    S, r >= S / 4, and the cap itself"""
    b = Bld(n, 5)
    for r in (T // 4 - 1, T // 4, T // 4 + 1, S // 8 - 1, S // 8, S // 8 + 1, S // 4 - 1, S // 4, S // 4 + 1, S // 8 * 7):
        b.add(64, 2000, r)
        b.add(8, 3000, r)
    return b.finish(6)


CASES = {"walk": case_walk_paths, "edges": case_edges, "tables": case_table_sizes}


@pytest.mark.parametrize("n", [N_LO, N_HI])
@pytest.mark.parametrize("name", sorted(CASES))
def test_direct_rows(name, n):
    """cases 1-3 (with 7, 11 and 12): every row has at most cap re-hits, none may fall back"""
    A, B, planted = CASES[name](n)
    assert planted.max() <= _cap()
    _, p, h = run(f"{name}-{n}", A, B, planted)
    h.close()
    assert p["fallback"] == 0, p


@pytest.mark.parametrize("name", sorted(CASES))
def test_old_path_switch(name):
    """case 10: SPGEMM_MIDDIRECT=0: the hash kernels for every row, on every call"""
    A, B, planted = CASES[name](N_HI)
    check(f"{name}-{N_HI}", A, B, planted, split=False, SPGEMM_MIDDIRECT=0)


def _cap_and_one_more(sizes, **env):
    """rows of `sizes` products with cap, cap - 1 (direct) and cap + 1, cap + 60 or so (hash kernel) re-hits"""
    cap = _cap(**env)
    b = Bld(N_HI, 7)
    for products in sizes:
        for r in (cap, cap + 1, cap - 1, min(cap + 60, products - 1)):
            b.add(64 if products != 2000 else 8, products, r)
    A, B, planted = b.finish(8)
    _, p, h = run(f"cap-{cap}-{sizes[0]}", A, B, planted, **env)
    h.close()
    assert (p["direct"], p["fallback"]) == (6, 6), p
    return cap


def test_rehits_at_the_cap_and_one_more():
    """case 4: exactly cap re-hits go direct, cap + 1 to the hash kernel, in both slots of bin 6 and in bin 7"""
    assert _cap_and_one_more((1000, 2000, 3000)) == S // 8 * 7


# SPGEMM_MD_CFG: waves x table slots of k_num_middirect in both bins (by default bin 6 runs 0 and bin 7 runs 1); with
# SPGEMM_MD_WAVE=0 the four-wave kernel sees the rows of bin 6 that the one-wave kernel takes otherwise
GEOMETRIES = {0: 1024, 1: 1024, 2: 2048, 3: 2048}


@pytest.mark.parametrize("cfg", sorted(GEOMETRIES))
def test_rehits_at_the_cap_and_one_more_in_every_geometry(cfg):
    """case 4 in every instantiation of the direct kernel; the cap is 7/8 of the table's slots (a row of 1000 products cannot
    have 1792 re-hits: the larger tables get rows of the second slot of bin 6 and of bin 7)"""
    slots = GEOMETRIES[cfg]
    sizes = (1000, 2000, 3000) if slots == 1024 else (2000, 3000, 4000)
    assert _cap_and_one_more(sizes, SPGEMM_MD_CFG=cfg, SPGEMM_MD_WAVE=0) == slots // 8 * 7


@pytest.mark.parametrize("cfg", sorted(GEOMETRIES))
def test_direct_rows_in_every_geometry(cfg):
    """case 1 in every instantiation of the direct kernel: none of its rows may fall back"""
    A, B, planted = CASES["walk"](N_HI)
    _, p, h = run(f"walk-{N_HI}", A, B, planted, SPGEMM_MD_CFG=cfg, SPGEMM_MD_WAVE=0)
    h.close()
    assert p["fallback"] == 0, p


def test_one_column_hit_many_times():
    """case 5: every A entry of a row reaches the same column (k - 1 copies of one key in the log: the insert's "key already
    there" exit); re-hits that all fall on one column of a long row; re-hits on two columns that share a slot of the
    smallest table"""
    slot = lambda c: ((c * 2654435761) & 0xffffffff) >> 24                 # T = 256 slots: the top 8 bits
    c1 = 1000
    c2 = next(c for c in range(c1 + 1, N_HI) if slot(c) == slot(c1))
    b = Bld(N_HI, 9, reserve=(c1, c2))
    for k in (513, 600, _cap() + 1):
        b.row([b._new(("same", k, i), [c1]) for i in range(k)], rehits=k - 1)
    b.add(64, 1500, 300, onecol=True)
    b.add(8, 700, 60, onecol=True)
    twins = [b._new(("twin", i), [c1 if i % 3 else c2]) for i in range(42)]
    b.row(b.part(64, 900, 0), twins, rehits=40)
    b.row(b.part(8, 2500, 5), twins, rehits=45)
    A, B, planted = b.finish(10)
    _, p, h = run("onecol", A, B, planted)
    h.close()
    assert p["fallback"] == 0, p


def test_signed_zeros_match_the_old_path():
    """case 6: products that cancel to 0.0 on a repeated column keep their entry; with +0.0 and -0.0 among the products the
    direct kernel's -0.0f accumulators give the bits of the hash kernels (the oracle is compared by value: its sums start
    from +0.0)"""
    b = Bld(N_HI, 11)
    b.add(64, 1200, 320)
    b.add(8, 2600, 200)
    b.add(64, 700, 0)
    A, B, planted = b.finish(12, lo=1, hi=1)
    rng = np.random.default_rng(13)
    B.values[:] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), size=len(B.values))
    new, p, h = run("zeros", A, B, planted, zero_signs=False)
    h.close()
    assert p["fallback"] == 0
    old, _, h = run("zeros", A, B, planted, split=False, zero_signs=False, SPGEMM_MIDDIRECT=0)
    h.close()
    z = new.values[new.values == 0]
    assert np.signbit(z).any() and (~np.signbit(z)).any()
    assert np.diff(np.asarray(new.rowPtr))[0] == 1200 - 320              # cancelled columns are entries all the same
    _same(new, old, "direct vs hash kernels")


def test_third_call_with_a_larger_product_regrows():
    """case 7: first call 0 direct, second the planned split (run()); then a larger product on the same handle -- more rows
    than the row-sized workspace holds, more re-hits than the log holds -- is exact whichever rows find room, and once the
    log has grown every row is direct again"""
    A, B, planted = case_walk_paths(N_HI)
    _, p2, h = run(f"walk-{N_HI}", A, B, planted)
    try:
        b = Bld(N_HI, 14)
        for i in range(150):
            b.add(64 if i % 2 else 8, 1500 + 13 * i, 100 + 5 * i)
        A3, B3, planted3 = b.finish(15, pad_rows=3000)
        want, mid = _plan("third", A3, B3, planted3)
        got3, p3 = _mul(h, A3, B3)
        _same(got3, want, "third call")
        assert p3["rows"] == 150 and p3["direct"] + p3["fallback"] == 150, p3
        got4, p4 = _mul(h, A3, B3)
        _same(got4, want, "fourth call")
        assert p4["capacity"] >= p3["reserved"] and (p4["direct"], p4["logged"]) == (150, int(planted3.sum())), (p3, p4)
    finally:
        h.close()


def test_small_bins_keep_the_hash_kernels_by_default():
    """below SPGEMM_MD_MINROWS (default: four rows per CU) rows in a bin, the bin stays with its hash kernel; the two bins
    decide separately"""
    A, B, planted = case_edges(N_HI)
    check(f"edges-{N_HI}", A, B, planted, split=False, SPGEMM_MD_MINROWS=100000)
    nb6 = int(((_flops(A, B) > 512) & (_flops(A, B) <= 2048)).sum())
    _, p, h = run(f"edges-{N_HI}", A, B, planted, split=None, SPGEMM_MD_MINROWS=nb6)
    h.close()
    assert 0 < nb6 < p["rows"] and (p["direct"], p["fallback"]) == (nb6, p["rows"] - nb6), p


def test_log_space_runs_out_mid_launch():
    """case 8: SPGEMM_MRLOG leaves the log two chunks of 4096 ints; 40 rows of 500 re-hits are dequeued four at a time, a
    chunk takes seven of them, so at most 14 rows go direct and the others fall back in the same launch"""
    b = Bld(N_HI, 16)
    for _ in range(40):
        b.add(64, 2000, 500)
    A, B, planted = b.finish(17)
    _, p, h = run("logfull", A, B, planted, split=None, SPGEMM_MRLOG=8192)
    h.close()
    assert p["capacity"] == 8192 and 1 <= p["direct"] <= 14 and p["direct"] + p["fallback"] == 40, p
    assert p["logged"] == 500 * p["direct"], p


def test_direct_and_fallback_rows_alternate_in_the_queue():
    """case 9: 301 rows of about 520 products (four per dequeue) and 151 of about 2100 (two per dequeue), neither a multiple of
    the batch; with the cap lowered to 100 every second row falls back"""
    b = Bld(N_HI, 18)
    for i in range(301):
        b.add(64 if i % 3 else 8, 520 + i % 7, 50 if i % 2 else 150)
    for i in range(151):
        b.add(64 if i % 3 else 8, 2100 + i % 5, 150 if i % 2 else 50)
    A, B, planted = b.finish(19)
    _, p, h = run("alternate", A, B, planted, SPGEMM_MD_CAP=100)
    h.close()
    assert p["cap"] == 100 and (p["direct"], p["fallback"]) == (150 + 76, 151 + 75), p


def test_bins_6_7_and_8_in_one_call():
    """case 11: rows of 513-2048, 2049-4096 and more than 4096 products, n above 262 144, SPGEMM_BD_MINROWS=1: both logging
    symbolic kernels and both direct kernels run in one call"""
    b = Bld(N_HI, 20)
    for i in range(6):
        b.add(64, 900 + 300 * i, 20 * i)                  # 900..2400
        b.add(8, 2500 + 300 * i, 31 * i)                  # 2500..4000
    for i in range(4):
        b.row(b.part(64, 4000, 64 * i), b.part(8, 1500, 10), rehits=64 * i + 10)       # 5500 products
    A, B, planted = b.finish(21)
    _, p, h = run("bins678", A, B, planted, SPGEMM_BD_MINROWS=1)
    try:
        big = h.bigrow_paths()
        assert (big["direct"], big["fallback"]) == (4, 0), big
        assert (p["rows"], p["fallback"]) == (12, 0), p
    finally:
        h.close()
