"""GPU (-m gpu): rows of 513-2048 products (bin 6) whose re-hits the symbolic pass logged, in the wave-per-row direct kernel
(k_num_midwave: one wave and a 512-slot table per row, at most 448 re-hits) beside the four-wave kernel (k_num_middirect,
the rows of 449-896 re-hits) and the hash kernel of the bin (everything else).

B is built from disjoint rows, so the re-hits of every row of A are planted exactly: a copy of a B row the row already uses
adds as many re-hits as it has columns, a one-column B row adds one.  The planted count is checked on the CPU (products minus
the oracle's row length) before anything is asserted about it.  A handle has no log on its first call, so every case
multiplies three times on a fresh handle and judges the second and the third call: against the CPU oracle (rowPtr and
per-row sorted columns exact, values within 1e-6 relative; a kernel error flag fails the call itself), and the rows each
kernel took (Handle.midrow_paths(): "wave", "multiwave", "fallback") against the plan.  SPGEMM_MD_MINROWS=1 and
SPGEMM_MW_MINROWS=1: the cases are a few hundred rows, far below the sizes at which a bin takes the direct kernels by default.
"""
import os

import numpy as np
import pytest

from devcsr import to_hs
from helpers import assert_parity, canonical_arrays, po
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu

N = 200000                      # columns of B (below the 262 144 of the big rows' rank kernel)
WCAP = 448                      # re-hits the wave kernel takes: 7/8 of its 512 slots
CAP = 896                       # ... and the four-wave kernel: 7/8 of 1024


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()
    assert hs.device_count() >= 1, "GPU tests need a HIP device (no CPU fallback exists)"


def _handle(**env):
    """a fresh handle; the SPGEMM_* knobs are read when it is created"""
    env.setdefault("SPGEMM_MD_MINROWS", 1)
    env.setdefault("SPGEMM_MW_MINROWS", 1)
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return hs.Handle(0)
    finally:
        for k in env:
            del os.environ[k]


class Bld:
    """B rows over n columns, all disjoint: 64 rows of 64 columns (one round of the walk each), 512 rows of 8, and long rows
    of 70, 600, 1500 and 2048 columns; on demand prefixes, copies and one-column rows of them.  A row of A is the sorted
    list of the B rows it uses; rows of A share B rows freely, only repeats inside one row plant re-hits."""
    LONG = (70, 600, 1500, 2048)

    def __init__(self, n, seed, reserve=()):
        rng = np.random.default_rng(seed)
        perm = rng.permutation(n)
        perm = perm[~np.isin(perm, np.asarray(reserve, np.int64))]
        self.n = n
        self.brows = [np.sort(perm[i * 64:(i + 1) * 64]) for i in range(64)]
        self.brows += [np.sort(perm[4096 + i * 8:4096 + (i + 1) * 8]) for i in range(512)]
        self.base = {64: list(range(64)), 8: list(range(64, 576))}
        at = 8192
        self.long = {}
        for L in self.LONG:
            self.long[L] = len(self.brows)
            self.brows.append(np.sort(perm[at:at + L]))
            at += L
        self.made = {}
        self.arows = []
        self.rehits = []

    def _new(self, key, cols):
        if key not in self.made:
            self.made[key] = len(self.brows)
            self.brows.append(np.asarray(cols, np.int64))
        return self.made[key]

    def copy(self, e, k=0):
        return self._new(("copy", e, k), self.brows[e])

    def singles(self, cols):
        """one-column B rows, one per entry of cols (a column may come several times)"""
        return [self._new(("single", int(c), k), [int(c)]) for k, c in enumerate(cols)]

    def part(self, L, products, rehits, onecol=False, spread=False):
        """B rows of length L giving `products` products with exactly `rehits` re-hits: copies of the first entry and
        one-column rows on its columns; onecol: all on its first column; spread: the copies go round all the full entries,
        so that no column is hit much more often than re-hits / distinct columns"""
        base = self.base[L]
        distinct = products - rehits
        assert distinct >= 1 and distinct <= L * len(base)
        nfull, rem = divmod(distinct, L)
        ent = base[:nfull]
        if rem:
            ent = ent + [self._new(("prefix", L, nfull, rem), self.brows[base[nfull]][:rem])]
        first = self.brows[ent[0]]
        full, rest = (0, rehits) if (onecol or nfull == 0) else divmod(rehits, L)
        src = ent[:nfull] if spread else ent[:1]
        ent = ent + [self.copy(src[k % len(src)], k // len(src)) for k in range(full)]
        ent = ent + self.singles([first[0 if onecol else k % len(first)] for k in range(rest)])
        return ent

    def row(self, *parts, rehits):
        ent = sorted(e for p in parts for e in p)
        assert len(set(ent)) == len(ent)
        self.arows.append(np.asarray(ent, np.int64))
        self.rehits.append(rehits)

    def add(self, L, products, rehits, **kw):
        self.row(self.part(L, products, rehits, **kw), rehits=rehits)

    def finish(self, seed, lo=1, hi=4, real=False):
        B = _csr(self.brows, self.n, seed, lo, hi, real)
        A = _csr(self.arows, len(self.brows), seed + 1, lo, hi, real)
        return A, B, np.asarray(self.rehits, np.int64)


def _csr(rows, ncols, seed, lo=1, hi=4, real=False):
    """values: small integers (any summation order is exact), or real=True: floats in [0.25, 1.25)"""
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    v = (rng.random(len(ci)) + 0.25 if real else rng.integers(lo, hi + 1, size=len(ci))).astype(np.float32)
    return po.CSRHost(rp, ci, v, len(rows), ncols)


def _flops(A, B):
    blen = np.diff(np.asarray(B.rowPtr, np.int64))
    per = blen[np.asarray(A.colInd)]
    rp = np.asarray(A.rowPtr, np.int64)
    return np.array([per[rp[i]:rp[i + 1]].sum() for i in range(A.rows)])


def _mul(h, A, B):
    dA, dB = to_hs(A).toGpuCSR(), to_hs(B).toGpuCSR()
    dC = hs.gpuSpMMWrapper(dA, dB, h)
    got = dC.toCpuCSR()
    for d in (dC, dA, dB):
        d.deviceDispose()
    return got, h.midrow_paths()


_ORACLE = {}


def _plan(case, A, B, planted):
    """the oracle's product (computed once per case and left alone), the products of every row, and the planted re-hits
    checked against the two"""
    if case not in _ORACLE:
        want = po.omp_spmm(A, B)
        f = _flops(A, B)
        mid = (f > 512) & (f <= 4096)
        assert np.array_equal((f - np.diff(np.asarray(want.rowPtr, np.int64)))[mid], planted[mid]), f"{case}: planted re-hits"
        _ORACLE[case] = (want, f)
    return _ORACLE[case]


def _split(f, planted, wcap=WCAP, cap=CAP):
    """rows per kernel when every row finds log space: wave, four-wave, fallback (of bins 6 and 7)"""
    b6, b7 = (f > 512) & (f <= 2048), (f > 2048) & (f <= 4096)
    wave = b6 & (planted <= wcap)
    multi = b6 & ~wave & (planted <= cap)
    return int(wave.sum()), int(multi.sum()), int((b6 & ~wave & ~multi).sum() + (b7 & (planted > cap)).sum())


def run(case, A, B, planted, split=True, **env):
    """three products on a fresh handle: the first has no log and keeps the hash kernels for every row; the second and the
    third are judged -- parity with the oracle, and (split=True) the planned rows per kernel.  Returns (third result, its
    paths)."""
    want, f = _plan(case, A, B, planted)
    nmid = int(((f > 512) & (f <= 4096)).sum())
    h = _handle(**env)
    try:
        got, p = _mul(h, A, B)
        assert_parity(got, want, what=case + " (first call)")
        assert (p["rows"], p["direct"], p["wave"], p["multiwave"]) == (nmid, 0, 0, 0), f"{case}: first call {p}"
        for call in ("second", "third"):
            got, p = _mul(h, A, B)
            assert_parity(got, want, what=f"{case} ({call} call)")
            assert p["rows"] == nmid and p["direct"] + p["fallback"] == nmid, f"{case}: {call} call {p}"
            if split:
                assert (p["wave"], p["multiwave"], p["fallback"]) == _split(f, planted), f"{case}: {call} call {p}"
        return got, p
    finally:
        h.close()


# ---- the inputs ---------------------------------------------------------------------------------------------------------
def test_product_counts():
    """the ends of bin 6 and of its two layout slots: 513, 1024, 1025 and 2048 products; expanded, one re-hit, a few dozen;
    long entries (64 products each) and flattened ones (8 each: up to 256 A entries, four groups)"""
    b = Bld(N, 1)
    for products in (513, 1024, 1025, 2048):
        for r in (0, 1, 40):
            b.add(64, products, r)
            b.add(8, products, r)
    A, B, planted = b.finish(2)
    _, p = run("products", A, B, planted)
    assert (p["wave"], p["multiwave"], p["fallback"]) == (24, 0, 0), p


def test_round_counts():
    """groups of 8, 9, 16, 17 and 32 rounds of 64 products (a trip gathers up to 8 rounds), and of 13 and 15 rounds, whose last
    trips of 5 and 7 rounds run as 6 and 8; every shape expanded and with a table"""
    b = Bld(N, 3)
    for rounds in (9, 13, 15, 16, 17, 32):              # one group: `rounds` B rows of 64 columns, exactly one round each
        b.row(b.base[64][:rounds], rehits=0)
        if rounds < 32:
            b.row(b.base[64][:rounds], b.singles(b.brows[0][:20]), rehits=20)
        else:
            b.row(b.base[64][:rounds - 1], b.singles(b.brows[0][:64]), rehits=64)      # 31 * 64 + 64 products
    # two groups of 64 entries x 8 products: 8 rounds each; then a third group of 20 one-column rows (their ids come last)
    b.row(b.base[8][:128], rehits=0)
    b.row(b.base[8][:128], b.singles(b.brows[64][:8].tolist() + b.brows[65][:8].tolist() + b.brows[100][:4].tolist()), rehits=20)
    # 5 and 7 rounds alone in a second group (64 entries x 8, then the tail)
    b.row(b.base[8][:64 + 40], rehits=0)                # 8 rounds + 5
    b.row(b.base[8][:64 + 55], b.singles(b.brows[64][:3]), rehits=3)                   # 8 rounds + 7 (443 products)
    A, B, planted = b.finish(4)
    f = _flops(A, B)
    assert f.min() > 512 and f.max() <= 2048
    _, p = run("rounds", A, B, planted)
    assert (p["wave"], p["fallback"]) == (A.rows, 0), p


def test_a_entries_per_row():
    """1, 64, 65 and more than 192 A entries (the groups of 64 entries the walk stages), with B rows of 70 (longer than 63),
    600 and 1500 (longer than 512) and 2048 columns among them"""
    b = Bld(N, 5)
    for L in (600, 1500, 2048):
        b.row([b.long[L]], rehits=0)                                                   # one A entry
    b.row([b.long[600]], b.singles(b.brows[b.long[600]][:30]), rehits=30)              # a long row first, then 30 re-hits of it
    b.row([b.long[70]], b.base[8][:63], rehits=0)                                      # 64 entries, 574 products
    b.row([b.long[70]], b.base[8][:62], [b.copy(b.base[8][0])], rehits=8)              # 64 entries, one a copy
    b.row([b.long[70]], b.base[8][:64], rehits=0)                                      # 65 entries
    b.row([b.long[70], b.copy(b.long[70])], b.base[8][:63], rehits=70)                 # 65 entries, the long one twice
    b.row([b.long[600]], b.base[8][:100], b.singles(b.brows[b.long[600]][100:200]), rehits=100)   # 201 entries
    b.row(b.base[8][:200], rehits=0)                                                   # 200 entries, 1600 products
    b.row(b.base[8][:193], b.singles(b.brows[64 + 192][:7]), [b.long[70]], rehits=7)   # 201 entries
    b.row(b.base[64][:2], [b.long[1500]], b.base[8][:40], [b.copy(b.base[64][1])], rehits=64)     # 2012 products
    A, B, planted = b.finish(6)
    f = _flops(A, B)
    assert f.min() > 512 and f.max() <= 2048
    _, p = run("entries", A, B, planted)
    assert (p["wave"], p["fallback"]) == (A.rows, 0), p


REHITS = (0, 1, 16, 17, 128, 129, 448, 449, 896, 900)


def test_rehits_per_row():
    """0 re-hits (expanded); 1; 16 and 17, 128 and 129 (table_size<4> steps 64 -> 128 slots, and reaches the 512 slots); 448
    re-hits take the wave kernel, 449 and 896 the four-wave kernel, 900 the hash kernel.  Copies of long entries and one-column
    rows, in both layout slots"""
    b = Bld(N, 7)
    for r in REHITS:
        b.add(64, 2000, r)
        b.add(8, 2040, r, onecol=r % 2 == 1)
        if r < 1000:
            b.add(64, 1000 + (r > 400) * 24, r)
    A, B, planted = b.finish(8)
    _, p = run("rehits", A, B, planted)
    nw = sum(3 for r in REHITS if r <= WCAP)
    assert (p["wave"], p["multiwave"], p["fallback"]) == (nw, 6, 3), p


def test_one_column_hit_many_times():
    """every A entry of a row reaches the same column (k - 1 copies of one key in the log: the insert's "key already there"
    exit); re-hits that all fall on one column of a long row; re-hits on two columns that share a slot of the smallest table"""
    slot = lambda c: ((c * 2654435761) & 0xffffffff) >> 26                 # 64 slots: the top 6 bits
    c1 = 1000
    c2 = next(c for c in range(c1 + 1, N) if slot(c) == slot(c1))
    b = Bld(N, 9, reserve=(c1, c2))
    for k in (513, 600):                                 # 512 and 599 re-hits: the four-wave kernel
        b.row([b._new(("same", k, i), [c1]) for i in range(k)], rehits=k - 1)
    b.row(b.base[64][:8], [b._new(("same", 449, i), [c1]) for i in range(449)], rehits=448)    # 448 on one column: the wave kernel
    b.add(64, 1500, 300, onecol=True)
    b.add(8, 700, 60, onecol=True)
    twins = [b._new(("twin", i), [c1 if i % 3 else c2]) for i in range(12)]
    b.row(b.part(64, 900, 0), twins, rehits=10)          # 10 re-hits: a 64-slot table, two keys on one slot
    b.row(b.part(8, 1500, 5), twins, rehits=15)
    A, B, planted = b.finish(10)
    _, p = run("onecol", A, B, planted)
    assert (p["wave"], p["multiwave"], p["fallback"]) == (5, 2, 0), p


def _bits(M):
    c, v = canonical_arrays(M.rowPtr, M.colInd, M.values)
    return np.asarray(M.rowPtr, np.int32).tobytes(), c.tobytes(), v.view(np.uint32).tobytes()


def test_signed_zeros_match_the_four_wave_kernel():
    """products of -0.0f and pairs that cancel to +0.0f on a repeated column: the bits of SPGEMM_MD_WAVE=0, whose rows all
    take the four-wave kernel (both start a repeated column from -0.0f; the oracle, which starts from +0.0, is compared by
    value)"""
    b = Bld(N, 11)
    b.add(64, 1200, 320)
    b.add(8, 1600, 200)
    b.add(64, 700, 0)
    b.add(8, 2048, 448, onecol=True)
    A, B, planted = b.finish(12, lo=1, hi=1)
    rng = np.random.default_rng(13)
    B.values[:] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), size=len(B.values))
    new, p = run("zeros", A, B, planted)
    assert (p["wave"], p["multiwave"]) == (4, 0), p
    old, q = run("zeros", A, B, planted, split=False, SPGEMM_MD_WAVE=0)
    assert (q["wave"], q["multiwave"]) == (0, 4), q
    z = new.values[new.values == 0]
    assert np.signbit(z).any() and (~np.signbit(z)).any()
    assert np.diff(np.asarray(new.rowPtr))[0] == 1200 - 320              # cancelled columns are entries all the same
    assert _bits(new) == _bits(old)


def _mixed(hubs=True):
    """wave (expanded, a few dozen re-hits, 440-448), four-wave and fallback rows alternating in queue order in both layout
    slots of bin 6 (a row of 1000-1023 products with 897-916 re-hits keeps 84 or more distinct columns), with rows of bins 5,
    7 and 8 between them.  hubs: every seventh row has all its re-hits on ONE column (up to 916 products summed into an
    entry); hubs=False spreads the re-hits of every row over its columns instead (at most 16 products per entry)"""
    b = Bld(N, 14)
    for i in range(240):
        slot_b = i % 2
        r = ((0, 30 + i % 50, 440 + i % 9)[i // 6 % 3], 449 + i % 40, 897 + i % 20)[i // 2 % 3]
        b.add(64 if i % 5 else 8, (1000 if not slot_b else 2000) + i % 24, r, onecol=hubs and i % 7 == 0, spread=not hubs)
        if i % 6 == 0:
            b.add(8, 300 + i, 10)                        # bin 5
        if i % 8 == 0:
            b.add(64, 3000 + i, 100 + i)                 # bin 7
        if i % 60 == 0:
            b.row(b.part(64, 4000, 64), b.part(8, 1500, 10), rehits=74)      # bin 8: 5500 products
    return b.finish(15)


def _kinds_alternate(f, planted):
    """every layout slot of bin 6 holds the three kinds of row, and in row order no four neighbours in it are of one kind"""
    for lo, hi in ((512, 1024), (1024, 2048)):
        r = planted[(f > lo) & (f <= hi)]
        kind = (r > WCAP).astype(int) + (r > CAP)
        assert min(np.bincount(kind, minlength=3)) >= 20, (lo, np.bincount(kind, minlength=3))
        assert all(len(set(kind[j:j + 4])) > 1 for j in range(len(kind) - 3)), lo


def test_mixed_queue_all_bins():
    A, B, planted = _mixed()
    f = _flops(A, B)
    for lo, hi in ((64, 512), (512, 1024), (1024, 2048), (2048, 4096), (4096, 1 << 30)):
        assert ((f > lo) & (f <= hi)).any(), (lo, hi)
    _kinds_alternate(f, planted)
    w, m, fb = _split(f, planted)
    assert min(w, m, fb) >= 40, (w, m, fb)
    run("mixed", A, B, planted)


def test_log_space_runs_out_mid_launch():
    """SPGEMM_MRLOG leaves the log two chunks of 4096 ints: 60 rows of 300 re-hits reserve more than that, so some rows find
    room and take the wave kernel and the others fall back in the same launch; the product does not change"""
    b = Bld(N, 16)
    for i in range(60):
        b.add(64 if i % 2 else 8, 1800 + i, 300)
    A, B, planted = b.finish(17)
    _, p = run("logfull", A, B, planted, split=False, SPGEMM_MRLOG=8192)
    assert p["capacity"] == 8192 and p["multiwave"] == 0, p
    assert 1 <= p["wave"] <= 26 and p["wave"] + p["fallback"] == 60 and p["logged"] == 300 * p["wave"], p


def test_knob_equality():
    """SPGEMM_MD_WAVE=0 against 1 on the mixed input.  With real values: the same structure; the values of columns hit once
    (stored straight from the walk by both kernels) bit for bit, the sums within 1e-6 relative.  The LDS adds of a sum land
    in another order on every launch, and two float32 sums of N positive terms in different orders differ by about
    sqrt(N) * 2^-24 relative (helpers.assert_parity: past 1e-6 at N ~ 500 in ANY implementation), so the real-valued input
    spreads its re-hits: no entry sums more than 16 products (checked), at which two orders differ by 2.4e-7 typically and
    by 2 * 15 * 2^-24 = 1.8e-6 only if every rounding of both sums fell the same way.  The hub columns (up to 916 products
    in one entry) are compared on the integer-valued input, whose sums are exact in any order: bit for bit."""
    A0, B0, planted = _mixed(hubs=False)
    A, B, _ = _mixed(hubs=False)
    rng = np.random.default_rng(18)
    A.values[:] = (rng.random(len(A.values)) + 0.25).astype(np.float32)
    B.values[:] = (rng.random(len(B.values)) + 0.25).astype(np.float32)
    f = _flops(A, B)
    _kinds_alternate(f, planted)
    ones = lambda M: po.CSRHost(M.rowPtr, M.colInd, np.ones_like(M.values), M.rows, M.cols)
    cnt = po.sequential_spmm(ones(A0), ones(B0))
    cc, cn = canonical_arrays(cnt.rowPtr, cnt.colInd, cnt.values)
    once = cn == 1
    assert once.any() and (~once).any() and cn.max() <= 16, cn.max()
    new, p = run("mixed-real", A, B, planted)
    old, q = run("mixed-real", A, B, planted, split=False, SPGEMM_MD_WAVE=0)
    w, m, fb = _split(f, planted)
    assert (q["wave"], q["multiwave"], q["fallback"]) == (0, w + m, fb), q
    assert np.array_equal(new.rowPtr, old.rowPtr)
    nc, nv = canonical_arrays(new.rowPtr, new.colInd, new.values)
    oc, ov = canonical_arrays(old.rowPtr, old.colInd, old.values)
    assert np.array_equal(nc, oc) and np.array_equal(cc, nc)
    assert nv[once].tobytes() == ov[once].tobytes()
    assert np.all(np.abs(nv.astype(np.float64) - ov) <= 1e-6 * np.maximum(np.abs(nv), np.abs(ov)))
    Ah, Bh, ph = _mixed()                                # the hubs, integer values (the input of test_mixed_queue_all_bins)
    newh, _ = run("mixed", Ah, Bh, ph)
    oldh, qh = run("mixed", Ah, Bh, ph, split=False, SPGEMM_MD_WAVE=0)
    assert (qh["wave"], qh["multiwave"], qh["fallback"]) == (0, w + m, fb), qh
    assert _bits(newh) == _bits(oldh)
