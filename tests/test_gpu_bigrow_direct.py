"""GPU (-m gpu): rows of more than 4096 products with more than 262 144 columns, where the symbolic pass logs the re-hit
columns and the direct kernel (k_num_bigdirect) hashes only those, against the multi-pass hash kernel it falls back to.

Every case is a handful of rows, n just above the rank kernel's 262 144 columns, values small integers (any summation
order is exact), compared with the CPU oracle after a per-row sort: rowPtr, columns and value BITS.  A handle sizes the
re-hit log at the end of its first call with big rows, so `twice()` runs every product two times on a fresh handle: the
first call takes the hash kernel for every row, the second the planned split (Handle.bigrow_paths() says which ran).
"""
import numpy as np
import pytest

from devcsr import bigrow_handle as _handle
from devcsr import bigrow_twice as twice
from devcsr import int_csr as _csr
from devcsr import row_flops as _flops
from devcsr import same_bits as _same
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu

N = 262208                      # BIG_WC + 64
L = 64                          # length of a B row


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()
    assert hs.device_count() >= 1, "GPU tests need a HIP device (no CPU fallback exists)"


def _disjoint_rows(count, n=N, seed=1):
    """`count` B rows of L columns each, no column in two rows, spread over [0, n)"""
    perm = np.random.default_rng(seed).permutation(n)[:count * L]
    return [np.sort(perm[i * L:(i + 1) * L]) for i in range(count)]


def _cap(**env):
    h = _handle(**env)
    try:
        return h.bigrow_paths()["cap"]
    finally:
        h.close()


# ---- the inputs ---------------------------------------------------------------------------------------------------------
def case_no_repeat():
    """1: 80 A entries times disjoint 64-long B rows: nothing is logged, every product is stored direct"""
    B = _csr(_disjoint_rows(80), N, 2)
    A = _csr([np.arange(80)], 80, 3)
    return A, B


def case_all_repeat(pairs=80):
    """2: the same row with every B row duplicated once: every product lands on a repeated column, no direct store
    (80 * 64 = 5120 re-hits; a direct kernel built with a smaller cap leaves this row to the hash kernel)"""
    rows = _disjoint_rows(80)[:pairs]
    B = _csr(rows + rows, N, 4)
    A = _csr([np.arange(2 * pairs)], 2 * pairs, 5)
    return A, B


def _pairs():
    """the longest all-repeat row of at most 80 pairs that the direct kernel takes"""
    return min(80, _cap() // L)


def case_all_repeat_direct():
    """2b: case 2 cut to the re-hit cap, so that the row with no direct store at all takes the direct kernel"""
    return case_all_repeat(_pairs())


def case_3_and_64():
    """3: one column hit 3 times, another 64 times; the extra hits come from one-column B rows (an add under a one-lane EXEC)"""
    rows = _disjoint_rows(80)
    c3, c64 = rows[7][11], rows[50][63]
    rows = rows + [np.array([c3])] * 2 + [np.array([c64])] * 63
    B = _csr(rows, N, 6)
    A = _csr([np.arange(len(rows))], len(rows), 7)
    return A, B


def case_copies(rehits):
    """copies of one B row plus one-column rows: exactly `rehits` re-hits on 64 distinct columns; 16 more B rows that
    share no column with anything keep the row above 4096 products whatever the cap"""
    pool = _disjoint_rows(17, seed=9)
    base = pool[0]
    full, rest = divmod(rehits, L)
    rows = [base] * (full + 1) + [base[:1]] * rest + pool[1:]
    B = _csr(rows, N, 10)
    A = _csr([np.arange(len(rows))], len(rows), 11)
    assert _flops(A, B)[0] == rehits + 17 * L > 4096
    return A, B


@pytest.mark.parametrize("make", [case_no_repeat, case_all_repeat, case_all_repeat_direct, case_3_and_64])
def test_logged_rows(make):
    """cases 1-3 (and 7): direct on the second call, but for an all-repeat row above the cap"""
    A, B = make()
    takes = 0 if make is case_all_repeat and 80 * L > _cap() else 1
    twice(A, B, make.__name__, direct=takes)


@pytest.mark.parametrize("make", [case_no_repeat, case_all_repeat, case_all_repeat_direct, case_3_and_64])
def test_old_path_switch(make):
    """case 10: cases 1-3 with SPGEMM_BIGDIRECT=0: the hash kernel for every row, on every call"""
    A, B = make()
    twice(A, B, make.__name__ + " old path", direct=0, SPGEMM_BIGDIRECT=0)


def test_few_big_rows_keep_the_hash_kernel_by_default():
    """below SPGEMM_BD_MINROWS (default: the CU count) rows of the last bin, the whole bin stays with the hash kernel"""
    A, B = case_all_repeat_direct()
    twice(A, B, "default threshold", direct=0, SPGEMM_BD_MINROWS=100000)


def _cap_and_one_more(**env):
    cap = _cap(**env)
    A, B = case_copies(cap)
    twice(A, B, "cap", direct=1, **env)
    A, B = case_copies(cap + 1)
    twice(A, B, "cap + 1", direct=0, **env)
    return cap


def test_rehits_at_the_cap_and_one_more():
    """case 4: exactly cap re-hits take the direct kernel, cap + 1 the hash kernel; the results are the oracle's either way"""
    _cap_and_one_more()


# SPGEMM_BD_CFG: waves x table slots of the direct kernel (1, 8 x 4096, is the default that every other test here runs)
GEOMETRIES = {0: 4096, 2: 8192, 3: 8192, 4: 4096}


@pytest.mark.parametrize("cfg", sorted(GEOMETRIES))
def test_rehits_at_the_cap_and_one_more_in_every_geometry(cfg):
    """case 4 in the other instantiations of the direct kernel; the cap is 7/8 of the table's slots"""
    assert _cap_and_one_more(SPGEMM_BD_CFG=cfg) == GEOMETRIES[cfg] // 8 * 7


@pytest.mark.parametrize("cfg", sorted(GEOMETRIES))
def test_logged_row_in_every_geometry(cfg):
    """case 3 in the other instantiations of the direct kernel"""
    A, B = case_3_and_64()
    twice(A, B, f"3 and 64, geometry {cfg}", direct=1, SPGEMM_BD_CFG=cfg)


def test_logged_and_fallback_rows_in_one_call():
    """case 5: rows of both kinds, interleaved in row order"""
    cap, r = _cap(), _pairs()
    assert r > 20
    rows = _disjoint_rows(80)
    heavy = [rows[3]] * (cap // L + 40)                   # re-hits well above the cap
    brows = rows + rows[:r] + heavy                       # B rows 0..79, copies of the first r from 80, the heavy copies behind
    nh, h0 = len(heavy), 80 + r
    B = _csr(brows, N, 12)
    A = _csr([np.concatenate([np.arange(r), 80 + np.arange(r)]),           # all repeat, 64 r re-hits: direct
              h0 + np.arange(nh),                                          # fallback
              np.arange(80),                                               # no repeat: direct
              h0 + np.arange(nh - 7),                                      # fallback
              np.concatenate([np.arange(20, 80), 80 + np.arange(r)])],     # 64 (r - 20) re-hits: direct
             len(brows), 13)
    assert (_flops(A, B) > 4096).all()
    twice(A, B, "mixed", direct=3)


def test_block_region_exhausted():
    """case 6: 600 rows of case 2 (cut to the cap: 64 r re-hits each) with a log region of one and a half such rows per block,
    fixed through SPGEMM_RLREGION and read back from the library: a block logs its first row and has no room for a second,
    and the symbolic kernel never runs more blocks than the device has CUs (at most 320 here), so rows fall back while
    others go direct.  The result is the oracle's."""
    r = _pairs()
    rows = _disjoint_rows(80)[:r]
    B = _csr(rows + rows, N, 14)
    A = _csr([np.arange(2 * r)] * 600, 2 * r, 15)
    region = L * r * 3 // 2
    _, p = twice(A, B, "region", direct=None, SPGEMM_RLREGION=region)
    assert p["region"] == region and L * r <= p["region"] < 2 * L * r
    assert p["direct"] + p["fallback"] == 600 and p["direct"] >= 1 and p["fallback"] >= 600 - 320, p


def test_two_symbolic_windows():
    """case 8: n = 2^20 + 64 is two symbolic windows; repeated columns on both sides of the edge"""
    n = (1 << 20) + 64
    rng = np.random.default_rng(16)
    low = _disjoint_rows(80, n=1 << 20, seed=17)
    rows = [np.concatenate([r[:56], (1 << 20) + np.sort(rng.choice(64, size=8, replace=False))]) for r in low]
    rows = rows + rows[:20] + [np.array([(1 << 20) - 1, 1 << 20])] * 5
    B = _csr(rows, n, 18)
    A = _csr([np.arange(len(rows))], len(rows), 19)
    twice(A, B, "two windows", direct=1)


def test_signed_zeros_match_the_old_path():
    """case 9: +0.0 and -0.0 on twice-hit (and once-hit) columns: the direct kernel's -0.0f accumulators give the bits of the
    hash kernel (the oracle is compared by value: its sums start from +0.0)"""
    rows = _disjoint_rows(80)
    B = _csr(rows + rows[:40], N, 20)
    rng = np.random.default_rng(21)
    B.values[:] = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], np.float32), size=len(B.values))
    A = _csr([np.arange(120)], 120, 22, lo=1, hi=1)
    new, _ = twice(A, B, "zeros", direct=1, zero_signs=False)
    old, _ = twice(A, B, "zeros old path", direct=0, zero_signs=False, SPGEMM_BIGDIRECT=0)
    assert np.signbit(new.values[new.values == 0]).any() and (~np.signbit(new.values[new.values == 0])).any()
    _same(new, old, "direct vs hash kernel")
