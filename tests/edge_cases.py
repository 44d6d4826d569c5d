"""Inputs that sit exactly on the edges of the row kernels, with an EXACT expected product (no GPU needed to build them).

A case is built from a list of row recipes.  Recipe = (F products, shape, regime[, D distinct columns | explicit columns]):

  shape   how the F products of the row are cut into B rows
            "one_long"   one A entry into one B row of length F
            "unit_rows"  F A entries into F B rows of length 1
            "rows16"     ceil(F/16) A entries into B rows of 16 (the last one shorter)
  regime  which columns the products hit (product p of the row -> column pool[idx(p)], pool = D distinct columns)
            "distinct"   idx = p mod D, D = min(F, n): every product on a column of its own while the width allows
            "one_col"    every product on ONE column
            "half"       idx = p mod D, D = min(ceil(F/2), n): the second half of the row repeats the first
            "cancel"     idx = (p div 2) mod D, D = min(ceil(F/2), n): products 2j and 2j+1 are +v and -v on one column, so
                         the entry sums to exactly 0 (and stays an entry of C); an odd F leaves one product alone
            "explicit"   product p on column cols[p] (the strided rows)

Every pool of more than one column starts with the seam columns below n (seam_columns: bitmap word, 64-word group, rank
window and symbolic window seams), rotated by the row number so that short rows cover all of them between them; the rest
is spread evenly over [0, n).  Every A row owns its B rows.

Exactness.  A's values are integers in +-{1,2,3}, B's in +-{1..4}: |a*b| <= MAX_ABS_PRODUCT = 12.  A row has at most
MAX_PRODUCTS = 400 000 products, so every partial sum of every entry of C, in any order, is an integer of magnitude
<= 12 * 400 000 = 4 800 000 < 2^24: exactly representable in float32 (and float64), hence every float addition on the way
is exact and the result does not depend on the order of the sums.  build() asserts the bound on the case it built (the sum
of |a*b| over the products of each entry), so the GPU tests may compare bit patterns.

The expectation is computed in int64 from the matrices themselves (not from the recipes): products expanded, keyed by
row*n + col, summed with np.unique / np.add.at; entries that sum to 0 are kept.
"""
from collections import namedtuple

import numpy as np

from helpers import po

# ---- the boundaries, restated from the comments of csrc/spgemm_device.hpp and csrc/spgemm_f64_device.hpp ---------------
NBINS = 9
BIN_UPPER = (0, 1, 4, 16, 64, 512, 2048, 4096)         # bin b < 8 holds rows of up to BIN_UPPER[b] products, bin 8 the rest
H1A_MAX, H4A_MAX = 256, 1024                           # bin 5 and bin 6 are two layout slots each, split here
NSUB = 6                                               # size classes of the last bin: 4097-8191, 8192-16383, ... (powers of two)
NSLOTS = 16
LONG_LEN = 64
BIG_WC = 262144                                        # n <= BIG_WC: rank kernel (+ saved bitmaps), above: LDS hash kernel
SYM_WC = 1 << 20                                       # columns per symbolic window
BIG_CAP = 16384                                        # ranks per pass of the rank kernel
BH_CAP = 11264                                         # distinct columns per pass of the hash kernel
BH_MAXCLS = 32                                         # hash classes with a parking region
BH_SPILL = 1 << 18                                     # parked products per block
BH_MARGIN = 125                                        # default parking margin, % (SPGEMM_BHMARGIN)
F64_LDS_MAXL, F64_PASS_L, F64_PASS_MAXL = 6144, 4096, 65536

MAX_PRODUCTS = 400000
MAX_ABS_PRODUCT = 12
assert MAX_PRODUCTS * MAX_ABS_PRODUCT < 2 ** 24

SHAPES = ("one_long", "unit_rows", "rows16")
REGIMES = ("distinct", "one_col", "half", "cancel")

BIN_EDGES = (0, 1, 2, 4, 5, 16, 17, 64, 65, 512, 513, 4096, 4097)
SLOT_EDGES = (256, 257, 1024, 1025, 2048, 2049)
CLASS_EDGES = (8191, 8192, 16383, 16384, 32767, 32768, 65535, 65536, 131071, 131072)
GRID_F = tuple(sorted(BIN_EDGES + SLOT_EDGES + CLASS_EDGES))
GRID_N = (9000, BIG_WC, BIG_WC + 1, SYM_WC, SYM_WC + 1)

STRIDES = (1, 2, 3, 64, 509, 4096, 5599, 11198, 65536, 65537)
STRIDED_W = (17000, 23000, 45000)


def bin_of(f):
    for b, hi in enumerate(BIN_UPPER):
        if f <= hi:
            return b
    return 8


def slot_of(f):
    """slots 0..4 = bins 0..4; 5, 6 = bin 5 split at H1A_MAX; 7, 8 = bin 6 split at H4A_MAX; 9 = bin 7; 10..15 = the size
    classes of bin 8, LARGEST first (class = floor(log2 f), everything from 2^17 on in the first)."""
    b = bin_of(f)
    if b < 5:
        return b
    if b == 5:
        return 5 if f <= H1A_MAX else 6
    if b == 6:
        return 7 if f <= H4A_MAX else 8
    if b == 7:
        return 9
    lg = min(int(f).bit_length() - 1, 12 + NSUB - 1)
    return 10 + (NSUB - 1 - (lg - 12))


def seam_columns(n):
    """columns on both sides of a bitmap word (31/32), a 64-bit half (63/64), the rank window (BIG_WC), the symbolic window
    (SYM_WC) and the ends of the matrix -- those that exist at width n"""
    s = [0, 31, 32, 63, 64, BIG_WC - 1, BIG_WC, SYM_WC - 1, SYM_WC, n - 1]
    return np.unique(np.array([c for c in s if 0 <= c < n], dtype=np.int64))


Recipe = namedtuple("Recipe", "F shape regime D cols", defaults=(None, None))
Case = namedtuple("Case", "name A B rowPtr colInd values intended recipes n")


def default_distinct(F, regime, n):
    if F == 0:
        return 0
    if regime == "distinct":
        return min(F, n)
    if regime == "one_col":
        return 1
    return min((F + 1) // 2, n)                       # half, cancel


def _pool(D, n, rowno):
    """D distinct columns of [0, n): the seams first (rotated by the row number), the rest spread evenly"""
    seams = seam_columns(n)
    seams = np.roll(seams, -((rowno // 4 + rowno % 4) % len(seams)))[:D]    # (rows come in runs of the 4 regimes)
    R = D - len(seams)
    if R == 0:
        return seams
    total = min(n, R + len(seam_columns(n)))
    cand = (np.arange(total, dtype=np.int64) * n) // total             # distinct: total <= n
    cand = np.setdiff1d(cand, seams, assume_unique=True)
    assert len(cand) >= R
    return np.concatenate([seams, cand[:R]])


def _b_row_lengths(F, shape):
    if shape == "one_long":
        return np.array([F], dtype=np.int64)
    if shape == "unit_rows":
        return np.ones(F, dtype=np.int64)
    assert shape == "rows16"
    return np.array([16] * (F // 16) + ([F % 16] if F % 16 else []), dtype=np.int64)


def expected_product(A, B):
    """exact C = A*B of integer-valued CSR matrices -> (rowPtr int32, colInd int32 ascending in every row, values int64,
    largest sum of |a*b| over the products of one entry, products per row)"""
    n = B.cols
    arp, brp = A.rowPtr.astype(np.int64), B.rowPtr.astype(np.int64)
    lens = brp[A.colInd.astype(np.int64) + 1] - brp[A.colInd]
    total = int(lens.sum())
    first = np.cumsum(lens) - lens
    jb = np.repeat(brp[A.colInd] - first, lens) + np.arange(total, dtype=np.int64)
    row_of_entry = np.repeat(np.arange(A.rows, dtype=np.int64), np.diff(arp))
    rows = np.repeat(row_of_entry, lens)
    va, vb = np.rint(A.values).astype(np.int64), np.rint(B.values).astype(np.int64)
    assert np.array_equal(va, A.values) and np.array_equal(vb, B.values), "integer values only"
    prod = np.repeat(va, lens) * vb[jb]
    key, inv = np.unique(rows * n + B.colInd.astype(np.int64)[jb], return_inverse=True)
    vals = np.zeros(len(key), dtype=np.int64)
    np.add.at(vals, inv, prod)
    mag = np.zeros(len(key), dtype=np.int64)
    np.add.at(mag, inv, np.abs(prod))
    rowPtr = np.zeros(A.rows + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n, minlength=A.rows), out=rowPtr[1:])
    flops = np.bincount(rows, minlength=A.rows)
    return rowPtr.astype(np.int32), (key % n).astype(np.int32), vals, int(mag.max()) if len(mag) else 0, flops


def build(name, n, recipes, seed=0):
    """-> Case: A (rows = recipes), B (n columns), the exact product, and per row the INTENDED (flops, distinct columns)"""
    rng = np.random.default_rng(seed)
    a_lens, a_cols, a_vals, b_lens, b_cols, b_vals, intended = [], [], [], [], [], [], []
    k = 0
    for rowno, rc in enumerate(recipes):
        F = int(rc.F)
        assert 0 <= F <= MAX_PRODUCTS and rc.shape in SHAPES
        lens = _b_row_lengths(F, rc.shape)
        nb = len(lens)
        a = rng.choice(np.array([-3, -2, -1, 1, 2, 3]), size=nb)
        b = rng.choice(np.array([-4, -3, -2, -1, 1, 2, 3, 4]), size=F)
        p = np.arange(F, dtype=np.int64)
        if rc.regime == "explicit":
            pool = np.asarray(rc.cols, dtype=np.int64)
            assert len(pool) == F and len(np.unique(pool)) == F and (F == 0 or (pool.min() >= 0 and pool.max() < n))
            D, idx = F, p
        else:
            assert rc.regime in REGIMES
            D = default_distinct(F, rc.regime, n) if rc.D is None else int(rc.D)
            assert D <= n and D <= F and (D > 0) == (F > 0)
            pool = rng.permutation(_pool(D, n, rowno))
            if rc.regime == "cancel":
                idx = (p // 2) % max(D, 1)
                b[1::2] = -b[0:F - 1:2]                        # the pair shares its A entry except in "unit_rows":
                if rc.shape == "unit_rows":
                    a[1::2] = a[0:F - 1:2]
            elif rc.regime == "one_col":
                idx = np.zeros(F, dtype=np.int64)
            else:
                idx = p % max(D, 1)
        a_lens.append(nb)
        a_cols.append(k + np.arange(nb, dtype=np.int64))
        a_vals.append(a)
        b_lens.append(lens)
        b_cols.append(pool[idx] if F else np.zeros(0, dtype=np.int64))
        b_vals.append(b)
        intended.append((F, D))
        k += nb
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    arp = np.concatenate([[0], np.cumsum(a_lens)])
    brp = np.concatenate([[0], np.cumsum(cat(b_lens, np.int64))])
    A = po.CSRHost(arp, cat(a_cols, np.int32), cat(a_vals, np.float32), len(recipes), max(k, 1))
    if k == 0:
        brp = np.array([0, 0])
    B = po.CSRHost(brp, cat(b_cols, np.int32), cat(b_vals, np.float32), max(k, 1), n)
    rowPtr, colInd, vals, mag, flops = expected_product(A, B)
    assert flops.max(initial=0) <= MAX_PRODUCTS and mag * 1 < 2 ** 24, "the exactness bound of this module does not hold"
    assert np.abs(A.values).max(initial=0) <= 3 and np.abs(B.values).max(initial=0) <= 4
    return Case(name, A, B, rowPtr, colInd, vals, np.array(intended, dtype=np.int64).reshape(-1, 2), list(recipes), n)


def expected_stats(case):
    """what spgemm_stats must say after the product: total_flops, nnzC, bin_rows"""
    F = case.intended[:, 0]
    bins = np.bincount([bin_of(int(f)) for f in F], minlength=NBINS)
    return {"total_flops": int(F.sum()), "nnzC": int(case.intended[:, 1].sum()), "bin_rows": [int(x) for x in bins]}


# ---- the cases ---------------------------------------------------------------------------------------------------------
def grid_recipes():
    """every edge F x every shape x every regime (348 rows, 6.3 M products)"""
    return [Recipe(F, sh, rg) for F in GRID_F for sh in SHAPES for rg in REGIMES]


def edge_grid(n):
    return build(f"edge grid n={n}", n, grid_recipes(), seed=n % 1000)


def _rows_with_distinct(ds):
    return [Recipe(D, SHAPES[i % 3], "distinct") for i, D in enumerate(ds)]


CAP_RANK_N = BIG_WC
CAP_HASH_N = 2500000
# rank kernel: BIG_CAP ranks per pass (1 | 2 passes, 2 | 3 passes); the f64 table and pass edges ride along
CAP_RANK_D = (BIG_CAP, BIG_CAP + 1, 2 * BIG_CAP, 2 * BIG_CAP + 1, F64_LDS_MAXL, F64_LDS_MAXL + 1, 2 * F64_PASS_L,
              2 * F64_PASS_L + 1, F64_PASS_MAXL, F64_PASS_MAXL + 1)
# hash kernel: BH_CAP columns per pass (1 | 2 | 3 passes), more classes than parking regions; f64: one pass | multi-pass,
# 2 | 3 passes, LDS | device-memory table
CAP_HASH_D = (BH_CAP, BH_CAP + 1, 2 * BH_CAP, 2 * BH_CAP + 1, BH_MAXCLS * BH_CAP + 1, F64_LDS_MAXL, F64_LDS_MAXL + 1,
              2 * F64_PASS_L, 2 * F64_PASS_L + 1, F64_PASS_MAXL, F64_PASS_MAXL + 1)
# a 3-pass row (25 000 columns) that would park 2 * (330 000 * 1.25 / 3 + 256) = 275 512 products > BH_SPILL: walks per pass
SPILL_ROW = Recipe(330000, "rows16", "distinct", 25000)


def capacity_rank_case():
    return build("capacity rows, rank kernel", CAP_RANK_N, _rows_with_distinct(CAP_RANK_D), seed=3)


def capacity_hash_case():
    return build("capacity rows, hash kernel", CAP_HASH_N, _rows_with_distinct(CAP_HASH_D) + [SPILL_ROW], seed=4)


def strided_patterns():
    """(stride, row length) of every strided row whose last column stays below 2^31"""
    pats = [(s, W) for s in STRIDES for W in STRIDED_W] + [(509, 300000)]
    return [(s, W) for s, W in pats if W * s < 2 ** 31]


def strided_case(s, W):
    """one row with the columns i*s, i < W, in a matrix of W*s columns"""
    return build(f"strided s={s} W={W}", W * s, [Recipe(W, "rows16", "explicit", None, np.arange(W, dtype=np.int64) * s)],
                 seed=s % 997 + W)
