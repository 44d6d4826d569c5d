"""Inputs and the reference for products whose B has up to 2^31 - 1 columns (no GPU import).

The C oracle holds dense arrays of n entries per call, about 19 GB at n = 2^31, so it cannot be the reference there.  A
product depends on B's columns only through equality and order: for a strictly increasing map phi: [0, n0) -> [0, n)

    A * relabel(B, phi, n) == relabel(A * B, phi, n)

exactly in structure, and bit for bit in values when every sum is exact.  Every case is therefore built over N0 compact
columns, multiplied there by the oracle, and relabelled; tests/test_wide_columns_ref.py checks the identity itself at
N_REF columns, which the oracle can still hold, for every case and every map.

Maps (n0 compact columns, width n):
  top     phi(j) = n - n0 + j: everything in the last symbolic window, at its top
  spread  phi(j) = j * ((n - 1) // (n0 - 1)), the last column on n - 1: column 0 and n - 1 present, every window hit
  edges   chosen compact columns (edge_positions) land, in order, on w * 2^20 - 1 and w * 2^20 for w in EDGE_WINDOWS where
          these are below n, and on n - 1; the other columns are spaced evenly between them

Values: float cases hold the integers 1..4; double cases hold k * 2^-30 with odd k < 2^12.  Every product and every sum
of a case is exact in its type, whatever the order of summation.

A case is a handful of rows of A over B rows of at most L = 64 columns; `claims` says, per row of A, how many products
and how many distinct columns it was built to have (the reference test counts both).
"""
import numpy as np

from f64ref import Host64, spgemm_f64
from helpers import po

L = 64                                   # longest B row
N0 = 200000                              # compact columns
WC = 1 << 20                             # columns per window of the big rows' symbolic pass
W = ((1 << 30) + 1,                      # bit 30 set
     (1 << 31) - WC,                     # the last width whose windows end below 2^31
     (1 << 31) - WC + 1,                 # the first whose last window does not
     (1 << 31) - 1)                      # the widest an int holds: columns up to 2^31 - 2
N_REF = 3 * WC + 5                       # three windows and a bit: the oracle's dense arrays still fit
MAPS = ("top", "spread", "edges")
EDGE_WINDOWS = (1, 2, 1024, 2047)
BIN_LAST = (0, 1, 4, 16, 64, 512, 2048, 4096)      # the last product count of bins 0..7; bin 8 is everything above


# ---- the maps ------------------------------------------------------------------------------------------------------------
def edge_columns(n):
    """the window-edge columns below n, and n - 1, ascending"""
    e = {n - 1}
    for w in EDGE_WINDOWS:
        e.update(c for c in (w * WC - 1, w * WC) if c < n)
    return np.array(sorted(e), np.int64)


def edge_positions(n0, n):
    """the compact columns that `edges` puts on edge_columns(n), ascending; the last is n0 - 1"""
    E = edge_columns(n)
    k = len(E)
    p = np.empty(k, np.int64)
    p[-1] = n0 - 1
    for i in range(k - 2, -1, -1):       # spread over [0, n0), but never further apart than the columns they land on
        p[i] = max(min((i + 1) * n0 // (k + 1), p[i + 1] - 1), p[i + 1] - (E[i + 1] - E[i]))
    assert 0 < p[0] <= E[0] and (np.diff(p) >= 1).all() and (np.diff(p) <= np.diff(E)).all(), (n0, n)
    return p


def phi(name, n0, n):
    """the map `name` as an int64 array of n0 columns"""
    j = np.arange(n0, dtype=np.int64)
    if name == "top":
        return n - n0 + j
    if name == "spread":
        out = j * ((n - 1) // (n0 - 1))
        out[-1] = n - 1
        return out
    assert name == "edges", name
    E, p = edge_columns(n), edge_positions(n0, n)
    out = np.empty(n0, np.int64)
    out[:p[0]] = j[:p[0]] * (E[0] // p[0])
    for i in range(len(E) - 1):
        span = p[i + 1] - p[i]
        out[p[i]:p[i + 1]] = E[i] + j[:span] * ((E[i + 1] - E[i]) // span)
    out[p[-1]] = E[-1]
    return out


def relabel(M, f, n):
    """M with column c renamed f[c] and n columns; rows, order inside the rows and values as they are"""
    cols = np.asarray(f, np.int64)[np.asarray(M.colInd, np.int64)]
    assert len(cols) == 0 or (0 <= cols.min() and cols.max() < n <= (1 << 31) - 1)
    return type(M)(M.rowPtr, cols.astype(np.int32), M.values, M.rows, n)


# ---- the reference -------------------------------------------------------------------------------------------------------
def is_double(M):
    return np.asarray(M.values).dtype == np.float64


def product(A, B):
    """A * B on the CPU: the C oracle for float operands, the expanded float64 product (f64ref) for double ones"""
    if is_double(A):
        R = spgemm_f64(A, B)
        return Host64(R.rowPtr, R.colInd, R.values, R.rows, R.cols)
    return po.sequential_spmm(A, B)


def sorted_bits(M):
    """(rowPtr, columns, value bits) as bytes, columns ascending inside every row"""
    rp = np.asarray(M.rowPtr, np.int64)
    row_of = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    order = np.lexsort((np.asarray(M.colInd, np.int64), row_of))
    v = np.ascontiguousarray(np.asarray(M.values)[order])
    return rp.astype(np.int32).tobytes(), np.asarray(M.colInd, np.int32)[order].tobytes(), v.tobytes(), str(v.dtype)


def row_products(A, B):
    blen = np.diff(np.asarray(B.rowPtr, np.int64))
    csum = np.concatenate([[0], np.cumsum(blen[np.asarray(A.colInd, np.int64)])])
    rp = np.asarray(A.rowPtr, np.int64)
    return csum[rp[1:]] - csum[rp[:-1]]


def bin_rows(products):
    """rows per bin of product counts, as the library reports them (Stats.bin_rows)"""
    return [int(x) for x in np.bincount(np.searchsorted(np.asarray(BIN_LAST), products, side="left"), minlength=9)]


# ---- the case builder ----------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, A, B, claims):
        self.name, self.A, self.B = name, A, B
        self.claims = np.asarray(claims, np.int64).reshape(-1, 2)          # per row of A: products, distinct columns
        self.products = self.claims[:, 0]
        self.rehits = self.claims[:, 0] - self.claims[:, 1]
        self._want = None

    def want(self):
        """the compact product, computed once and left alone"""
        if self._want is None:
            self._want = product(self.A, self.B)
        return self._want


class Builder:
    """B rows over n0 compact columns: disjoint rows of L columns cut from one permutation (row 0 holds columns 0 and
    n0 - 1), and on demand parts of them.  A row of A with d distinct columns takes the first d // L disjoint rows and a
    part of the next (its lowest columns and its highest); its further products re-hit those d columns in turn, L at a time,
    through B rows of their own.  Rows of A share B rows freely."""

    def __init__(self, seed, n0=N0):
        perm = np.random.default_rng(seed).permutation(n0).astype(np.int64)
        self.perm = np.concatenate([[0, n0 - 1], perm[(perm != 0) & (perm != n0 - 1)]])
        self.n0 = n0
        self.brows, self.made, self.arows, self.claims = [], {}, [], []

    def _brow(self, key, cols):
        if key not in self.made:
            self.made[key] = len(self.brows)
            self.brows.append(np.sort(np.asarray(cols, np.int64)))
        return self.made[key]

    def _base(self, i):
        return np.sort(self.perm[i * L:(i + 1) * L])

    def add_columns(self, cols, products):
        """a row over exactly the columns `cols` (at most L of them), hit in turn until it has `products` products"""
        cols = np.asarray(cols, np.int64)
        d = len(cols)
        assert 1 <= d <= L and products >= d
        ent = [self._brow(("cols", cols.tobytes(), k), cols) for k in range(products // d)]
        if products % d:
            ent.append(self._brow(("cols", cols.tobytes(), "rest", products % d), cols[:products % d]))
        self.arows.append(np.sort(np.asarray(ent, np.int64)))
        self.claims.append((products, d))

    def add(self, products, distinct):
        assert (products == 0 and distinct == 0) or 1 <= distinct <= products
        assert distinct <= (self.n0 // L) * L
        nfull, rem = divmod(distinct, L)
        ent = [self._brow(("base", i), self._base(i)) for i in range(nfull)]
        dcols = [self._base(i) for i in range(nfull)]
        if rem:
            c = self._base(nfull)
            part = np.r_[c[:rem - 1], c[-1:]] if rem >= 2 else c[:1]
            ent.append(self._brow(("part", nfull, rem), part))
            dcols.append(part)
        dcols = np.concatenate(dcols) if dcols else np.zeros(0, np.int64)
        left, at, k, chunk = products - distinct, 0, 0, min(L, max(distinct, 1))
        while left > 0:
            take = min(chunk, left)
            ent.append(self._brow(("hit", distinct, k, take), dcols[(at + np.arange(take)) % distinct]))
            at, left, k = at + take, left - take, k + 1
        assert len(set(ent)) == len(ent)
        self.arows.append(np.sort(np.asarray(ent, np.int64)))
        self.claims.append((products, distinct))

    def finish(self, name, seed, dtype=np.float32):
        rng = np.random.default_rng(seed)

        def csr(rows, ncols):
            rp = np.zeros(len(rows) + 1, np.int32)
            rp[1:] = np.cumsum([len(r) for r in rows])
            ci = np.concatenate(list(rows) + [np.zeros(0, np.int64)]).astype(np.int32)
            if np.dtype(dtype) == np.float64:
                return Host64(rp, ci, (2 * rng.integers(0, 1 << 11, size=len(ci)) + 1) * 2.0 ** -30, len(rows), ncols)
            return po.CSRHost(rp, ci, rng.integers(1, 5, size=len(ci)).astype(np.float32), len(rows), ncols)

        B = csr(self.brows, self.n0)
        A = csr(self.arows, len(self.brows))
        return Case(name, A, B, self.claims)


# ---- the cases -----------------------------------------------------------------------------------------------------------
BIN_PRODUCTS = (0, 1, 2, 4, 5, 16, 17, 64, 65, 512, 513, 2048, 2049, 4096, 4097)
BH_CAP = 11264                           # distinct columns of one pass of the big rows' hash kernel


def case_bins(dtype=np.float32):
    """every bin at both ends, each row twice: all columns distinct (the expanded / direct store), and about half of the
    products on a repeated column (the table insert and the LDS add)"""
    b = Builder(11)
    for p in BIN_PRODUCTS:
        b.add(p, p)
        b.add(p, (p + 1) // 2)
    return b.finish("bins", 12, dtype)


def case_big(dtype=np.float32):
    """four rows of more than 4096 products: 4097 all distinct; about 6000 with repeats; 12 288 distinct columns, more than
    one pass of the hash kernel holds (classes and parking); 4200 products on 70 columns"""
    b = Builder(21)
    b.add(4097, 4097)
    b.add(6000, 5000)
    b.add(12288 + 500, 12288)
    b.add(4200, 70)
    assert 12288 > BH_CAP
    return b.finish("big", 22, dtype)


MID_ROWS = ((513, 10), (2048, 10), (1025, 10),            # up to 448 re-hits: the wave kernel (bin 6)
            (513, 449), (2048, 896),                      # 449-896: the four-wave kernel in bin 6
            (2049, 10), (4096, 896),                      # ... and in bin 7
            (1025, 900), (4096, 2000))                    # more than 896: the hash kernel of the bin


def case_mid():
    """rows of 513-4096 products at the smallest and the largest product count of every numeric route (and of the two
    symbolic kernels of bin 6, whose ends are 513 and 2048, and 1025 for the whole-block mode of the pair kernel)"""
    b = Builder(31)
    for products, rehits in MID_ROWS:
        b.add(products, products - rehits)
    return b.finish("mid", 32)


def case_sym(n):
    """for the symbolic pass alone at width n: a big row whose columns are exactly the window-edge columns of `edges` (a
    column counted in two windows or in none shows in its count), a big row with repeats, and a row of every bin's end"""
    b = Builder(41)
    b.add_columns(edge_positions(N0, n), 4104)
    b.add(6000, 5000)
    for p in BIN_PRODUCTS:
        b.add(p, (p + 1) // 2)
    return b.finish(f"sym-{n}", 42)


F64_WIDE = 2561 * L                      # 163 904 distinct columns: the device-memory table of the double path


def case_wide_f64():
    """one row of 2 561 B rows of 64: more distinct columns than any LDS pass scheme of the double path takes"""
    b = Builder(51)
    b.add(F64_WIDE + 640, F64_WIDE)
    return b.finish("wide-f64", 52, np.float64)
