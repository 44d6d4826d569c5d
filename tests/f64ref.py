"""Float64 reference for the double-precision SpGEMM tests (the C oracle is float-only).

Every product (row, col, a*b) is expanded with numpy, sorted by (row, col) and summed, so structural zeros and repeated
columns are kept exactly as the reference's kernels keep them (scipy.sparse would drop exact zeros).  For every entry the
reference also returns S = sum |a*b| and N = the number of terms: two summation orders of the same N terms differ by at
most 2 * N * 2^-53 * S (each is within (N-1) * 2^-53 * S of the exact sum), which is the acceptance bound of a value.
"""
import numpy as np

EPS64 = 2.0 ** -53


class Host64:
    """host CSR triple with float64 values (the oracle's CSRHost casts values to float32)"""

    def __init__(self, rowPtr, colInd, values, rows, cols):
        self.rowPtr = np.ascontiguousarray(rowPtr, dtype=np.int32)
        self.colInd = np.ascontiguousarray(colInd, dtype=np.int32)
        self.values = np.ascontiguousarray(values, dtype=np.float64)
        self.rows, self.cols = int(rows), int(cols)
        self.nnz = int(self.rowPtr[-1]) if len(self.rowPtr) else 0


class Ref64:
    def __init__(self, rowPtr, colInd, values, absSum, nterms, rows, cols):
        self.rowPtr, self.colInd, self.values = rowPtr, colInd, values
        self.absSum, self.nterms = absSum, nterms
        self.rows, self.cols, self.nnz = rows, cols, len(colInd)


def expand_products(IA, JA, VA, IB, JB, VB, rows):
    """-> (row, col, a*b) of every intermediate product of A*B (A given by IA/JA/VA with `rows` rows)."""
    IA = np.asarray(IA, np.int64)
    JA = np.asarray(JA, np.int64)
    IB = np.asarray(IB, np.int64)
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(IA))
    blen = IB[JA + 1] - IB[JA]
    total = int(blen.sum())
    owner = np.repeat(np.arange(len(JA), dtype=np.int64), blen)
    first = np.cumsum(blen) - blen
    bidx = IB[JA][owner] + (np.arange(total, dtype=np.int64) - first[owner])
    vals = np.asarray(VA, np.float64)[owner] * np.asarray(VB, np.float64)[bidx]
    return row_of[owner], np.asarray(JB, np.int64)[bidx], vals


def spgemm_f64(A, B):
    """A*B in float64 for objects with rowPtr/colInd/values/rows/cols: rows column-sorted, plus S and N per entry."""
    r, c, v = expand_products(A.rowPtr, A.colInd, A.values, B.rowPtr, B.colInd, B.values, A.rows)
    key = r * max(int(B.cols), 1) + c
    order = np.argsort(key, kind="stable")
    key, v = key[order], v[order]
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if len(key) else np.zeros(0, np.int64)
    vals = np.add.reduceat(v, starts) if len(key) else np.zeros(0)
    S = np.add.reduceat(np.abs(v), starts) if len(key) else np.zeros(0)
    N = np.diff(np.r_[starts, len(key)]).astype(np.int64)
    ukey = key[starts]
    urow = ukey // max(int(B.cols), 1)
    rp = np.zeros(A.rows + 1, np.int64)
    np.add.at(rp, urow + 1, 1)
    return Ref64(np.cumsum(rp).astype(np.int32), (ukey % max(int(B.cols), 1)).astype(np.int32), vals, S, N, A.rows, B.cols)


def sorted_rows(rowPtr, colInd, values):
    """(colInd, values) sorted by column inside every row (values keep their dtype)."""
    rp = np.asarray(rowPtr, np.int64)
    row_of = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    order = np.lexsort((np.asarray(colInd, np.int64), row_of))
    return np.asarray(colInd)[order], np.asarray(values)[order]


def bound_violations(values_sorted, ref):
    """entries (indices into the sorted arrays) where |x - ref| > 2 * N * 2^-53 * S"""
    x = np.asarray(values_sorted, np.float64)
    err = np.abs(x - ref.values)
    return np.flatnonzero(err > 2.0 * ref.nterms * EPS64 * ref.absSum)
