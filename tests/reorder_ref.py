"""numpy restatement of the reference's reordering operations, the expected side of the reorder tests.

  PM / MP / PMPt / PtMP             CSR::PM ... PtMP                     nlibs/CSR.cc:431-482
  permutation_transpose             permutationTranspose                 nlibs/tools/util.cc:162-168
  row_descending                    CSR::rowDescendingOrderPermutation   nlibs/CSR.cc:484-494 (ties: ascending row id)
  transpose                         the transposed load readSNAPFile(isTrans), as a stable sort by column

Inputs expose rowPtr / colInd / values / rows / cols; results are `Host` triples whose values keep the input's dtype.
tests/test_reorder_abi.py pins PM / MP to the reference's own identity (PM(M,P) == Pmat * M, MP(M,Q) == M * Qmat) and
transpose to the loader."""
import numpy as np


class Host:
    def __init__(self, rowPtr, colInd, values, rows, cols):
        self.rowPtr = np.ascontiguousarray(rowPtr, dtype=np.int32)
        self.colInd = np.ascontiguousarray(colInd, dtype=np.int32)
        self.values = np.ascontiguousarray(values)
        self.rows, self.cols = int(rows), int(cols)
        self.nnz = int(self.rowPtr[-1]) if len(self.rowPtr) else 0


def PM(M, P):
    """row i of the result = row P[i] of M, entries in M's in-row order"""
    P = np.asarray(P, np.int64)
    rp = np.asarray(M.rowPtr, np.int64)
    lens = (rp[1:] - rp[:-1])[P]
    out_rp = np.zeros(M.rows + 1, np.int64)
    np.cumsum(lens, out=out_rp[1:])
    # source position of every output entry: start of its source row + offset inside the row
    src = np.repeat(rp[:-1][P] - out_rp[:-1], lens) + np.arange(int(out_rp[-1]), dtype=np.int64)
    return Host(out_rp, np.asarray(M.colInd)[src], np.asarray(M.values)[src], M.rows, M.cols)


def MP(M, P):
    """column c of M becomes column P[c]; rows keep their storage order (unsorted afterwards)"""
    return Host(M.rowPtr, np.asarray(P, np.int32)[np.asarray(M.colInd, np.int64)], np.asarray(M.values).copy(), M.rows, M.cols)


def permutation_transpose(P):
    P = np.asarray(P, np.int64)
    Pt = np.empty(len(P), np.int32)
    Pt[P] = np.arange(len(P), dtype=np.int32)
    return Pt


def PMPt(M, P):
    return MP(PM(M, P), permutation_transpose(P))        # nlibs/CSR.cc:466-473


def PtMP(M, P):
    return PM(MP(M, P), permutation_transpose(P))        # nlibs/CSR.cc:475-482


def row_descending(rowPtr):
    lens = np.diff(np.asarray(rowPtr, np.int64))
    return np.argsort(-lens, kind="stable").astype(np.int32)


def transpose(M):
    ci = np.asarray(M.colInd, np.int64)
    rp = np.asarray(M.rowPtr, np.int64)
    order = np.argsort(ci, kind="stable")
    row_of = np.repeat(np.arange(M.rows, dtype=np.int32), np.diff(rp))
    t_rp = np.zeros(M.cols + 1, np.int64)
    np.cumsum(np.bincount(ci, minlength=M.cols)[:M.cols] if M.cols else np.zeros(0, np.int64), out=t_rp[1:])
    return Host(t_rp, row_of[order], np.asarray(M.values)[order], M.cols, M.rows)


def perm_matrix(P, cols=None):
    """Pmat: one 1.0 per row, at column P[i] (tests/CSR_test.cc:14-29 builds the same)"""
    P = np.asarray(P, np.int32)
    n = len(P)
    return Host(np.arange(n + 1, dtype=np.int32), P, np.ones(n, np.float32), n, n if cols is None else cols)


def sort_rows(M):
    """rows sorted by column, stable (entries of one column keep their order)"""
    rp = np.asarray(M.rowPtr, np.int64)
    row_of = np.repeat(np.arange(M.rows, dtype=np.int64), np.diff(rp))
    order = np.lexsort((np.asarray(M.colInd, np.int64), row_of))
    return Host(M.rowPtr, np.asarray(M.colInd)[order], np.asarray(M.values)[order], M.rows, M.cols)


def same_bits(X, Y):
    """rowPtr, colInd and the value BITS equal"""
    xv, yv = np.ascontiguousarray(X.values), np.ascontiguousarray(Y.values)
    return (X.rows == Y.rows and X.cols == Y.cols and np.array_equal(np.asarray(X.rowPtr), np.asarray(Y.rowPtr)) and
            np.array_equal(np.asarray(X.colInd), np.asarray(Y.colInd)) and xv.dtype == yv.dtype and
            xv.tobytes() == yv.tobytes())
