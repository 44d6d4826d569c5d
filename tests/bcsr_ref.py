"""numpy / Python restatement of the blocked CSR (BCSR), the expected side of the BCSR tests, written from the contract in
include/spgemm_hip.h ("blocked CSR"):

  to_bcsr(A, r, c)        BCSR::BCSR(const CSR&, r, c)     nlibs/BCSR.cc:3-65     sequential: the block row's rows ascending,
                                                                                  each in storage order; a block column is
                                                                                  appended when first met; a later store to
                                                                                  a cell overwrites an earlier one
  to_csr(B, drop_tol)     the row walk of BCSR::isEqual    nlibs/BCSR.cc:67-116   tile after tile, ej = 0..c-1, a cell kept when
                                                                                  its column < n and fabs((double)v) > drop_tol
  density(B)              BCSR::nonzeroDensity             nlibs/BCSR.h:61-63

There is no reference binary for BCSR, so tests/test_bcsr_abi.py pins this file on hand-worked matrices.  Inputs expose
rowPtr / colInd / values / rows / cols; values keep the input's dtype and bits (they are moved, never computed)."""
import numpy as np

import reorder_ref as rr


class Blocked:
    def __init__(self, rowPtr, colInd, values, m, n, r, c, nnz):
        self.rowPtr = np.ascontiguousarray(rowPtr, dtype=np.int32)
        self.colInd = np.ascontiguousarray(colInd, dtype=np.int32)
        self.values = np.ascontiguousarray(values)
        self.m, self.n, self.r, self.c, self.nnz = int(m), int(n), int(r), int(c), int(nnz)
        self.bm, self.bn = (self.m + self.r - 1) // self.r, (self.n + self.c - 1) // self.c
        self.nnzb = int(self.rowPtr[-1])


def to_bcsr(A, r, c):
    m, n = A.rows, A.cols
    rp, ci, v = np.asarray(A.rowPtr, np.int64), np.asarray(A.colInd, np.int64), np.asarray(A.values)
    bm = (m + r - 1) // r
    rowPtr, colInd, tiles = [0], [], []
    for bi in range(bm):
        where = {}                                          # block column -> tile of this block row
        for i in range(bi * r, min(bi * r + r, m)):
            for j in range(rp[i], rp[i + 1]):
                col = int(ci[j])
                bcol = col // c
                if bcol not in where:
                    where[bcol] = len(tiles)
                    colInd.append(bcol)
                    tiles.append(np.zeros(r * c, v.dtype))  # +0.0 everywhere
                tiles[where[bcol]][(i % r) * c + col % c] = v[j]       # the last store stays
        rowPtr.append(len(tiles))
    values = np.concatenate(tiles) if tiles else np.zeros(0, v.dtype)
    return Blocked(rowPtr, colInd, values, m, n, r, c, int(rp[m]) if m else 0)


def to_csr(B, drop_tol=1e-9):
    r, c = B.r, B.c
    tiles = B.values.reshape(B.nnzb, r, c)
    rowPtr, cols, vals = [0], [], []
    for i in range(B.m):
        bi, ei = divmod(i, r)
        s, e = int(B.rowPtr[bi]), int(B.rowPtr[bi + 1])
        cell_v = tiles[s:e, ei, :].reshape(-1)              # the row's cells in walk order: tile after tile, ej ascending
        cell_c = (B.colInd[s:e].astype(np.int64)[:, None] * c + np.arange(c, dtype=np.int64)[None, :]).reshape(-1)
        with np.errstate(invalid="ignore"):
            keep = (cell_c < B.n) & (np.abs(cell_v.astype(np.float64)) > float(drop_tol))     # false for NaN
        cols.append(cell_c[keep])
        vals.append(cell_v[keep])
        rowPtr.append(rowPtr[-1] + int(keep.sum()))
    colInd = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    values = np.concatenate(vals) if vals else np.zeros(0, B.values.dtype)
    return rr.Host(rowPtr, colInd, values, B.m, B.n)


def density(B):
    cells = B.nnzb * B.r * B.c
    return B.nnz / cells * 100.0 if cells else 0.0


def same_bits(X, Y):
    """the three arrays of two Blocked: rowPtr, colInd and the value BITS equal"""
    return ((X.m, X.n, X.r, X.c) == (Y.m, Y.n, Y.r, Y.c) and np.array_equal(X.rowPtr, Y.rowPtr) and
            np.array_equal(X.colInd, Y.colInd) and X.values.dtype == Y.values.dtype and
            X.values.tobytes() == Y.values.tobytes())
