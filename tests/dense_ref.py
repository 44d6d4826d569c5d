"""numpy restatement of the dense matrix entry points, the expected side of the dense tests, written from the contract in
include/spgemm_hip.h ("dense matrix"):

  to_dense(A)             DenseMatrix::DenseMatrix(const CSR&)   nlibs/DenseMatrix.h:6-21   zero-fill, then every entry in
                                                                                            storage order: a later store to
                                                                                            a cell overwrites an earlier one
  to_csr(D, rule, tol)    CSR::initWithDenseMatrix               nlibs/CSR.h:54-82          row-major walk; KEEP_REFERENCE
                                                                                            drops a cell when (double)v < tol,
                                                                                            KEEP_ABS keeps it when
                                                                                            fabs((double)v) > tol

tests/test_dense_abi.py pins this file by hand.  Values keep the input's dtype and bits (they are moved, never computed).
The kernel geometry the GPU tests aim at is restated here, in one place (csrc/dense_device.hpp)."""
import numpy as np

import reorder_ref as rr

KEEP_REFERENCE, KEEP_ABS = 0, 1
SEG = 4096                      # DS_SEG: cells of a dense -> CSR segment
BM, BN, BK = 128, 128, 32       # GM_BM, GM_BN, GM_BK: the block tile of the product
CP_TILE = 1024                  # entries per block of the scatter kernel (csr_common_device.hpp)
RS_TILE = 2048                  # keys per block of the radix kernels (csr_common_device.hpp)


def to_dense(A):
    v = np.asarray(A.values)
    D = np.zeros((A.rows, A.cols), v.dtype)
    rows = np.repeat(np.arange(A.rows), np.diff(np.asarray(A.rowPtr, np.int64)))
    for i, j, x in zip(rows, np.asarray(A.colInd), v):          # sequential: the last store to a cell stays
        D[i, j] = x
    return D


def to_csr(D, rule=KEEP_REFERENCE, tol=1e-8):
    D = np.asarray(D)
    wide = D.astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = ~(wide < tol) if rule == KEEP_REFERENCE else np.abs(wide) > tol
    rowPtr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
    return rr.Host(rowPtr, np.nonzero(keep)[1], D[keep], D.shape[0], D.shape[1])   # boolean indexing walks row-major
