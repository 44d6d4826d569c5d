"""numpy / Python restatement of the mixed CSR (MCSR), the expected side of the MCSR tests, written from the contract in
include/spgemm_hip.h ("mixed CSR") on top of tests/bcsr_ref.py:

  to_mcsr(A, r, c, blockRows, blockCols)   the FILL pass of MCSR::MCSR     nlibs/MCSR.cc:58-92   an entry (i, col) with
                                                                          i < blockRows and col < blockCols goes into its
                                                                          tile, every other entry into the remainder, both
                                                                          in A's storage order
  to_csr(M, drop_tol)                      defined here (the reference has no MCSR::isEqual): row i < blockRows is the
                                           corner's row as bcsr_ref.to_csr writes it, then the remainder's row

The reference's count pass (nlibs/MCSR.cc:16-40) is wrong for r > 1 and is not restated.  tests/test_mcsr_abi.py pins this
file on the reference's known-answer vectors (tests/golden/mcsr_kat.json, r = 1) and on a hand-worked r > 1 case."""
import numpy as np

import bcsr_ref as br
import reorder_ref as rr


class Mixed:
    """corner: a bcsr_ref.Blocked of shape blockRows x blockCols whose nnz is the number of entries that went into it;
    rest: an m x n rr.Host with global columns"""

    def __init__(self, corner, rest, m, n, blockRows, blockCols):
        self.corner, self.rest = corner, rest
        self.m, self.n, self.blockRows, self.blockCols = int(m), int(n), int(blockRows), int(blockCols)


def to_mcsr(A, r, c, blockRows, blockCols):
    assert blockRows % r == 0 and 0 <= blockRows <= A.rows and 0 <= blockCols <= A.cols
    rp, ci, v = np.asarray(A.rowPtr, np.int64), np.asarray(A.colInd, np.int64), np.asarray(A.values)
    row_of = np.repeat(np.arange(A.rows, dtype=np.int64), np.diff(rp))
    inside = (row_of < blockRows) & (ci < blockCols)

    def part(keep, rows, cols):
        ptr = np.zeros(rows + 1, np.int64)
        np.cumsum(np.bincount(row_of[keep], minlength=max(rows, 1))[:rows], out=ptr[1:])
        return rr.Host(ptr, ci[keep], v[keep], rows, cols)

    return Mixed(br.to_bcsr(part(inside, blockRows, blockCols), r, c), part(~inside, A.rows, A.cols), A.rows, A.cols,
                 blockRows, blockCols)


def to_csr(M, drop_tol=1e-9):
    top, rest = br.to_csr(M.corner, drop_tol), M.rest
    dtype = np.asarray(rest.values).dtype
    rowPtr, cols, vals, count = [0], [np.zeros(0, np.int32)], [np.zeros(0, dtype)], 0
    for i in range(M.m):
        for part in ([top] if i < M.blockRows else []) + [rest]:           # the corner's row first
            s, e = int(part.rowPtr[i]), int(part.rowPtr[i + 1])
            cols.append(np.asarray(part.colInd)[s:e])
            vals.append(np.asarray(part.values, dtype)[s:e])
            count += e - s
        rowPtr.append(count)
    return rr.Host(rowPtr, np.concatenate(cols), np.concatenate(vals), M.m, M.n)


def density(M):
    return br.density(M.corner)
