"""numpy restatement of the reference's column-partitioned CSR, the expected side of the PCSR tests.

  split            PCSR::PCSR(const CSR&, c)        nlibs/PCSR.cc:3-56     (the two passes over the rows, as one stable sort)
  join             the row walk of PCSR::isEqual    nlibs/PCSR.h:69-86     (block 0's row i, block 1's row i, ...)
  spmm             spmm(A, pB)                      correctTests/pcsrTest.cc:7-19, through the oracle's product

stride = (n + c - 1) / c (1 when n == 0); an entry with column col goes to block col / stride with local column
col - block * stride.  Inputs expose rowPtr / colInd / values / rows / cols; a split is a `Split` (the packed arrays as
hip_csr_split_columns returns them), whose block(b) is a reorder_ref.Host of shape rows x stride; values keep the
input's dtype.  tests/test_pcsr_abi.py pins split and join on a hand-worked 3 x 5 matrix."""
import numpy as np

from reorder_ref import Host


def stride_of(n, c):
    return max(1, (int(n) + int(c) - 1) // int(c))


class Split:
    def __init__(self, rowPtrs, colInd, values, blockPtr, rows, cols, c):
        self.rowPtrs = np.ascontiguousarray(rowPtrs, dtype=np.int32)        # c * (rows + 1), block b's at b * (rows + 1)
        self.colInd = np.ascontiguousarray(colInd, dtype=np.int32)          # local columns, block b's at blockPtr[b]
        self.values = np.ascontiguousarray(values)
        self.blockPtr = np.ascontiguousarray(blockPtr, dtype=np.int32)      # c + 1
        self.rows, self.cols, self.c = int(rows), int(cols), int(c)
        self.stride = stride_of(cols, c)

    def block(self, b):
        s, e = int(self.blockPtr[b]), int(self.blockPtr[b + 1])
        rp = self.rowPtrs[b * (self.rows + 1):(b + 1) * (self.rows + 1)]
        return Host(rp, self.colInd[s:e], self.values[s:e], self.rows, self.stride)

    def blocks(self):
        return [self.block(b) for b in range(self.c)]


def split(M, c):
    """entries ordered by (block, row, storage order): a stable sort by block id of entries already in row order"""
    c = int(c)
    stride = stride_of(M.cols, c)
    ci = np.asarray(M.colInd, np.int64)
    rp = np.asarray(M.rowPtr, np.int64)
    block = ci // stride
    assert len(ci) == 0 or (ci.min() >= 0 and block.max() < c)
    order = np.argsort(block, kind="stable")
    row_of = np.repeat(np.arange(M.rows, dtype=np.int64), np.diff(rp))
    blockPtr = np.zeros(c + 1, np.int64)
    np.cumsum(np.bincount(block, minlength=c), out=blockPtr[1:])
    rowPtrs = np.zeros((c, M.rows + 1), np.int64)
    if M.rows:
        counts = np.bincount(block * M.rows + row_of, minlength=c * M.rows).reshape(c, M.rows)
        np.cumsum(counts, axis=1, out=rowPtrs[:, 1:])
    return Split(rowPtrs.reshape(-1), (ci - block * stride)[order], np.asarray(M.values)[order], blockPtr, M.rows, M.cols, c)


def join(blocks, cols):
    """blocks: c CSRs of shape rows x stride.  Row i = block 0's row i, block 1's row i, ...; block b's columns + b * stride"""
    c, rows = len(blocks), blocks[0].rows
    stride = stride_of(cols, c)
    rps = [np.asarray(B.rowPtr, np.int64) for B in blocks]
    lens = np.stack([np.diff(rp) for rp in rps]) if rows else np.zeros((c, 0), np.int64)       # [c][rows]
    out_rp = np.zeros(rows + 1, np.int64)
    np.cumsum(lens.sum(axis=0), out=out_rp[1:])
    nnz = int(out_rp[-1])
    dtype = np.asarray(blocks[0].values).dtype
    ci, v = np.zeros(nnz, np.int32), np.zeros(nnz, dtype)
    before = np.cumsum(lens, axis=0) - lens                 # entries of the same row in the blocks in front of b
    for b, B in enumerate(blocks):
        n_b = int(rps[b][-1])
        if n_b == 0:
            continue
        row_of = np.repeat(np.arange(rows, dtype=np.int64), lens[b])
        dst = out_rp[:-1][row_of] + before[b][row_of] + (np.arange(n_b, dtype=np.int64) - rps[b][:-1][row_of])
        ci[dst] = np.asarray(B.colInd, np.int64)[:n_b] + b * stride
        v[dst] = np.asarray(B.values)[:n_b]
    return Host(out_rp, ci, v, rows, cols)


def stable_partition(M, c):
    """join(split(M, c)): M with every row stably partitioned by block"""
    return join(split(M, c).blocks(), M.cols)


def spmm(A, S, product):
    """spmm(A, pB): product(A, block) per block -> list of c results (each A.rows x stride, local columns)"""
    return [product(A, B) for B in S.blocks()]
