"""The numpy restatement the selection entry points (hip_csr_row_topk / _f64) are held to.

Row i keeps its min(len_i, k) best entries in their storage order.  Entry a beats entry b iff va > vb, or va == vb and
ca < cb, or both are equal and a is stored before b.  The two zeros are equal; a NaN ranks below every number (-inf
included), and among NaNs the column decides, then the position.  Values are compared in their own dtype.  With
normalise the kept values of the rows that were cut, and of those only, are divided in the value dtype by their sum
(math.fsum, rounded to the dtype); every other value keeps its bits."""
import math

import numpy as np

from reorder_ref import Host


def row_order(cols, vals):
    """the positions of a row's entries from the best to the worst"""
    vals = np.asarray(vals)
    nan = np.isnan(vals)
    worse = np.where(nan, vals.dtype.type(0), -vals) + vals.dtype.type(0)      # ascending = better first; -0.0 + 0.0 = +0.0
    pos = np.arange(len(vals))
    return np.lexsort((pos, np.asarray(cols), worse, nan))                     # the last key is the primary one


def keep_of_row(cols, vals, k):
    """the positions row_topk keeps, ascending (= storage order)"""
    return np.sort(row_order(cols, vals)[:k])


def row_topk(rowPtr, colInd, values, rows, cols, k, normalise=False):
    """-> (Host, rows_cut)"""
    rowPtr = np.asarray(rowPtr, np.int64)
    colInd = np.asarray(colInd, np.int32)
    values = np.asarray(values)
    assert k >= 1
    out_ptr = np.zeros(rows + 1, np.int64)
    keep_all, cut = [], 0
    out_vals = values.copy()
    for r in range(rows):
        a, b = int(rowPtr[r]), int(rowPtr[r + 1])
        if b - a <= k:
            keep = np.arange(a, b)
        else:
            cut += 1
            keep = a + keep_of_row(colInd[a:b], values[a:b], k)
            if normalise:
                den = values.dtype.type(math.fsum(float(x) for x in values[keep]))
                with np.errstate(all="ignore"):
                    out_vals[keep] = values[keep] / den
        keep_all.append(keep)
        out_ptr[r + 1] = out_ptr[r] + len(keep)
    sel = np.concatenate(keep_all).astype(np.int64) if keep_all else np.zeros(0, np.int64)
    return Host(out_ptr, colInd[sel], np.ascontiguousarray(out_vals[sel]), rows, cols), cut


def of(M, k, normalise=False):
    """row_topk of anything with rowPtr / colInd / values / rows / cols"""
    return row_topk(M.rowPtr, M.colInd, M.values, M.rows, M.cols, k, normalise)
