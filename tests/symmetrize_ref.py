"""numpy restatement of the sparse add and symmetrisation entry points (include/spgemm_hip.h "sparse add and the
symmetrisation of a directed graph").  The reference has no counterpart (its loader only transposes), so this module is
what pins the semantics; tests/test_symmetrize_abi.py pins `add` itself against dense numpy.

  add(A, B, alpha, beta)       per-row two-pointer merge in the value dtype, one rounding per operation
  scale(A, rowScale, colScale) (rowScale[r] * v) * colScale[c], a scale of None is not multiplied
  col_counts(A)                entries per column
  degree_factors(count, e, dt) count ** -e in float64, rounded to dt; 0 where the count is 0
  sym_sum / sym_bibliometric / sym_degree_discounted   the three symmetrisations, dense, in float64

Inputs expose rowPtr / colInd / values / rows / cols; sparse results are reorder_ref.Host triples."""
import numpy as np

from reorder_ref import Host, transpose  # noqa: F401  (transpose: A^T of a Host, for the callers)

SYM_SUM, SYM_BIBLIOMETRIC, SYM_DEGREE_DISCOUNTED = 0, 1, 2


def add(A, B, alpha=1.0, beta=1.0):
    """alpha * A + beta * B for operands with strictly ascending rows: the union of the patterns, rows ascending, an
    entry that sums to zero stays.  alpha and beta are converted once to the value type V; a common column gets
    V(alpha)*a + V(beta)*b (three roundings), a column of one operand V(alpha)*a or V(beta)*b."""
    assert (A.rows, A.cols) == (B.rows, B.cols) and A.values.dtype == B.values.dtype
    V = A.values.dtype.type
    al, be = V(alpha), V(beta)
    arp, brp = np.asarray(A.rowPtr, np.int64), np.asarray(B.rowPtr, np.int64)
    rp = np.zeros(A.rows + 1, np.int64)
    cols, vals = [], []
    with np.errstate(all="ignore"):
        ta, tb = al * A.values, be * B.values           # one rounding each, in V
        for r in range(A.rows):
            i, ie, j, je = int(arp[r]), int(arp[r + 1]), int(brp[r]), int(brp[r + 1])
            while i < ie or j < je:
                ca = A.colInd[i] if i < ie else None
                cb = B.colInd[j] if j < je else None
                if cb is None or (ca is not None and ca < cb):
                    cols.append(ca); vals.append(ta[i]); i += 1
                elif ca is None or cb < ca:
                    cols.append(cb); vals.append(tb[j]); j += 1
                else:
                    cols.append(ca); vals.append(ta[i] + tb[j]); i += 1; j += 1
            rp[r + 1] = len(cols)
    return Host(rp, np.array(cols, np.int32), np.array(vals, A.values.dtype), A.rows, A.cols)


def scale(A, rowScale=None, colScale=None):
    """-> the values (rowScale[r] * v) * colScale[c] in A's dtype: the row factor first, then the column factor"""
    v = np.asarray(A.values).copy()
    row_of = np.repeat(np.arange(A.rows, dtype=np.int64), np.diff(np.asarray(A.rowPtr, np.int64)))
    with np.errstate(all="ignore"):
        if rowScale is not None:
            v = np.asarray(rowScale, v.dtype)[row_of] * v
        if colScale is not None:
            v = v * np.asarray(colScale, v.dtype)[np.asarray(A.colInd, np.int64)]
    return v


def col_counts(A):
    return np.bincount(np.asarray(A.colInd, np.int64), minlength=A.cols).astype(np.int32)[:A.cols]


def degree_factors(count, exponent, dtype):
    count = np.asarray(count, np.float64)
    out = np.zeros(len(count), np.float64)
    pos = count > 0
    out[pos] = np.power(count[pos], -float(exponent))
    return out.astype(dtype)


def to_dense(M, dtype=None):
    D = np.zeros((M.rows, M.cols), dtype or M.values.dtype)
    row_of = np.repeat(np.arange(M.rows, dtype=np.int64), np.diff(np.asarray(M.rowPtr, np.int64)))
    D[row_of, np.asarray(M.colInd, np.int64)] = M.values
    return D


def pattern(M):
    P = np.zeros((M.rows, M.cols), bool)
    row_of = np.repeat(np.arange(M.rows, dtype=np.int64), np.diff(np.asarray(M.rowPtr, np.int64)))
    P[row_of, np.asarray(M.colInd, np.int64)] = True
    return P


def from_dense(D, P):
    """the CSR that holds D where the pattern P is set"""
    r, c = np.nonzero(P)
    rp = np.zeros(D.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=D.shape[0]), out=rp[1:])
    return Host(rp, c, D[r, c], D.shape[0], D.shape[1])


def sym_sum(A):
    """A + A^T, sparse and in A's dtype (the bits hip_csr_symmetrize(SUM) returns)"""
    return add(A, transpose(A), 1.0, 1.0)


def _dense_pair(X, Y):
    """X Y^T-style sums evaluated densely in float64 with their patterns: (values, pattern) of X @ Y"""
    return X[0] @ Y[0], (X[1].astype(np.int64) @ Y[1].astype(np.int64)) > 0


def sym_bibliometric(A):
    """A A^T + A^T A, dense float64 -> Host (pattern: where either product has a term, cancelled or not)"""
    D, P = to_dense(A, np.float64), pattern(A)
    v1, p1 = _dense_pair((D, P), (D.T, P.T))
    v2, p2 = _dense_pair((D.T, P.T), (D, P))
    return from_dense(v1 + v2, p1 | p2)


def sym_degree_discounted(A, alpha=0.5, beta=0.5):
    """Do^-a A Di^-b A^T Do^-a + Di^-b A^T Do^-a A Di^-b with Do / Di the out- / in-degree counts, dense float64"""
    D, P = to_dense(A, np.float64), pattern(A)
    do = degree_factors(np.diff(np.asarray(A.rowPtr, np.int64)), alpha, np.float64)
    di = degree_factors(col_counts(A), beta, np.float64)
    v1 = (do[:, None] * D * di[None, :]) @ (D.T * do[None, :])
    v2 = (di[:, None] * D.T * do[None, :]) @ (D * di[None, :])
    p1 = (P.astype(np.int64) @ P.T.astype(np.int64)) > 0
    p2 = (P.T.astype(np.int64) @ P.astype(np.int64)) > 0
    return from_dense(v1 + v2, p1 | p2)
