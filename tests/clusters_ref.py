"""numpy restatement of the clusters entry points (include/spgemm_hip.h "clusters from a finished R-MCL result"): the
reference has no counterpart (it stops at Mt, nlibs/qrmcl.cc:136-164), so this module is what pins the semantics.
Everything is integers: every comparison against it is exact equality.

  attractors(rowPtr, colInd, values)   per row the column of the largest value under the tie rule
  components(m, rowPtr, colInd)        union-find -> the smallest vertex id of every vertex's component
  compact(label)                       canonical labels -> (k, cluster, ptr, members)
  rmcl_clusters(rowPtr, colInd, values) the three chained on the functional graph i -> parent[i]
"""
import numpy as np

INT_MAX = 2 ** 31 - 1


def attractors(rowPtr, colInd, values):
    """parent[i] = column of the largest value of row i.  (v, c) beats (bv, bc) iff v > bv, or v == bv and c < bc, from
    (-inf, INT_MAX): equal maxima -> the smallest column; NaN never wins (both comparisons are false); -0.0 == +0.0;
    an empty or all-NaN row -> i.  Compared in the dtype of `values`; a plain loop in storage order."""
    rowPtr = np.asarray(rowPtr, np.int64)
    colInd = np.asarray(colInd)
    values = np.asarray(values)
    m = len(rowPtr) - 1
    parent = np.arange(m, dtype=np.int32)
    ninf = values.dtype.type(-np.inf)
    for i in range(m):
        a, b = int(rowPtr[i]), int(rowPtr[i + 1])
        if a == b:
            continue
        bv, bc = ninf, INT_MAX
        if b - a > 64:                                  # long rows: the same rule, vectorised
            v, c = values[a:b], colInd[a:b]
            ok = ~np.isnan(v)
            if ok.any():
                top = v[ok].max()
                bc = int(c[ok][v[ok] == top].min())
        else:
            for v, c in zip(values[a:b], colInd[a:b]):
                if v > bv or (v == bv and c < bc):
                    bv, bc = v, int(c)
        if bc != INT_MAX:
            parent[i] = bc
    return parent


def components(m, rowPtr, colInd):
    """weakly connected components of a square pattern, every stored (i, j) an undirected edge -> (label, ncomp):
    label[v] = the smallest vertex id of v's component.  Union-find that always hangs the larger root under the smaller,
    so a root is its tree's minimum."""
    rowPtr = np.asarray(rowPtr, np.int64)
    colInd = np.asarray(colInd, np.int64)
    f = list(range(m))

    def find(x):
        r = x
        while f[r] != r:
            r = f[r]
        while f[x] != r:
            f[x], x = r, f[x]
        return r

    src = np.repeat(np.arange(m, dtype=np.int64), np.diff(rowPtr))
    for u, v in zip(src.tolist(), colInd.tolist()):
        a, b = find(u), find(v)
        if a != b:
            f[max(a, b)] = min(a, b)
    label = np.array([find(v) for v in range(m)], dtype=np.int32).reshape(m)
    return label, int(np.count_nonzero(label == np.arange(m)))


def is_canonical(label):
    label = np.asarray(label, np.int64)
    v = np.arange(len(label))
    return bool(np.all((label >= 0) & (label <= v)) and np.all(label[label] == label))


def compact(label):
    """canonical labels -> (k, cluster, ptr, members): clusters numbered by ascending smallest member, members ascending
    inside a cluster"""
    label = np.asarray(label, np.int64)
    m = len(label)
    assert is_canonical(label)
    root = label == np.arange(m)
    rank = np.cumsum(root) - root                       # exclusive scan
    k = int(root.sum())
    cluster = rank[label].astype(np.int32) if m else np.zeros(0, np.int32)
    members = np.argsort(cluster, kind="stable").astype(np.int32)
    ptr = np.zeros(k + 1, np.int32)
    np.cumsum(np.bincount(cluster, minlength=k), out=ptr[1:])
    return k, cluster, ptr, members


def rmcl_clusters(rowPtr, colInd, values):
    """-> (k, cluster, ptr, members, parent, label) of a flow matrix: components of the functional graph i -> parent[i]"""
    parent = attractors(rowPtr, colInd, values)
    m = len(parent)
    label, _ = components(m, np.arange(m + 1), parent)
    return compact(label) + (parent, label)
