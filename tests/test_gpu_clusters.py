"""GPU (-m gpu): clusters from an R-MCL result on the device -- hip_rmcl_attractors, hip_csr_connected_components,
hip_labels_to_clusters, hip_rmcl_clusters and the _f64 twins -- against the numpy restatement tests/clusters_ref.py (pinned
by hand in tests/test_clusters_abi.py).  Every result is integers: every comparison is exact equality."""
import functools
import os
import subprocess

import numpy as np
import pytest

from devcsr import built_gpu, handle  # noqa: F401
from devcsr import to_hs
from helpers import DATA, ROOT, po
from sparse_matrix_with_flops_amd import hipspgemm as hs
import clusters_ref as cr

pytestmark = pytest.mark.gpu

ERR_INPUT = "status 5"
DTYPES = [np.float32, np.float64]
# filler rows (count, length) that put the mean row length of the attractor matrix into each group width's range
FILLER = {4: (4000, 2), 16: (1000, 20), 64: (300, 300)}


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _assemble(rows, dtype):
    """rows: list of (columns, values) -> rowPtr, colInd, values"""
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(c) for c, _ in rows])
    ci = np.concatenate([np.asarray(c, np.int32) for c, _ in rows]) if rows else np.zeros(0, np.int32)
    v = np.concatenate([np.asarray(x, dtype) for _, x in rows]) if rows else np.zeros(0, dtype)
    return rp, ci, v


def _tie_row(length, at, order):
    """`length` entries with distinct columns, values below 1.5, the maximum 2.0 stored at the positions `at`; order[j] =
    rank of the column that goes to at[j] (0 = the smallest column of the row), so the winner sits at at[order.index(0)]"""
    rng = np.random.default_rng(length * 31 + sum(at))
    cols = 5 + rng.permutation(length)                           # distinct, all >= 5
    vals = 0.25 + rng.random(length)
    for j, p in enumerate(at):
        cols[p] = order[j]                                       # 0, 1, 2: below every other column
        vals[p] = 2.0
    return cols, vals


@functools.lru_cache(maxsize=None)
def attractor_case(G, dtype):
    """-> rowPtr, colInd, values (dtype), the reference parents: every row length at which a G-lane group changes its
    trip count, a 20 000-entry row, repeated maxima across the group / stride boundary, the special values"""
    fill_n, fill_len = FILLER[G]
    lengths = [0, 1, G - 1, G, G + 1, 63, 64, 65, 20000]
    nan, inf = np.nan, np.inf
    two = [(G - 1, G), (0, 3 * G), (G, 2 * G - 1)]
    three = [(G - 1, G, 2 * G + 1), (0, G, 2 * G), (G - 1, 2 * G - 1, 3 * G - 1)]
    ties = [_tie_row(4 * G + 3, at, order) for at in two for order in ((0, 1), (1, 0))]
    ties += [_tie_row(4 * G + 3, at, order) for at in three for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0))]
    special = [([7, 3, 9], [nan, 0.5, nan]),                     # NaN beside finite values
               ([1, 2], [nan, nan]),                             # all NaN: the row itself
               ([9, 4, 6], [-inf, -inf, -inf]),                  # only -inf: the smallest column
               ([8, 2, 5], [-0.0, 0.0, -1.0]),                   # -0.0 == +0.0: the smaller column
               ([8, 2, 5], [0.0, -0.0, -1.0]),
               ([3, 6], [0.5 + 2.0 ** -40, 0.5 + 2.0 ** -39]),   # float64: the larger column wins; float: a tie, the smaller
               (list(range(10, 10 + G + 2)) + [4, 60], [0.5] * (G + 2) + [0.75, 0.75 + 2.0 ** -40])]
    m = len(lengths) + len(ties) + len(special) + fill_n
    assert m > 4 * G + 10                                        # every fixed column exists
    rng = np.random.default_rng(100 + G)
    rows = [(rng.integers(0, m, size=n), 0.25 + rng.random(n)) for n in lengths] + ties + special
    rows += [(rng.integers(0, m, size=fill_len), 0.25 + rng.random(fill_len)) for _ in range(fill_n)]
    rp, ci, v = _assemble(rows, dtype)
    assert hs.rmcl_attractor_lanes(m, len(ci)) == G, (G, m, len(ci))
    return rp, ci, v, cr.attractors(rp, ci, v)


def _shuffled(rp, ci, v, seed):
    """the same matrix, every row's entries in another order"""
    rng = np.random.default_rng(seed)
    ci, v = ci.copy(), v.copy()
    for a, b in zip(rp[:-1], rp[1:]):
        p = a + rng.permutation(b - a)
        ci[a:b], v[a:b] = ci[p], v[p]
    return ci, v


def _edges_csr(m, src, dst):
    """pattern CSR of the directed entries (src[i], dst[i]), kept in the given order inside a row"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.argsort(src, kind="stable")
    rp = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(src, minlength=m), out=rp[1:])
    return rp, dst[order].astype(np.int32)


def _clique(ids):
    ids = np.asarray(ids)
    return np.repeat(ids, len(ids)), np.tile(ids, len(ids))


def _graph(name):
    rng = np.random.default_rng(11)
    if name == "isolated":
        return _edges_csr(1000, [], [])
    if name == "path":                                           # 65 536 vertices, scrambled ids, one direction only
        p = rng.permutation(65536)
        return _edges_csr(65536, p[:-1], p[1:])
    if name == "path_sorted":                                    # ids ascend along the path: round 1 hooks it into ONE chain,
        v = np.arange(30000)                                     # far deeper than one bounded chase of the shortcut
        return _edges_csr(30000, v[:-1], v[1:])
    if name == "star":                                           # the hub is the largest id: one 70 000-entry row
        return _edges_csr(70001, np.full(70000, 70000), np.arange(70000))
    if name in ("cliques", "cliques_joined"):
        s1, d1 = _clique(np.arange(0, 600, 2))
        s2, d2 = _clique(np.arange(1, 600, 2))
        extra = ([599], [0]) if name == "cliques_joined" else ([], [])
        return _edges_csr(600, np.concatenate([s1, s2, extra[0]]), np.concatenate([d1, d2, extra[1]]))
    if name == "cycle_tails":                                    # a functional graph: a 1 000-cycle, tails of depth 2
        parent = np.concatenate([(np.arange(1000) + 1) % 1000, np.arange(1000), np.arange(1000, 2000)])
        return np.arange(3001, dtype=np.int32), parent.astype(np.int32)
    if name == "loops_repeats":
        src = rng.integers(0, 3000, size=2500)
        dst = rng.integers(0, 3000, size=2500)
        v = np.arange(3000)
        return _edges_csr(3000, np.concatenate([src, src, v[::3]]), np.concatenate([dst, dst, v[::3]]))
    if name == "forest":                                         # 100 000 vertices, about 1 000 trees, scrambled ids
        n = 100000
        up = (rng.random(n) * np.arange(n)).astype(np.int64)     # a parent below the vertex
        keep = (rng.random(n) > 0.01) & (np.arange(n) > 0)
        p = rng.permutation(n)
        return _edges_csr(n, p[np.arange(n)[keep]], p[up[keep]])
    raise KeyError(name)


GRAPHS = ["isolated", "path", "path_sorted", "star", "cliques", "cliques_joined", "cycle_tails", "loops_repeats", "forest"]


@functools.lru_cache(maxsize=None)
def graph_case(name):
    """-> rowPtr, colInd, reference labels, reference component count (made once, never modified)"""
    rp, ci = _graph(name)
    label, ncomp = cr.components(len(rp) - 1, rp, ci)
    return rp, ci, label, ncomp


# ---- device helpers --------------------------------------------------------------------------------------------------
def _device(rp, ci, v, dtype):
    m = len(rp) - 1
    return hs.CSR.from_arrays(rp, ci, v, m, m, dtype=dtype).toGpuCSR()


def _attractors(handle, rp, ci, v, dtype):
    d = _device(rp, ci, v, dtype)
    try:
        parent = hs.rmcl_attractors(d, handle)
        try:
            return hs.d2h(parent, d.rows, np.int32)
        finally:
            hs.dev_free(parent)
    finally:
        d.deviceDispose()


def _components(handle, rp, ci):
    d = _device(rp, ci, np.ones(len(ci), np.float32), np.float32)
    try:
        label, ncomp, rounds = hs.connected_components(d, handle)
        try:
            return hs.d2h(label, d.rows, np.int32), ncomp, rounds
        finally:
            hs.dev_free(label)
    finally:
        d.deviceDispose()


def _clusters_of_labels(handle, label):
    dl = hs.h2d(np.asarray(label, np.int32))
    try:
        cl = hs.labels_to_clusters(dl, len(label), handle)
        try:
            return (cl.k,) + cl.to_host()
        finally:
            cl.dispose()
    finally:
        hs.dev_free(dl)


def _assert_clusters(got, want, m):
    k, cluster, ptr, members = got
    wk, wcluster, wptr, wmembers = want[:4]
    assert k == wk and np.array_equal(cluster, wcluster) and np.array_equal(ptr, wptr) and np.array_equal(members, wmembers)
    assert len(ptr) == k + 1 and ptr[k] == m and ptr[0] == 0
    for c in range(k):                                            # members ascend inside a cluster
        assert np.all(np.diff(members[ptr[c]:ptr[c + 1]]) > 0)
    if k:                                                         # clusters ascend by their smallest member
        assert np.all(np.diff(members[ptr[:-1]]) > 0)


# ---- attractors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", [4, 16, 64])
def test_attractors_every_group_width(handle, G, dtype):
    rp, ci, v, want = attractor_case(G, dtype)
    got = _attractors(handle, rp, ci, v, dtype)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    for seed in (1, 2):                                           # any storage order: the same parents
        sci, sv = _shuffled(rp, ci, v, seed)
        assert np.array_equal(_attractors(handle, rp, sci, sv, dtype), want), seed
    assert np.array_equal(_attractors(handle, rp, ci, v, dtype), got)


def test_attractors_float64_does_not_pass_through_float(handle):
    rp, ci, v, want = attractor_case(16, np.float64)
    _, _, _, want32 = attractor_case(16, np.float32)
    assert not np.array_equal(want, want32)                       # the 2^-40 rows tell the two apart
    assert np.array_equal(_attractors(handle, rp, ci, v, np.float64), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attractors_smallest_matrices(handle, dtype):
    assert len(_attractors(handle, [0], [], [], dtype)) == 0
    assert _attractors(handle, [0, 0], [], [], dtype).tolist() == [0]
    assert _attractors(handle, [0, 1], [0], [0.5], dtype).tolist() == [0]
    assert _attractors(handle, [0, 2, 2, 3], [2, 1, 0], [0.5, 0.5, np.nan], dtype).tolist() == [1, 1, 2]


@pytest.mark.parametrize("dtype", DTYPES)
def test_attractors_refuse_a_column_outside_the_matrix(handle, dtype):
    for bad in (3, -1):
        with pytest.raises(hs.SpgemmError, match=ERR_INPUT):
            _attractors(handle, [0, 1, 2, 3], [0, bad, 1], [1.0, 1.0, 1.0], dtype)
    with pytest.raises(hs.SpgemmError, match=ERR_INPUT):
        _attractors(handle, [0, 2, 1, 3], [0, 1, 1], [1.0, 1.0, 1.0], dtype)   # rowPtr not monotone
    assert _attractors(handle, [0, 1, 2, 3], [0, 2, 1], [1.0, 1.0, 1.0], dtype).tolist() == [0, 2, 1]   # the handle still works


# ---- components ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_components_equal_the_union_find(handle, name):
    rp, ci, want, wncomp = graph_case(name)
    label, ncomp, rounds = _components(handle, rp, ci)
    print(f"{name}: m={len(rp) - 1} nnz={len(ci)} components={ncomp} rounds={rounds}")
    assert np.array_equal(label, want), np.nonzero(label != want)[0][:10]
    assert ncomp == wncomp == np.count_nonzero(label == np.arange(len(label)))
    assert 1 <= rounds < hs.CC_MAX_ROUNDS
    again = _components(handle, rp, ci)
    assert np.array_equal(again[0], label) and again[1] == ncomp


def test_components_known_counts(handle):
    assert graph_case("isolated")[3] == 1000 and graph_case("path")[3] == 1 and graph_case("star")[3] == 1
    assert graph_case("path_sorted")[3] == 1
    assert graph_case("cliques")[3] == 2 and graph_case("cliques_joined")[3] == 1 and graph_case("cycle_tails")[3] == 1
    label, ncomp, rounds = _components(handle, [0], [])
    assert len(label) == 0 and ncomp == 0 and rounds == 0


def test_components_refuse_bad_input(handle):
    with pytest.raises(hs.SpgemmError, match=ERR_INPUT):
        _components(handle, [0, 1, 2], [0, 2])
    with pytest.raises(hs.SpgemmError, match=ERR_INPUT):
        _components(handle, [0, 2, 1], [0, 1])
    assert _components(handle, [0, 1, 2], [1, 1])[0].tolist() == [0, 0]


# ---- labels to clusters ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_labels_to_clusters_equal_the_reference(handle, name):
    label = graph_case(name)[2]
    _assert_clusters(_clusters_of_labels(handle, label), cr.compact(label), len(label))


def test_labels_to_clusters_smallest_and_refusals(handle):
    assert _clusters_of_labels(handle, [])[0] == 0
    k, cluster, ptr, members = _clusters_of_labels(handle, [0])
    assert (k, cluster.tolist(), ptr.tolist(), members.tolist()) == (1, [0], [0, 1], [0])
    for bad in ([1, 1], [0, 0, 1], [0, -1], [0, 5], [0, 1, 2, 4, 4]):
        with pytest.raises(hs.SpgemmError, match=ERR_INPUT):
            _clusters_of_labels(handle, bad)
    assert _clusters_of_labels(handle, [0, 0, 2, 2, 0])[2].tolist() == [0, 3, 5]


# ---- end to end ------------------------------------------------------------------------------------------------------
def _rmcl_then_clusters(handle, Mt, iters):
    """-> (device clusters as host arrays, the flow matrix the device produced, downloaded)"""
    dM = to_hs(Mt).toGpuCSR()
    try:
        dOut = hs.gpuRmclIter_device(iters, dM, dM, handle)
    finally:
        dM.deviceDispose()
    try:
        cl = hs.rmcl_clusters(dOut, handle)
        try:
            got = (cl.k,) + cl.to_host()
        finally:
            cl.dispose()
        return got, dOut.toCpuCSR()
    finally:
        dOut.deviceDispose()


def _clusters_f64(handle, out):
    """the float64 twin on the same structure, values with bits a float cannot hold"""
    v = np.asarray(out.values, np.float64) * (1.0 + 2.0 ** -40)
    d = hs.CSR.from_arrays(out.rowPtr, out.colInd, v, out.rows, out.cols, dtype=np.float64).toGpuCSR()
    try:
        cl = hs.rmcl_clusters(d, handle)
        try:
            return (cl.k,) + cl.to_host(), cr.rmcl_clusters(out.rowPtr, out.colInd, v)
        finally:
            cl.dispose()
    finally:
        d.deviceDispose()


@pytest.mark.parametrize("iters", [1, 10])
def test_own_graph_file_to_clusters(handle, iters):
    Mt = po.load(os.path.join(DATA, "own_graph.snap"), isTrans=True, mode=1)
    got, out = _rmcl_then_clusters(handle, Mt, iters)
    _assert_clusters(got, cr.rmcl_clusters(out.rowPtr, out.colInd, out.values), Mt.rows)   # the same bits in: exact
    got64, want64 = _clusters_f64(handle, out)
    _assert_clusters(got64, want64, Mt.rows)


def test_planted_cliques_never_mix(handle):
    rng = np.random.default_rng(2024)
    sizes = rng.integers(3, 41, size=200)
    n = int(sizes.sum())
    ids = rng.permutation(n)                                       # scrambled ids
    clique_of = np.empty(n, np.int64)
    src, dst, at = [], [], 0
    for q, s in enumerate(sizes):
        mine = ids[at:at + s]
        clique_of[mine] = q
        a, b = _clique(mine)
        off = a != b
        src.append(a[off]); dst.append(b[off])
        at += s
    src, dst = np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32)
    Mt = po.rmcl_init(n, n, src, dst, np.ones(len(src), np.float32))
    got, out = _rmcl_then_clusters(handle, Mt, 10)
    _assert_clusters(got, cr.rmcl_clusters(out.rowPtr, out.colInd, out.values), n)
    k, cluster = got[0], got[1]
    # flow never leaves a block of a block-diagonal matrix: a cluster lies inside one clique
    assert len(np.unique(np.stack([cluster, clique_of]), axis=1)[0]) == k
    print(f"planted: {len(sizes)} cliques, {n} vertices, {k} clusters")
    got64, want64 = _clusters_f64(handle, out)
    _assert_clusters(got64, want64, n)


def test_cpp_mirror_prints_same():
    """tests/cpp/clusters_check.cc: own_graph.snap through rmclInit, gpuRmclIterDevice and gpuRmclClusters against a host
    union-find over the downloaded result"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "clusters.mk", "clusters_check.x"])
    out = subprocess.run([os.path.join(cpp, "clusters_check.x"), os.path.join(DATA, "own_graph.snap")], capture_output=True,
                         text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "Same" in lines and "Diffs" not in lines
