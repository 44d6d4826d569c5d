"""GPU (-m gpu): the R-MCL loop with a row cap, hip_gpuRmclIter_device_topk / _f64 (every iteration is
hip_rmcl_expand_prune, then hip_csr_row_topk with SPGEMM_TOPK_NORMALISE), and the C++ check of the selection.

Product values vary within rounding between the device and the oracle, and ties at the cut are the normal case (rmclInit
rows are all 1/deg, clique products are all equal): no test here assumes a gap between the k-th and the (k+1)-th value, and
no row is left out of a check.  1e-5 is the tolerance the multi-iteration loop tests of the uncapped loop use."""
import functools
import os
import subprocess

import numpy as np
import pytest

from devcsr import built_gpu, handle  # noqa: F401
from devcsr import _graph, take, to_hs
from helpers import DATA, ROOT, assert_rmcl_step, po
from sparse_matrix_with_flops_amd import hipspgemm as hs
import clusters_ref as cr

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _host(dev):
    out = take(dev)
    return po.CSRHost(out.rowPtr, out.colInd, out.values, out.rows, out.cols)


def _steps(handle, Mgt, k, steps):
    """the capped loop one iteration per call: yields (i, Mt_i as downloaded, Mt_i+1 as downloaded, iter_nnz, iter_cut)"""
    dG = to_hs(Mgt).toGpuCSR()
    cur_dev, cur = dG, Mgt
    try:
        for i in range(steps):
            nxt_dev, inz, icut = hs.gpuRmclIterTopK_device(1, k, dG, cur_dev, handle)
            if cur_dev is not dG:
                cur_dev.deviceDispose()
            cur_dev = nxt_dev
            nxt = cur_dev.toCpuCSR()
            nxt = po.CSRHost(nxt.rowPtr, nxt.colInd, nxt.values, nxt.rows, nxt.cols)
            assert inz == [nxt.nnz] and len(icut) == 1
            yield i, cur, nxt, inz[0], icut[0]
            cur = nxt
    finally:
        if cur_dev is not dG:
            cur_dev.deviceDispose()
        dG.deviceDispose()


def test_one_step_at_a_time_against_the_oracle_step(handle):
    """Every step from the device's own previous output.  With t the oracle's k-th largest value of a row: every kept
    column has an oracle value >= t (1 - 1e-5), every oracle entry above t (1 + 1e-5) is kept, the row is min(len, k) long,
    and the values are the oracle's, renormalised over the columns the device kept, within 1e-5."""
    k = 16
    Mgt = _graph(3000, 41)
    cut_rows = 0
    for i, prev, got, _, icut in _steps(handle, Mgt, k, 3):
        want = po.rmcl_iters(Mgt, prev, 1)
        assert np.array_equal(np.diff(got.rowPtr), np.minimum(np.diff(want.rowPtr), k)), f"step {i}: row lengths"
        cut_rows += icut
        for r in range(Mgt.rows):
            wc, wv = want.colInd[want.rowPtr[r]:want.rowPtr[r + 1]], want.values[want.rowPtr[r]:want.rowPtr[r + 1]].astype(np.float64)
            gc, gv = got.colInd[got.rowPtr[r]:got.rowPtr[r + 1]], got.values[got.rowPtr[r]:got.rowPtr[r + 1]].astype(np.float64)
            if len(wc) == 0:
                continue
            order = np.argsort(wc, kind="stable")
            at = np.searchsorted(wc[order], gc)
            assert np.all(at < len(wc)) and np.array_equal(wc[order][at], gc), f"step {i} row {r}: a kept column the oracle has not"
            assert len(np.unique(gc)) == len(gc), f"step {i} row {r}: a column kept twice"
            oracle_of_kept = wv[order][at]
            t = np.sort(wv)[::-1][k - 1] if len(wv) > k else -np.inf
            assert np.all(oracle_of_kept >= t * (1 - TOL)), f"step {i} row {r}: kept below the cut"
            must = wc[wv > t * (1 + TOL)]
            assert np.isin(must, gc).all(), f"step {i} row {r}: an entry above the cut is missing"
            scale = oracle_of_kept.sum() if len(wv) > k else 1.0
            assert np.allclose(gv, oracle_of_kept / scale, rtol=TOL, atol=0), f"step {i} row {r}: values"
    assert cut_rows > 0


def test_three_iterations_in_one_call(handle):
    k = 16
    Mgt = _graph(3000, 43)
    dG = to_hs(Mgt).toGpuCSR()
    try:
        dOut, inz, icut = hs.gpuRmclIterTopK_device(3, k, dG, dG, handle)
        onnz = dOut.nnz
        out = _host(dOut)
    finally:
        dG.deviceDispose()
    lens = np.diff(out.rowPtr)
    assert lens.max() <= k and lens.min() >= 1
    sums = np.add.reduceat(out.values.astype(np.float64), out.rowPtr[:-1])
    assert np.allclose(sums, 1.0, rtol=0, atol=TOL)
    assert len(inz) == 3 and len(icut) == 3 and inz[-1] == onnz == out.nnz and icut[0] > 0
    # zero iterations: a copy of Mt, nothing reported
    dG = to_hs(Mgt).toGpuCSR()
    try:
        dSame, inz0, icut0 = hs.gpuRmclIterTopK_device(0, k, dG, dG, handle)
        same = _host(dSame)
    finally:
        dG.deviceDispose()
    assert inz0 == [] and icut0 == []
    assert np.array_equal(same.rowPtr, Mgt.rowPtr) and np.array_equal(same.colInd, Mgt.colInd)
    assert same.values.tobytes() == np.ascontiguousarray(Mgt.values, np.float32).tobytes()


def test_a_cap_no_row_reaches_is_the_uncapped_loop(handle):
    """k >= cols: nothing is cut, and every step agrees with the oracle under the comparison the uncapped loops are held
    to (test_fused_and_two_step_loops_agree: helpers.assert_rmcl_step)"""
    Mgt = _graph(3000, 47)
    for k in (Mgt.cols, 2 ** 31 - 1):
        for i, prev, got, _, icut in _steps(handle, Mgt, k, 3):
            assert icut == 0
            assert_rmcl_step(got, Mgt, prev, what=f"k={k} iteration {i + 1}")
    dG = to_hs(Mgt).toGpuCSR()
    try:
        dOut, inz, icut = hs.gpuRmclIterTopK_device(3, Mgt.cols, dG, dG, handle)
        dRef = hs.gpuRmclIter_device(3, dG, dG, handle)
        out, ref = _host(dOut), _host(dRef)
    finally:
        dG.deviceDispose()
    assert icut == [0, 0, 0] and inz[-1] == out.nnz
    assert abs(out.nnz - ref.nnz) <= 0.001 * ref.nnz                    # (threshold ties aside, the same matrix)


# ---- planted cliques -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planted():
    """60 cliques of 3 to 40 vertices with scrambled ids and n / 4 noise edges between cliques -> (clique of every vertex,
    the R-MCL start matrix).  A numpy restatement of the capped loop (the oracle step, then topk_ref with normalise, ten
    times) gives exactly the cliques on this graph at k = 8, k = 16 and uncapped."""
    rng = np.random.default_rng(2024)
    sizes = rng.integers(3, 41, size=60)
    n = int(sizes.sum())
    ids = rng.permutation(n)
    clique_of = np.empty(n, np.int64)
    src, dst, at = [], [], 0
    for q, s in enumerate(sizes):
        mine = ids[at:at + s]
        clique_of[mine] = q
        a, b = np.repeat(mine, s), np.tile(mine, s)
        src.append(a[a != b]); dst.append(b[a != b])
        at += s
    u, v = rng.integers(0, n, n // 4), rng.integers(0, n, n // 4)
    across = clique_of[u] != clique_of[v]
    src += [u[across], v[across]]; dst += [v[across], u[across]]
    key = np.unique(np.concatenate(src).astype(np.int64) * n + np.concatenate(dst))
    src, dst = (key // n).astype(np.int32), (key % n).astype(np.int32)
    return clique_of, po.rmcl_init(n, n, src, dst, np.ones(len(src), np.float32))


def _assert_exactly_the_cliques(handle, dOut, clique_of):
    cl = hs.rmcl_clusters(dOut, handle)
    try:
        cluster = cl.to_host()[0]
        k = cl.k
    finally:
        cl.dispose()
    ncliques = len(np.unique(clique_of))
    assert k == ncliques and len(np.unique(np.stack([cluster, clique_of]), axis=1)[0]) == ncliques


@pytest.mark.parametrize("k", [8, 16])
def test_planted_cliques_are_the_clusters(handle, k):
    clique_of, Mgt = _planted()
    dG = to_hs(Mgt).toGpuCSR()
    try:
        dOut, inz, icut = hs.gpuRmclIterTopK_device(10, k, dG, dG, handle)
    finally:
        dG.deviceDispose()
    try:
        assert icut[0] > 0 and inz[-1] == dOut.nnz
        _assert_exactly_the_cliques(handle, dOut, clique_of)
        out = dOut.toCpuCSR()
        assert np.diff(out.rowPtr).max() <= k
        assert cr.rmcl_clusters(out.rowPtr, out.colInd, out.values)[0] == len(np.unique(clique_of))
    finally:
        dOut.deviceDispose()


def test_double_twin_on_the_planted_cliques(handle):
    clique_of, Mgt = _planted()
    k = 8
    dG = hs.CSR.from_arrays(Mgt.rowPtr, Mgt.colInd, np.asarray(Mgt.values, np.float64), Mgt.rows, Mgt.cols,
                            dtype=np.float64).toGpuCSR()
    try:
        dOut, inz, icut = hs.gpuRmclIterTopK_device(10, k, dG, dG, handle)
    finally:
        dG.deviceDispose()
    try:
        assert dOut.dtype == np.float64 and icut[0] > 0 and inz[-1] == dOut.nnz
        _assert_exactly_the_cliques(handle, dOut, clique_of)
        out = dOut.toCpuCSR()
        lens = np.diff(out.rowPtr)
        assert lens.max() <= k and out.values.dtype == np.float64
        assert np.allclose(np.add.reduceat(out.values, out.rowPtr[:-1]), 1.0, rtol=0, atol=1e-12)
    finally:
        dOut.deviceDispose()


def test_cpp_mirror_prints_same():
    """tests/cpp/topk_check.cc: own_graph.snap through rmclInit, one product on the device, CSR::gpuRowTopK at k = 1, 3, 64
    against a host std::stable_sort on the downloaded product: the same bits in, so bit-equal out"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "topk.mk", "topk_check.x"])
    out = subprocess.run([os.path.join(cpp, "topk_check.x"), os.path.join(DATA, "own_graph.snap")], capture_output=True,
                         text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "Same" in lines and "Diffs" not in lines
