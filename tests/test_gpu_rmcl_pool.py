"""GPU (-m gpu): every pool block an R-MCL call takes comes back.  Each case runs its call once to warm the pool, frees
the outputs, records the cached bytes of the device, runs the same call again, frees the outputs, and expects the same
cached bytes: a block that is not released leaves the figure short (its replacement comes out of the cache) or makes
the pool grow (the replacement comes from the driver and is cached when it is released in turn)."""
import ctypes as C

import numpy as np
import pytest

from devcsr import _seasoned_pool, built_gpu, handle  # noqa: F401
from devcsr import start_graph as _graph
from devcsr import taken, twice
from helpers import po
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu
ENV = ("SPGEMM_RMCL_MAXP", "SPGEMM_RMCL_SYMBOLIC", "SPGEMM_RMCL_PACK")


@pytest.fixture(scope="module")
def graph():
    M0, dM = _graph(2)
    yield M0, dM
    dM.deviceDispose()


@pytest.fixture(scope="module")
def thin_graph():
    """the same with half the degree: no row of its first three iterations has more than 512 products"""
    M0, dM = _graph(1)
    yield M0, dM
    dM.deviceDispose()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def loop(handle, dM, iters):
    return taken(*hs.rmcl_iter_device_raw(handle, iters, dM.rows, dM.cols, dM.rowPtr, dM.colInd, dM.values, dM.nnz,
                                          dM.rowPtr, dM.colInd, dM.values, dM.nnz), dM.rows)


def step(handle, dA, dB):
    return taken(*hs.rmcl_expand_prune_raw(handle, dA.rowPtr, dA.colInd, dA.values, dA.nnz, dB.rowPtr, dB.colInd, dB.values,
                                           dB.nnz, dA.rows, dA.cols, dB.cols), dA.rows)


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("known_nnz", [False, True])
def test_prune(handle, graph, known_nnz):
    _, dM = graph
    dC = hs.gpuSpMMWrapper(dM, dM, handle)
    try:
        rp, _, _ = twice(lambda: taken(*hs.rmcl_prune_raw(handle, dC.rows, dC.rowPtr, dC.colInd, dC.values,
                                                          dC.nnz if known_nnz else None), dC.rows))
        assert 0 < rp[-1] < dC.nnz
    finally:
        dC.deviceDispose()


@pytest.mark.parametrize("symbolic", [False, True])
def test_fused_step(handle, graph, symbolic, monkeypatch):
    _, dM = graph
    if symbolic:
        monkeypatch.setenv("SPGEMM_RMCL_SYMBOLIC", "1")
    rp, _, _ = twice(lambda: step(handle, dM, dM))
    assert (handle.stats()["nnzC"] >= 0) == symbolic and rp[-1] > 0


@pytest.mark.parametrize("pack", [False, True])
def test_loop_three_iterations(handle, graph, pack, monkeypatch):
    _, dM = graph
    if pack:
        monkeypatch.setenv("SPGEMM_RMCL_PACK", "1")
    rp, _, _ = twice(lambda: loop(handle, dM, 3))
    assert rp[-1] > 0


def test_loop_zero_iterations(handle, graph):
    M0, dM = graph
    got = twice(lambda: loop(handle, dM, 0))
    assert same_bits(got, (M0.rowPtr, M0.colInd, M0.values))


def test_loop_gives_up_in_iteration_two(handle, graph, monkeypatch):
    """SPGEMM_RMCL_MAXP between the products of iterations 1 and 2: iteration 1 leaves Mt unpacked, iteration 2 packs it
    and runs SpGEMM + prune; a third iteration has fewer products than the bound and runs fused again, from a packed Mt"""
    M0, dM = graph
    rp, ci, v = loop(handle, dM, 1)
    M1 = po.CSRHost(rp, ci, v, M0.rows, M0.cols)
    P1, P2 = int(po.row_flops(M0, M0).sum()), int(po.row_flops(M0, M1).sum())
    assert P2 > P1
    monkeypatch.setenv("SPGEMM_RMCL_MAXP", str((P1 + P2) // 2))
    twice(lambda: loop(handle, dM, 2))
    assert handle.stats()["nnzC"] >= 0                                    # the last step counted its product: SpGEMM + prune
    twice(lambda: loop(handle, dM, 3))


def test_loop_after_a_forced_failure(handle, thin_graph):
    """The failed call gives every block back and leaves the handle usable: the next call returns the bits of the call
    before.  Two runs agree on bits where one wave sums a row, in a fixed order: rows of at most 512 products (longer
    rows are summed by the LDS atomics of four waves and differ in the last bit from run to run), hence the thin graph."""
    M0, dM = thin_graph
    cur = M0
    for it in range(3):
        assert po.row_flops(M0, cur).max() <= 512, f"iteration {it + 1} has a row for a four-wave kernel"
        cur = po.CSRHost(*loop(handle, dM, it + 1), M0.rows, M0.cols)
    want = loop(handle, dM, 3)
    before = hs.pool_cached_bytes(handle.device)
    handle.fail_next(1)
    o = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
    n = C.c_int(7)
    p = [C.c_void_p(x) for x in (dM.rowPtr, dM.colInd, dM.values)]
    rc = hs.lib().hip_gpuRmclIter_device(handle.ptr, 3, dM.rows, dM.cols, *p, dM.nnz, *p, dM.nnz,
                                         *[C.byref(x) for x in o], C.byref(n))
    assert rc != 0 and [x.value for x in o] == [None, None, None] and n.value == 0
    assert hs.pool_cached_bytes(handle.device) == before
    assert same_bits(loop(handle, dM, 3), want)
    assert hs.pool_cached_bytes(handle.device) == before


def test_step_without_rows_and_without_products(handle):
    def dev(rp, ci, rows, cols):
        return hs.CSR.from_arrays(np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.ones(len(ci), np.float32), rows,
                                  cols).toGpuCSR()

    none, A, B, B0 = dev([0], [], 0, 4), dev([0, 2, 2, 3], [0, 3, 1], 3, 4), dev([0, 1, 2, 2, 3], [0, 4, 2], 4, 5), dev([0] * 5, [], 4, 5)
    try:
        rp, ci, _ = twice(lambda: step(handle, none, B))                  # m == 0
        assert rp.tolist() == [0] and len(ci) == 0
        rp, ci, _ = twice(lambda: step(handle, A, B0))                    # P == 0
        assert rp.tolist() == [0, 0, 0, 0] and len(ci) == 0
    finally:
        for d in (none, A, B, B0):
            d.deviceDispose()


def test_sharded_job_two_shards_on_one_device(graph):
    M0, _ = graph
    Mt = hs.CSR.from_arrays(M0.rowPtr, M0.colInd, M0.values, M0.rows, M0.cols)
    g = hs.Group(2, devices=[0, 0], transport=hs.XCHG_PEER)

    def job():
        j = hs.ShardedRmcl(g, Mt, Mt)
        try:
            nnz = j.run(2)
            r = j.result(0)
        finally:
            j.close()
        assert r.nnz == nnz > 0

    try:
        twice(job)
    finally:
        g.close()
