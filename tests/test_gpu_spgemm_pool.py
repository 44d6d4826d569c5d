"""GPU (-m gpu): every pool block an SpGEMM call takes comes back -- the five routes of hip_gpuSpMM, the double
product, the two-phase ABI, the classification calls and the host API.  The protocol is test_gpu_rmcl_pool.py's: a
seasoned pool, then each case runs its call once to warm, frees the outputs, records the cached bytes of the device, runs
the same call again, frees the outputs and expects the same cached bytes, exactly."""
import ctypes as C

import numpy as np
import pytest

from devcsr import _seasoned_pool, built_gpu, handle  # noqa: F401
from devcsr import start_graph, take, taken, to_hs, twice, typed_plain
from helpers import canonical_arrays, po
from sparse_matrix_with_flops_amd import hipspgemm as hs
from test_gpu_wbatch import _two_entry_rows, handle_with

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def graph():
    """the 2000-node R-MCL start graph: host, device, and its square by the oracle"""
    M0, dM = start_graph(2)
    yield M0, dM, po.omp_spmm(M0, M0)
    dM.deviceDispose()


def squared_256():
    """256 x 256, 32 random columns per row: P = 262 144 products for at most 65 536 entries of the square"""
    rng = np.random.default_rng(3)
    ci = np.concatenate([np.sort(rng.choice(256, 32, replace=False)) for _ in range(256)])
    return po.CSRHost((np.arange(257) * 32).astype(np.int32), ci.astype(np.int32), (rng.random(len(ci)) + 0.25).astype(np.float32), 256, 256)


def args(d):
    return d.rowPtr, d.colInd, d.values, d.nnz


def product(handle, dA, dB, dtype=np.float32):
    """hip_gpuSpMM[_f64] -> (rowPtr, colInd, values, bytes the three arrays of C occupied in the pool); C is freed"""
    raw = hs.gpu_spmm_raw_f64 if np.dtype(dtype) == np.float64 else hs.gpu_spmm_raw
    i, j, v, n = raw(handle, *args(dA), *args(dB), dA.rows, dA.cols, dB.cols)
    mid = hs.pool_cached_bytes(handle.device)
    out = taken(i, j, v, n, dA.rows, dtype)
    return out + (hs.pool_cached_bytes(handle.device) - mid,)


def same_structure(rp, ci, want):
    """rowPtr and per-row sorted columns equal the oracle's"""
    wc, _ = canonical_arrays(want.rowPtr, want.colInd, want.values)
    gc, _ = canonical_arrays(rp, ci, np.zeros(len(ci), np.float32))
    return np.array_equal(rp, want.rowPtr) and np.array_equal(gc, wc)


def test_route_1_one_shot(handle, graph):
    """C sized by P.  The graph's square compresses (nnz(C) / P = 0.62), so a handle that remembers it sizes the next one
    exactly: a different product in between keeps every call of the graph's on route 1."""
    M0, dM, want = graph
    S = squared_256()
    P = int(po.row_flops(M0, M0).sum())
    dS = to_hs(S).toGpuCSR()
    try:
        rp, ci, _, held = twice(lambda: (product(handle, dS, dS), product(handle, dM, dM))[1])
    finally:
        dS.deviceDispose()
    assert same_structure(rp, ci, want)
    assert held >= 8 * P                                                  # colInd and values of P entries each: route 1


def test_route_4_exact_allocation_of_a_compressive_product(handle):
    S = squared_256()
    want = po.omp_spmm(S, S)
    P = int(po.row_flops(S, S).sum())
    assert P == 262144 and want.nnz <= 0.25 * P                           # below the handle's 0.75 rule
    dS = to_hs(S).toGpuCSR()
    try:
        product(handle, dS, dS)                                           # sized by P unless the handle has seen it
        product(handle, dS, dS)                                           # from here on: the exact route
        rp, ci, _, held = twice(lambda: product(handle, dS, dS))
    finally:
        dS.deviceDispose()
    assert same_structure(rp, ci, want)
    # exact: 8 nnz(C) + 4 (m + 1) bytes, <= 2 P + 1 KiB, in blocks of the ladder (a step is 6 %: well under twice that);
    # sized by P the two arrays alone are 8 P bytes
    assert held < 4 * P, f"C held {held} bytes: values sized by P = {P}, not by nnz(C) = {want.nnz}?"


def test_route_5_no_rows(handle):
    def dev(rp, ci, rows, cols):
        return hs.CSR.from_arrays(np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.ones(len(ci), np.float32), rows, cols).toGpuCSR()

    none, B = dev([0], [], 0, 4), dev([0, 1, 2, 2, 3], [0, 4, 2], 4, 5)
    try:
        rp, ci, _, _ = twice(lambda: product(handle, none, B))
        assert rp.tolist() == [0] and len(ci) == 0
    finally:
        none.deviceDispose()
        B.deviceDispose()


def classified_product(handle, dM):
    """hip_gpuFlopsClassify + hip_sgpuSpMM; the classification arrays are freed with the product"""
    hv, _, ids, fl, _ = hs.gpuFlopsClassify(dM, dM, handle)
    try:
        return take(hs.sgpuSpMMWrapper(dM, dM, ids, hv, fl, handle))
    finally:
        hs.dev_free(ids)
        hs.dev_free(fl)


def test_route_5_caller_classification(handle, graph):
    _, dM, want = graph
    got = twice(lambda: classified_product(handle, dM))
    assert same_structure(got.rowPtr, got.colInd, want)


def test_route_2_capacity_redo(handle, monkeypatch):
    """test_gpu_wbatch.py::test_one_pass_capacity_guard's pair on a one-pass handle: the first product compresses, the
    second has its shape and product count and twice the entries, finds C sized by the first and is redone two-phase"""
    h = handle_with(monkeypatch, 2)
    m = 50000
    (A1, B1), (A2, B2) = _two_entry_rows(m, same=True), _two_entry_rows(m, same=False)
    want1, want2 = po.omp_spmm(A1, B1), po.omp_spmm(A2, B2)
    assert want1.nnz == 4 * m and want2.nnz == 8 * m
    dev = [to_hs(M).toGpuCSR() for M in (A1, B1, A2, B2)]
    try:
        first, second = twice(lambda: (product(h, dev[0], dev[1]), product(h, dev[2], dev[3])), h.device)
    finally:
        for d in dev:
            d.deviceDispose()
        h.close()                                                         # (the module's handle keeps the pool)
    assert same_structure(first[0], first[1], want1) and same_structure(second[0], second[1], want2)


def wide_row_operands(case):
    """double products whose only row lands in bin 8: `probe` 5000 products into 300 columns (the probe words are
    allocated), `table` 70 000 entries, more than the 16 LDS passes hold (a device-memory table is)"""
    if case == "probe":
        A = po.CSRHost(np.r_[0, np.full(300, 100)].astype(np.int32), np.arange(100, dtype=np.int32), np.ones(100, np.float32), 300, 300)
        cols = (np.arange(300)[:, None] * 7 + np.arange(50)[None, :] * 6) % 300
        B = po.CSRHost((np.arange(301) * 50).astype(np.int32), cols.astype(np.int32).ravel(), np.full(15000, 0.5, np.float32), 300, 300)
        return A, B, 5000
    A = po.CSRHost(np.array([0, 700], np.int32), np.arange(700, dtype=np.int32), np.ones(700, np.float32), 1, 700)
    B = po.CSRHost((np.arange(701) * 100).astype(np.int32), np.arange(70000, dtype=np.int32), np.full(70000, 0.5, np.float32), 700, 70000)
    return A, B, 70000


@pytest.mark.parametrize("case", ["graph", "probe", "table"])
def test_double_product(handle, graph, case):
    if case == "graph":
        M0, _, want = graph
        A = B = M0
    else:
        A, B, P = wide_row_operands(case)
        want = po.omp_spmm(A, B)
        assert po.row_flops(A, B).max() == P > 4096 and (case == "probe" or want.nnz == 70000 > 16 * 4096)
    dA, dB = typed_plain(A, np.float64).toGpuCSR(), typed_plain(B, np.float64).toGpuCSR()
    try:
        rp, ci, _, _ = twice(lambda: product(handle, dA, dB, np.float64))
    finally:
        dA.deviceDispose()
        dB.deviceDispose()
    assert same_structure(rp, ci, want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_phase_abi_into_caller_buffers(handle, graph, dtype):
    M0, _, want = graph
    dM = typed_plain(M0, dtype).toGpuCSR()
    numeric = hs.spgemm_numeric_raw_f64 if dtype == np.float64 else hs.spgemm_numeric_raw
    shape = (dM.rows, dM.cols, dM.cols)

    def call():
        ic = hs.dev_alloc(4 * (dM.rows + 1))
        nnz = hs.spgemm_symbolic_raw(handle, dM.rowPtr, dM.colInd, dM.nnz, dM.rowPtr, dM.colInd, dM.nnz, *shape, ic)
        jc, cv = hs.dev_alloc(4 * nnz), hs.dev_alloc(np.dtype(dtype).itemsize * nnz)
        numeric(handle, *args(dM), *args(dM), *shape, ic, jc, cv)
        return taken(ic, jc, cv, nnz, dM.rows, dtype)

    try:
        rp, ci, _ = twice(call)
    finally:
        dM.deviceDispose()
    assert same_structure(rp, ci, want)


def test_classification_calls(handle, graph):
    M0, dM, _ = graph
    flops = po.row_flops(M0, M0)

    def row_flops():
        out = hs.dev_alloc(4 * dM.rows)
        total = hs.row_flops_raw(handle, dM.rowPtr, dM.colInd, dM.rowPtr, dM.rows, out)
        got = hs.d2h(out, dM.rows, np.int32)
        hs.dev_free(out)
        return total, got

    def classify():
        hv, hv_len, ids, fl, total = hs.gpuFlopsClassify(dM, dM, handle)
        rows = np.sort(hs.d2h(ids, dM.rows, np.int32))
        hs.dev_free(ids)
        hs.dev_free(fl)
        return total, rows, hv[hv_len - 1]

    total, got = twice(row_flops)
    assert total == int(flops.sum()) and np.array_equal(got, flops)
    total, rows, last = twice(classify)
    assert total == int(flops.sum()) and np.array_equal(rows, np.arange(dM.rows)) and last == dM.rows + 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_api(graph, dtype):
    M0, _, want = graph
    A = typed_plain(M0, dtype)
    got = twice(lambda: A.hip_spmm(A))
    assert got.values.dtype == dtype and same_structure(got.rowPtr, got.colInd, want)


def test_forced_failure_gives_every_block_back(handle, graph):
    """spgemm_hip_debug_fail_next fails the next symbolic phase, which hip_gpuSpMM_f64 and hip_sgpuSpMM both reach with
    C's rowPtr allocated: the call returns non-zero with cleared outputs and an unchanged pool, and the handle works on"""
    M0, dM, want = graph
    d64 = typed_plain(M0, np.float64).toGpuCSR()
    dev = handle.device
    shape = (dM.rows, dM.cols, dM.cols)

    def failed(entry, *operands):
        o, n = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)], C.c_int(7)
        handle.fail_next(1)
        rc = entry(handle.ptr, *operands, *[C.byref(x) for x in o], C.byref(n))
        return rc != 0 and [x.value for x in o] == [None, None, None] and n.value == 0

    def inputs(d):
        return [C.c_void_p(x) for x in (d.rowPtr, d.colInd, d.values)] + [d.nnz]

    try:
        product(handle, d64, d64, np.float64)
        before = hs.pool_cached_bytes(dev)
        assert failed(hs.lib().hip_gpuSpMM_f64, *inputs(d64), *inputs(d64), *shape)
        assert hs.pool_cached_bytes(dev) == before
        rp, ci, _, _ = product(handle, d64, d64, np.float64)
        assert same_structure(rp, ci, want) and hs.pool_cached_bytes(dev) == before

        classified_product(handle, dM)
        hv, _, ids, fl, _ = hs.gpuFlopsClassify(dM, dM, handle)
        try:
            before = hs.pool_cached_bytes(dev)
            assert failed(hs.lib().hip_sgpuSpMM, *inputs(dM), *inputs(dM), *shape, C.c_void_p(ids), (C.c_int * hs.HV_LEN)(*hv), C.c_void_p(fl))
            assert hs.pool_cached_bytes(dev) == before
            got = take(hs.sgpuSpMMWrapper(dM, dM, ids, hv, fl, handle))
            assert same_structure(got.rowPtr, got.colInd, want) and hs.pool_cached_bytes(dev) == before
        finally:
            hs.dev_free(ids)
            hs.dev_free(fl)
    finally:
        d64.deviceDispose()
