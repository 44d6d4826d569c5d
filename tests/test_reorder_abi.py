"""CPU: the reorder entry points (hip_csr_permute, hip_csr_transpose, hip_permutation_transpose,
hip_csr_row_descending_permutation) check their arguments without a GPU, the Python mirror refuses a non-square PMPt and
a P of the wrong length before any device work, and the numpy restatement the GPU tests compare against
(tests/reorder_ref.py) is pinned to the reference: PM / MP through the identity of the reference's own test
(tests/CSR_test.cc:14-29, 41-61: PM(M,P) == Pmat * M, MP(M,Q) == M * Qmat), transpose through the loader's isTrans."""
import ctypes as C
import os

import numpy as np
import pytest

import reorder_ref as rr
from devcsr import built  # noqa: F401
from helpers import DATA, po, random_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

ERR_ARG = 2


# unlike devcsr._outs: null slots (these entry points must leave them null on an argument error)
def _outs():
    return [C.c_void_p(), C.c_void_p(), C.c_void_p()]


@pytest.mark.parametrize("name", ["hip_csr_permute", "hip_csr_permute_f64"])
def test_permute_argument_errors_do_not_need_a_gpu(name):
    fn = getattr(hs.lib(), name)
    o = _outs()
    refs = [C.byref(x) for x in o]
    one = C.c_void_p(8)                                     # a non-null "device pointer": never dereferenced
    for k in range(3):                                      # a null output
        a = list(refs)
        a[k] = None
        assert fn(None, 1, 1, 0, one, None, None, None, None, *a) == ERR_ARG
    assert fn(None, -1, 1, 0, one, None, None, None, None, *refs) == ERR_ARG
    assert fn(None, 1, -1, 0, one, None, None, None, None, *refs) == ERR_ARG
    assert fn(None, 1, 1, -1, one, None, None, None, None, *refs) == ERR_ARG
    assert fn(None, 1, 1, 3, one, None, one, None, None, *refs) == ERR_ARG      # nnz > 0, colInd null
    assert fn(None, 1, 1, 3, one, one, None, None, None, *refs) == ERR_ARG      # nnz > 0, values null
    assert fn(None, 1, 1, 3, None, one, one, None, None, *refs) == ERR_ARG      # rowPtr null
    assert all(x.value is None for x in o)
    assert hs.lib().spgemm_hip_last_error()


@pytest.mark.parametrize("name", ["hip_csr_transpose", "hip_csr_transpose_f64"])
def test_transpose_argument_errors_do_not_need_a_gpu(name):
    fn = getattr(hs.lib(), name)
    o = _outs()
    refs = [C.byref(x) for x in o]
    one = C.c_void_p(8)
    for k in range(3):
        a = list(refs)
        a[k] = None
        assert fn(None, 1, 1, 0, one, None, None, *a) == ERR_ARG
    assert fn(None, -1, 1, 0, one, None, None, *refs) == ERR_ARG
    assert fn(None, 1, -1, 0, one, None, None, *refs) == ERR_ARG
    assert fn(None, 1, 1, -1, one, None, None, *refs) == ERR_ARG
    assert fn(None, 1, 1, 3, one, None, one, *refs) == ERR_ARG
    assert fn(None, 1, 1, 3, one, one, None, *refs) == ERR_ARG
    assert fn(None, 1, 1, 3, None, one, one, *refs) == ERR_ARG
    assert all(x.value is None for x in o)


def test_permutation_helpers_argument_errors_do_not_need_a_gpu():
    L = hs.lib()
    one = C.c_void_p(8)
    assert L.hip_permutation_transpose(None, -1, one, one) == ERR_ARG
    assert L.hip_permutation_transpose(None, 4, None, one) == ERR_ARG
    assert L.hip_permutation_transpose(None, 4, one, None) == ERR_ARG
    out = C.c_void_p()
    assert L.hip_csr_row_descending_permutation(None, 3, one, None) == ERR_ARG
    assert L.hip_csr_row_descending_permutation(None, -3, one, C.byref(out)) == ERR_ARG
    assert L.hip_csr_row_descending_permutation(None, 3, None, C.byref(out)) == ERR_ARG
    assert out.value is None


def test_mirror_refuses_bad_shapes_before_device_work():
    # device CSRs with no memory behind them: anything that reached the device would fail differently
    for dt in (np.float32, np.float64):
        rect = hs.CSR(None, None, None, 3, 4, 0, on_device=True, dtype=dt)
        with pytest.raises(hs.SpgemmError, match="square"):
            rect.PMPt(np.arange(3, dtype=np.int32))
        with pytest.raises(hs.SpgemmError, match="square"):
            rect.PtMP(np.arange(3, dtype=np.int32))
        sq = hs.CSR(None, None, None, 4, 4, 0, on_device=True, dtype=dt)
        for call in (sq.PM, sq.MP, sq.PMPt, sq.PtMP):
            with pytest.raises(hs.SpgemmError, match="entries"):
                call(np.arange(3, dtype=np.int32))
        with pytest.raises(hs.SpgemmError, match="entries"):
            rect.PM(np.arange(4, dtype=np.int32))           # PM takes a row permutation: 3 entries
        with pytest.raises(hs.SpgemmError, match="entries"):
            rect.MP(np.arange(3, dtype=np.int32))           # MP a column permutation: 4 entries


def _product(A, B):
    a = po.CSRHost(A.rowPtr, A.colInd, A.values, A.rows, A.cols)
    b = po.CSRHost(B.rowPtr, B.colInd, B.values, B.rows, B.cols)
    return po.ref_spmm(a, b) if po.have_ref() else po.sequential_spmm(a, b)


@pytest.mark.parametrize("rows,cols", [(37, 53), (257, 100)])
def test_restatement_satisfies_the_reference_identity(rows, cols):
    M = random_csr(rows, cols, 0.15, 100 + rows, sorted_rows=False)
    rng = np.random.default_rng(rows)
    P, Q = rng.permutation(rows).astype(np.int32), rng.permutation(cols).astype(np.int32)
    # every product is one term times 1.0: bit-exact
    assert rr.same_bits(rr.sort_rows(rr.PM(M, P)), rr.sort_rows(_product(rr.perm_matrix(P), M)))
    assert rr.same_bits(rr.sort_rows(rr.MP(M, Q)), rr.sort_rows(_product(M, rr.perm_matrix(Q))))
    # in-row order: PM keeps the source row's storage order, MP renames in place
    r = 5
    s, e = M.rowPtr[P[r]], M.rowPtr[P[r] + 1]
    pm = rr.PM(M, P)
    assert np.array_equal(pm.colInd[pm.rowPtr[r]:pm.rowPtr[r + 1]], M.colInd[s:e])
    assert np.array_equal(rr.MP(M, Q).colInd, Q[M.colInd])


@pytest.mark.parametrize("n", [37, 257])
def test_restatement_ptmp_undoes_pmpt(n):
    M = random_csr(n, n, 0.1, 7 + n, sorted_rows=False)
    P = np.random.default_rng(n).permutation(n).astype(np.int32)
    assert rr.same_bits(rr.PtMP(rr.PMPt(M, P), P), M)
    Pt = rr.permutation_transpose(P)
    assert np.array_equal(Pt[P], np.arange(n)) and np.array_equal(P[Pt], np.arange(n))


def test_restatement_row_descending_is_stable():
    rp = np.array([0, 2, 2, 7, 9, 9, 14], np.int32)          # lengths 2 0 5 2 0 5
    assert list(rr.row_descending(rp)) == [2, 5, 0, 3, 1, 4]


@pytest.mark.parametrize("name", ["own_graph.snap", "own_dups.mtx", "test2.mtx"])
def test_restatement_transpose_matches_the_transposed_load(name):
    path = os.path.join(DATA, name)
    M, Mt = po.load(path, isTrans=False), po.load(path, isTrans=True)
    assert M.nnz > 0
    assert rr.same_bits(rr.transpose(M), Mt)
    assert rr.same_bits(rr.transpose(rr.transpose(M)), M)


def test_device_synchronize_is_exported():
    assert "spgemm_hip_device_synchronize" in hs.EXPORTS
    assert callable(hs.lib().spgemm_hip_device_synchronize) and callable(hs.device_synchronize)
