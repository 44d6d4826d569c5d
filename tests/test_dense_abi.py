"""CPU: the dense matrix entry points (hip_csr_to_dense, hip_dense_to_csr, hip_dense_gemm and their _f64 twins) check their
arguments without a GPU, the Python class refuses a shape or dtype mismatch before any device work, and the restatement the
GPU tests compare against (tests/dense_ref.py) is pinned on values written out below."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dense_ref as dr
import reorder_ref as rr
from devcsr import built  # noqa: F401
from devcsr import _outs
from helpers import GOLDEN
from sparse_matrix_with_flops_amd import hipspgemm as hs

ERR_ARG = 2
TWINS = ["", "_f64"]
ONE = C.c_void_p(8)
FAR = C.c_void_p(1 << 40)


def kat():
    with open(os.path.join(GOLDEN, "dense_kat.json")) as f:
        return json.load(f)


# ---- the restatement, by hand ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_on_the_known_answer(dtype):
    k = kat()
    D = np.array(k["dense"], dtype).reshape(k["rows"], k["cols"])
    A = dr.to_csr(D)
    assert A.rowPtr.tolist() == [0, 2, 3, 5, 6, 9] == k["expected"]["rowPtr"]
    assert A.colInd.tolist() == [0, 1, 2, 1, 5, 4, 0, 3, 5] == k["expected"]["colInd"]
    assert A.values.tolist() == [1, 2, 3, 4, 5, 2, 3, 1, 8] == k["expected"]["values"] and A.values.dtype == dtype
    back = dr.to_dense(A)
    assert back.dtype == dtype and back.tobytes() == D.tobytes()


def test_restatement_last_of_a_repeated_column_wins():
    # row 0: (2, 1.0) (0, 2.0) (2, 3.0); row 1: (1, 4.0) (1, 5.0) (1, 6.0)
    A = rr.Host([0, 3, 6], [2, 0, 2, 1, 1, 1], np.array([1, 2, 3, 4, 5, 6], np.float32), 2, 3)
    assert dr.to_dense(A).tolist() == [[2, 0, 3], [0, 6, 0]]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_rules_on_the_special_values(dtype):
    t = np.dtype(dtype).type
    at = t(1e-8)
    up = np.nextafter(at, t(1))
    if dtype == np.float32:
        assert float(at) == 9.99999993922529e-09 < 1e-8 < float(up)          # float(1e-8) is below the double 1e-8
    D = np.array([[-1, np.nan, at, up, 0.0, -0.0]], dtype)
    ref = dr.to_csr(D, dr.KEEP_REFERENCE, 1e-8)
    # negative: dropped; NaN: kept (NaN < tol is false); 1e-8: dropped as float (kept as double: not below itself);
    # the next number up: kept; +0 and -0: dropped
    assert ref.colInd.tolist() == ([1, 3] if dtype == np.float32 else [1, 2, 3])
    assert ref.values.tobytes() == D[0, ref.colInd].tobytes()
    ab = dr.to_csr(D, dr.KEEP_ABS, 1e-8)
    # |-1| kept; NaN dropped; float(1e-8) not above 1e-8, nor is the double 1e-8; the next up kept; zeros dropped
    assert ab.colInd.tolist() == [0, 3] and ab.rowPtr.tolist() == [0, 2]
    assert dr.to_csr(D, dr.KEEP_ABS, 0.0).colInd.tolist() == [0, 2, 3]
    assert dr.to_csr(D, dr.KEEP_REFERENCE, 0.0).colInd.tolist() == [1, 2, 3, 4, 5]   # -0.0 < 0 is false: both zeros stay


# ---- argument errors: no device is touched (the "device pointers" are never dereferenced) ----------------------------
@pytest.mark.parametrize("twin", TWINS)
def test_csr_to_dense_argument_errors_do_not_need_a_gpu(twin):
    fn = getattr(hs.lib(), "hip_csr_to_dense" + twin)

    def call(m=4, n=4, nnz=0, IA=ONE, JA=None, A=None, D=ONE, ld=4):
        return fn(None, m, n, nnz, IA, JA, A, D, ld)

    assert call(m=-1) == ERR_ARG and call(n=-1) == ERR_ARG and call(nnz=-1) == ERR_ARG
    assert call(IA=None) == ERR_ARG and call(D=None) == ERR_ARG
    assert call(nnz=3, JA=None, A=ONE) == ERR_ARG and call(nnz=3, JA=ONE, A=None) == ERR_ARG
    assert call(m=0, nnz=3, JA=ONE, A=ONE) == ERR_ARG           # entries in a matrix without rows
    assert call(ld=3) == ERR_ARG and call(ld=-1) == ERR_ARG and call(ld=-2 ** 40) == ERR_ARG
    assert hs.lib().spgemm_hip_last_error()


@pytest.mark.parametrize("twin", TWINS)
def test_dense_to_csr_argument_errors_do_not_need_a_gpu(twin):
    fn = getattr(hs.lib(), "hip_dense_to_csr" + twin)
    nnzC = C.c_int(7)

    def call(m=4, n=4, D=ONE, ld=4, rule=0, tol=1e-8, outs=None, count=C.byref(nnzC)):
        o = outs if outs is not None else [C.byref(x) for x in _outs()]
        return fn(None, m, n, D, ld, rule, tol, *o, count)

    for k in range(3):
        o = [C.byref(x) for x in _outs()]
        o[k] = None
        assert call(outs=o) == ERR_ARG                          # a null output
    assert call(count=None) == ERR_ARG
    assert call(m=-1) == ERR_ARG and call(n=-1) == ERR_ARG and call(D=None) == ERR_ARG
    assert call(ld=3) == ERR_ARG and call(ld=-1) == ERR_ARG
    assert call(rule=2) == ERR_ARG and call(rule=-1) == ERR_ARG
    assert call(tol=-1e-30) == ERR_ARG and call(tol=float("nan")) == ERR_ARG and call(tol=float("-inf")) == ERR_ARG
    assert hs.lib().spgemm_hip_last_error()
    outs = _outs()
    assert call(rule=7, outs=[C.byref(x) for x in outs]) == ERR_ARG
    assert [x.value for x in outs] == [None, None, None] and nnzC.value == 0


@pytest.mark.parametrize("twin", TWINS)
def test_dense_gemm_argument_errors_do_not_need_a_gpu(twin):
    fn = getattr(hs.lib(), "hip_dense_gemm" + twin)
    size = 8 if twin else 4
    a, b, c = 1 << 40, 1 << 41, 1 << 42

    def call(m=4, n=5, k=6, A=a, lda=6, B=b, ldb=5, Cd=c, ldc=5):
        return fn(None, m, n, k, C.c_void_p(A) if A else None, lda, C.c_void_p(B) if B else None, ldb,
                  C.c_void_p(Cd) if Cd else None, ldc)

    assert call(m=-1) == ERR_ARG and call(n=-1) == ERR_ARG and call(k=-1) == ERR_ARG
    assert call(A=None) == ERR_ARG and call(B=None) == ERR_ARG and call(Cd=None) == ERR_ARG
    assert call(lda=5) == ERR_ARG and call(ldb=4) == ERR_ARG and call(ldc=4) == ERR_ARG and call(lda=-1) == ERR_ARG
    # C against A (4 x 6, lda 6: 24 elements) and against B (6 x 5, ldb 5: 30 elements), by address range
    assert call(Cd=a) == ERR_ARG and call(Cd=b) == ERR_ARG
    assert call(Cd=a + 23 * size) == ERR_ARG                    # C begins at A's last element
    assert call(Cd=a - 19 * size) == ERR_ARG                    # C's last element (4 x 5, ldc 5: 20) is A's first
    assert call(Cd=b + 29 * size) == ERR_ARG and call(Cd=b - 19 * size) == ERR_ARG
    assert call(Cd=a + 3 * size, lda=100, ldc=100) == ERR_ARG   # interleaved by the padding still counts as overlapping
    assert hs.lib().spgemm_hip_last_error()


# ---- the Python class refuses before device work ---------------------------------------------------------------------
def _hollow(rows, cols, dtype=np.float32):
    """a hs.DenseMatrix with no memory behind it: anything that reached the device would fail differently"""
    d = hs.DenseMatrix()
    d.values, d.rows, d.cols, d.ld, d.dtype = 1 << 40, rows, cols, cols, np.dtype(dtype)
    return d


def test_python_class_refuses_mismatches_before_device_work():
    A = _hollow(4, 6)
    with pytest.raises(hs.SpgemmError, match="shape mismatch"):
        A.matmul(_hollow(5, 3))
    with pytest.raises(hs.SpgemmError, match="mixed value types"):
        A.matmul(_hollow(6, 3, np.float64))
    with pytest.raises(hs.SpgemmError, match="DenseMatrix"):
        A.matmul(np.zeros((6, 3), np.float32))
    with pytest.raises(hs.SpgemmError, match="2-D"):
        hs.DenseMatrix.from_host(np.zeros(5, np.float32))
    with pytest.raises(hs.SpgemmError):
        hs.DenseMatrix.from_host(np.zeros((2, 2), np.int32))    # not a value type
    with pytest.raises(hs.SpgemmError, match="rule"):
        A.to_csr(rule=2)
    with pytest.raises(hs.SpgemmError, match="tol"):
        A.to_csr(tol=-1.0)
    assert (hs.DENSE_KEEP_REFERENCE, hs.DENSE_KEEP_ABS) == (dr.KEEP_REFERENCE, dr.KEEP_ABS) == (0, 1)
