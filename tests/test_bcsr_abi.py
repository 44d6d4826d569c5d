"""CPU: the blocked-CSR entry points (hip_csr_to_bcsr, hip_bcsr_to_csr and their _f64 twins) check their arguments without
a GPU, the mirrors refuse a shape or dtype mismatch before any device work, and the restatement the GPU tests compare
against (tests/bcsr_ref.py) is pinned on hand-worked matrices whose expected arrays are written out below."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bcsr_ref as br
import reorder_ref as rr
from devcsr import built  # noqa: F401
from devcsr import _outs
from helpers import ROOT, random_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

ERR_ARG = 2
TWINS = ["", "_f64"]


# ---- the hand-worked matrices ----------------------------------------------------------------------------------------
# per format: a matrix worked by hand for this format's layout (3 x 6 for 2 x 2 tiles)
def _hand():
    """A is 3 x 6, r = c = 2, so bm = 2, bn = 3:
    row 0   (5, 1.0) (0, 2.0)
    row 1   (2, 3.0) (4, 4.0) (0, 5.0)
    row 2   (3, 6.0) (3, 7.0)            repeated column"""
    return rr.Host([0, 2, 5, 7], [5, 0, 2, 4, 0, 3, 3], np.array([1, 2, 3, 4, 5, 6, 7], np.float32), 3, 6)


def _ragged():
    """5 x 5: rows {1:2} {1:3, 4:3} {0:4} {1:1, 3:5} {0:2}"""
    return rr.Host([0, 1, 3, 4, 6, 7], [1, 1, 4, 0, 1, 3, 0], np.array([2, 3, 3, 4, 1, 5, 2], np.float32), 5, 5)


def test_restatement_on_the_hand_worked_matrix():
    B = br.to_bcsr(_hand(), 2, 2)
    assert (B.bm, B.bn, B.nnzb, B.nnz) == (2, 3, 4, 7)
    assert B.rowPtr.tolist() == [0, 3, 4]
    # block row 0: row 0 meets block column 2 (col 5), then 0 (col 0); row 1 adds 1 (col 2); 4 and 0 are known by then
    assert B.colInd.tolist() == [2, 0, 1, 1]
    assert B.values.tolist() == [0, 1, 4, 0, 2, 0, 5, 0, 0, 0, 3, 0, 0, 7, 0, 0]     # (2, 3): 7.0 came last
    assert B.values.dtype == np.float32 and br.density(B) == 43.75
    back = br.to_csr(B, 1e-9)
    assert back.rowPtr.tolist() == [0, 2, 5, 6]
    assert back.colInd.tolist() == [5, 0, 4, 0, 2, 3]
    assert back.values.tolist() == [1, 2, 4, 5, 3, 7] and back.values.dtype == np.float32


def test_restatement_on_the_ragged_matrix():
    B = br.to_bcsr(_ragged(), 2, 2)
    assert (B.bm, B.bn) == (3, 3)
    assert B.rowPtr.tolist() == [0, 2, 4, 5] and B.colInd.tolist() == [0, 2, 0, 1, 0]
    assert B.values.tolist() == [0, 2, 0, 3, 0, 0, 3, 0, 4, 0, 0, 1, 0, 0, 0, 5, 2, 0, 0, 0]
    # the cells beyond row 4 / column 4 exist, hold +0.0, and never come back out
    assert rr.same_bits(rr.sort_rows(br.to_csr(B)), rr.sort_rows(_ragged()))


def test_restatement_with_unit_tiles_is_the_csr_itself():
    A = random_csr(23, 31, 0.2, 5, sorted_rows=False)
    B = br.to_bcsr(A, 1, 1)
    assert np.array_equal(B.rowPtr, A.rowPtr) and np.array_equal(B.colInd, A.colInd)
    assert B.values.tobytes() == np.ascontiguousarray(A.values).tobytes() and br.density(B) == 100.0
    assert rr.same_bits(br.to_csr(B), rr.Host(A.rowPtr, A.colInd, A.values, A.rows, A.cols))
    # a sorted A comes back as it was after a row sort, whatever the tile
    S = rr.sort_rows(rr.Host(A.rowPtr, A.colInd, A.values, A.rows, A.cols))
    for r, c in ((2, 2), (3, 5), (64, 64)):
        assert rr.same_bits(rr.sort_rows(br.to_csr(br.to_bcsr(S, r, c))), S), (r, c)


def test_restatement_keeps_float64_bits_and_applies_the_tolerance_in_double():
    A = _hand()
    A64 = rr.Host(A.rowPtr, A.colInd, A.values.astype(np.float64) + 2.0 ** -40, 3, 6)
    B = br.to_bcsr(A64, 2, 2)
    assert B.values.dtype == np.float64
    assert B.values[[1, 2, 4, 6, 10, 13]].tolist() == [x + 2.0 ** -40 for x in (1, 4, 2, 5, 3, 7)]
    assert br.to_csr(B).values.tolist() == [x + 2.0 ** -40 for x in (1, 2, 4, 5, 3, 7)]
    # one row of special values: NaN, -0.0, a denormal, 1e-9 and the next double above it
    up = np.nextafter(1e-9, 1.0)
    v = np.array([np.nan, -0.0, 5e-324, 1e-9, up], np.float64)
    S = rr.Host([0, 5], [0, 1, 2, 3, 4], v, 1, 5)
    T = br.to_bcsr(S, 1, 5)
    assert T.values.tobytes() == v.tobytes()
    assert br.to_csr(T, 1e-9).colInd.tolist() == [4] and br.to_csr(T, 0.0).colInd.tolist() == [2, 3, 4]
    assert br.density(br.to_bcsr(rr.Host([0, 0], [], np.zeros(0, np.float32), 1, 5), 2, 2)) == 0.0


# ---- argument errors: no device is touched (the "device pointers" are never dereferenced) ----------------------------
ONE = C.c_void_p(8)


@pytest.mark.parametrize("twin", TWINS)
def test_to_bcsr_argument_errors_do_not_need_a_gpu(twin):
    fn = getattr(hs.lib(), "hip_csr_to_bcsr" + twin)
    nnzb = C.c_int(7)

    def call(m=4, n=4, nnz=0, IA=ONE, JA=None, A=None, r=2, c=2, outs=None, count=C.byref(nnzb)):
        o = outs if outs is not None else [C.byref(x) for x in _outs()]
        return fn(None, m, n, nnz, IA, JA, A, r, c, *o, count)

    assert call(r=0) == ERR_ARG and call(c=0) == ERR_ARG and call(r=-1) == ERR_ARG and call(c=-1) == ERR_ARG
    assert call(r=4097, c=1) == ERR_ARG and call(r=1, c=4097) == ERR_ARG and call(r=17, c=241) == ERR_ARG     # 4097 cells
    assert call(r=2 ** 16, c=2 ** 16) == ERR_ARG                # r * c wraps to 0 in 32 bits
    for k in range(3):
        o = [C.byref(x) for x in _outs()]
        o[k] = None
        assert call(outs=o) == ERR_ARG                          # a null output
    assert call(count=None) == ERR_ARG
    assert call(m=-1) == ERR_ARG and call(n=-1) == ERR_ARG and call(nnz=-1) == ERR_ARG
    assert call(IA=None) == ERR_ARG
    assert call(nnz=3, JA=None, A=ONE) == ERR_ARG and call(nnz=3, JA=ONE, A=None) == ERR_ARG
    assert call(m=0, nnz=3, JA=ONE, A=ONE) == ERR_ARG           # entries in a matrix without rows
    assert hs.lib().spgemm_hip_last_error()
    outs = _outs()
    assert call(r=0, outs=[C.byref(x) for x in outs]) == ERR_ARG
    assert [x.value for x in outs] == [None, None, None] and nnzb.value == 0


@pytest.mark.parametrize("twin", TWINS)
def test_to_csr_argument_errors_do_not_need_a_gpu(twin):
    fn = getattr(hs.lib(), "hip_bcsr_to_csr" + twin)
    nnzC = C.c_int(7)

    def call(m=4, n=4, r=2, c=2, nnzb=0, IB=ONE, JB=None, B=None, tol=1e-9, outs=None, count=C.byref(nnzC)):
        o = outs if outs is not None else [C.byref(x) for x in _outs()]
        return fn(None, m, n, r, c, nnzb, IB, JB, B, tol, *o, count)

    assert call(r=0) == ERR_ARG and call(c=0) == ERR_ARG and call(r=-1) == ERR_ARG and call(c=-1) == ERR_ARG
    assert call(r=4097, c=1) == ERR_ARG and call(r=1, c=4097) == ERR_ARG and call(r=17, c=241) == ERR_ARG
    for k in range(3):
        o = [C.byref(x) for x in _outs()]
        o[k] = None
        assert call(outs=o) == ERR_ARG
    assert call(count=None) == ERR_ARG
    assert call(m=-1) == ERR_ARG and call(n=-1) == ERR_ARG and call(nnzb=-1) == ERR_ARG
    assert call(tol=-1e-30) == ERR_ARG and call(tol=float("nan")) == ERR_ARG and call(tol=float("-inf")) == ERR_ARG
    assert call(IB=None) == ERR_ARG
    assert call(nnzb=3, JB=None, B=ONE) == ERR_ARG and call(nnzb=3, JB=ONE, B=None) == ERR_ARG
    assert call(m=0, nnzb=3, JB=ONE, B=ONE) == ERR_ARG          # tiles in a matrix without rows
    assert hs.lib().spgemm_hip_last_error()
    outs = _outs()
    assert call(tol=-1.0, outs=[C.byref(x) for x in outs]) == ERR_ARG
    assert [x.value for x in outs] == [None, None, None] and nnzC.value == 0


# ---- the mirrors refuse before device work ---------------------------------------------------------------------------
def _hollow_bcsr(m, n, r, c, dtype=np.float32):
    """a hs.BCSR with no memory behind it: anything that reached the device would fail differently"""
    b = hs.BCSR.__new__(hs.BCSR)
    b.m, b.n, b.r, b.c, b.nnz, b.nnzb, b.dtype = m, n, r, c, 7, 4, np.dtype(dtype)
    b.bm, b.bn = (m + r - 1) // r, (n + c - 1) // c
    b.rowPtr = b.colInd = b.values = None
    return b


def test_python_mirror_refuses_mismatches_before_device_work():
    b = _hollow_bcsr(3, 6, 2, 2)
    assert b.nonzero_density() == 43.75
    for rows, cols in ((4, 6), (3, 5)):
        with pytest.raises(hs.SpgemmError, match="shape"):
            b.is_equal(hs.CSR(None, None, None, rows, cols, 7, on_device=True))
    with pytest.raises(hs.SpgemmError, match="mixed"):
        b.is_equal(hs.CSR(None, None, None, 3, 6, 7, on_device=True, dtype=np.float64))
    with pytest.raises(hs.SpgemmError, match="mixed"):
        _hollow_bcsr(3, 6, 2, 2, np.float64).is_equal(hs.CSR(None, None, None, 3, 6, 7, on_device=True))
    dM = hs.CSR(None, None, None, 3, 6, 7, on_device=True)
    for r, c in ((0, 2), (2, 0), (4097, 1), (64, 65)):
        with pytest.raises(hs.SpgemmError, match="tile"):
            hs.BCSR.from_csr(dM, r, c)
    with pytest.raises(hs.SpgemmError, match="dtype"):
        hs.BCSR(hs.CSR(None, None, None, 3, 6, 7, on_device=True, dtype=np.int32), 2, 2)
    empty = _hollow_bcsr(3, 6, 2, 2)
    empty.nnz = empty.nnzb = 0
    assert empty.nonzero_density() == 0.0                       # no NaN, no division by zero


def test_cpp_mirror_refuses_a_shape_mismatch_before_device_work():
    """tests/cpp/bcsr_check.cc --shape-check: BCSR::isEqual against another row count and another column count"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "bcsr_check.x"])
    out = subprocess.run([os.path.join(cpp, "bcsr_check.x"), "--shape-check"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refused" in out.stdout and "B 5 x 4" in out.stdout and "B 4 x 5" in out.stdout
