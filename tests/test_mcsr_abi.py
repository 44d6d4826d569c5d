"""CPU: the mixed-CSR entry points (hip_csr_to_mcsr, hip_mcsr_to_csr and their _f64 twins) check their arguments without
a GPU, the Python mirror refuses a shape or dtype mismatch before any device work, and the restatement the GPU tests
compare against (tests/mcsr_ref.py) is pinned on the reference's known-answer vectors (tests/golden/mcsr_kat.json,
r = 1) and on a hand-worked r > 1 case -- the case where the reference's count pass would be wrong."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mcsr_ref as mr
import reorder_ref as rr
from devcsr import built  # noqa: F401
from devcsr import _outs
from helpers import ROOT, random_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

ERR_ARG = 2
TWINS = ["", "_f64"]


def kat():
    with open(os.path.join(ROOT, "tests", "golden", "mcsr_kat.json")) as f:
        return json.load(f)


# ---- the restatement -------------------------------------------------------------------------------------------------
def test_restatement_on_the_reference_vectors():
    k = kat()
    A = rr.Host(k["rowPtr"], k["colInd"], np.array(k["values"], np.float32), k["rows"], k["cols"])
    M = mr.to_mcsr(A, k["r"], k["c"], k["blockRows"], k["blockCols"])
    e = k["expected"]
    assert M.rest.rowPtr.tolist() == e["remainder_rowPtr"] and M.rest.colInd.tolist() == e["remainder_colInd"]
    assert M.rest.values.tolist() == e["remainder_values"] and M.rest.values.dtype == np.float32
    assert (M.rest.rows, M.rest.cols) == (7, 7)
    assert M.corner.rowPtr.tolist() == e["block_rowPtr"] and M.corner.colInd.tolist() == e["block_colInd"]
    assert M.corner.values.tolist() == e["tiles"] and M.corner.values.dtype == np.float32
    assert (M.corner.m, M.corner.n, M.corner.bm, M.corner.bn, M.corner.nnzb, M.corner.nnz) == (4, 4, 4, 2, 4, 6)
    assert mr.density(M) == 75.0
    assert rr.same_bits(mr.to_csr(M, 1e-9), A)               # r == 1, sorted rows: the matrix itself


# per format: a matrix worked by hand for this format's layout (5 x 6 with a 4 x 3 corner)
def _hand():
    """A is 5 x 6; r = c = 2, blockRows = 4, blockCols = 3, so bm = 2, bn = 2 (the last block column is ragged):
    row 0   (4, 1) (1, 2) (2, 3)
    row 1   (0, 4) (5, 5) (2, 6)
    row 2   (3, 7)
    row 3   (2, 8) (2, 9) (0, 10)        repeated column
    row 4   (1, 11) (5, 12)              below the corner
    Rows 0 and 2 are not the last of their block rows and hold remainder entries: the reference's count pass, which
    resets its counter per block row, would give the remainder rowPtr {0,1,3,4,5,7} instead."""
    return rr.Host([0, 3, 6, 7, 10, 12], [4, 1, 2, 0, 5, 2, 3, 2, 2, 0, 1, 5], np.arange(1, 13, dtype=np.float32), 5, 6)


def test_restatement_on_the_hand_worked_tiles_of_two_rows():
    M = mr.to_mcsr(_hand(), 2, 2, 4, 3)
    assert M.corner.rowPtr.tolist() == [0, 2, 4] and M.corner.colInd.tolist() == [0, 1, 1, 0]
    assert M.corner.values.tolist() == [0, 2, 4, 0, 3, 0, 6, 0, 0, 0, 9, 0, 0, 0, 10, 0]       # cell (3, 2): 9 came last
    assert M.rest.rowPtr.tolist() == [0, 1, 2, 3, 3, 5] and M.rest.colInd.tolist() == [4, 5, 3, 1, 5]
    assert M.rest.values.tolist() == [1, 5, 7, 11, 12]
    assert M.corner.nnz == 7 and (M.corner.bm, M.corner.bn, M.corner.nnzb) == (2, 2, 4)
    back = mr.to_csr(M, 1e-9)
    assert back.rowPtr.tolist() == [0, 3, 6, 7, 9, 11]
    assert back.colInd.tolist() == [1, 2, 4, 0, 2, 5, 3, 2, 0, 1, 5]
    assert back.values.tolist() == [2, 3, 1, 4, 6, 5, 7, 9, 10, 11, 12] and back.values.dtype == np.float32


def test_restatement_edges():
    A = random_csr(23, 31, 0.2, 5, sorted_rows=False)
    H = rr.Host(A.rowPtr, A.colInd, A.values, A.rows, A.cols)
    for br_, bc in ((0, 31), (22, 0), (0, 0)):                # no corner: the remainder is A
        M = mr.to_mcsr(H, 2, 3, br_, bc)
        assert M.corner.nnzb == 0 and M.corner.nnz == 0 and rr.same_bits(M.rest, H) and rr.same_bits(mr.to_csr(M), H)
    M = mr.to_mcsr(H, 1, 1, 23, 31)                           # the corner is everything, unit tiles: the CSR itself
    assert M.rest.nnz == 0 and M.rest.rowPtr.tolist() == [0] * 24 and (M.rest.rows, M.rest.cols) == (23, 31)
    assert np.array_equal(M.corner.rowPtr, H.rowPtr) and np.array_equal(M.corner.colInd, H.colInd)
    assert rr.same_bits(mr.to_csr(M), H)
    S = rr.sort_rows(H)
    for r, c, br_, bc in ((1, 4, 7, 9), (1, 64, 23, 30)):     # r == 1 and sorted rows: bit for bit without a sort
        assert rr.same_bits(mr.to_csr(mr.to_mcsr(S, r, c, br_, bc)), S), (r, c, br_, bc)
    for r, c, br_, bc in ((2, 2, 22, 31), (3, 5, 21, 16), (64, 64, 0, 31)):
        assert rr.same_bits(rr.sort_rows(mr.to_csr(mr.to_mcsr(S, r, c, br_, bc))), S), (r, c, br_, bc)
    A64 = rr.Host(H.rowPtr, H.colInd, H.values.astype(np.float64) + 2.0 ** -40, 23, 31)
    M = mr.to_mcsr(A64, 3, 5, 21, 16)
    assert M.corner.values.dtype == np.float64 and M.rest.values.dtype == np.float64
    assert mr.to_csr(M).values.dtype == np.float64


# ---- argument errors: no device is touched (the "device pointers" are never dereferenced) ----------------------------
ONE = C.c_void_p(8)


@pytest.mark.parametrize("twin", TWINS)
def test_to_mcsr_argument_errors_do_not_need_a_gpu(twin):
    fn = getattr(hs.lib(), "hip_csr_to_mcsr" + twin)
    nnzb, nnzR = C.c_int(7), C.c_int(7)

    def call(m=4, n=4, nnz=0, IA=ONE, JA=None, A=None, r=2, c=2, brows=2, bcols=3, outs=None, counts=None):
        o = outs if outs is not None else [C.byref(x) for x in _outs(6)]
        k = counts if counts is not None else [C.byref(nnzb), C.byref(nnzR)]
        return fn(None, m, n, nnz, IA, JA, A, r, c, brows, bcols, o[0], o[1], o[2], k[0], o[3], o[4], o[5], k[1])

    assert call(r=0, brows=0) == ERR_ARG and call(c=0) == ERR_ARG and call(r=-1) == ERR_ARG and call(c=-1) == ERR_ARG
    assert call(r=4097, c=1, brows=0) == ERR_ARG and call(r=1, c=4097) == ERR_ARG and call(r=17, c=241, brows=0) == ERR_ARG
    assert call(r=2 ** 16, c=2 ** 16, brows=0) == ERR_ARG
    assert call(brows=-2) == ERR_ARG and call(brows=6, m=5) == ERR_ARG          # 0 <= blockRows <= m
    assert call(bcols=-1) == ERR_ARG and call(bcols=5) == ERR_ARG               # 0 <= blockCols <= n
    assert call(brows=3) == ERR_ARG and call(r=3, brows=4) == ERR_ARG           # blockRows % r == 0
    for k in range(6):
        o = [C.byref(x) for x in _outs(6)]
        o[k] = None
        assert call(outs=o) == ERR_ARG                                          # a null output
    assert call(counts=[None, C.byref(nnzR)]) == ERR_ARG and call(counts=[C.byref(nnzb), None]) == ERR_ARG
    assert call(m=-1, brows=0) == ERR_ARG and call(n=-1, bcols=0) == ERR_ARG and call(nnz=-1) == ERR_ARG
    assert call(IA=None) == ERR_ARG
    assert call(nnz=3, JA=None, A=ONE) == ERR_ARG and call(nnz=3, JA=ONE, A=None) == ERR_ARG
    assert call(m=0, brows=0, nnz=3, JA=ONE, A=ONE) == ERR_ARG                  # entries in a matrix without rows
    assert hs.lib().spgemm_hip_last_error()
    outs = _outs(6)
    assert call(brows=3, outs=[C.byref(x) for x in outs]) == ERR_ARG
    assert [x.value for x in outs] == [None] * 6 and (nnzb.value, nnzR.value) == (0, 0)


@pytest.mark.parametrize("twin", TWINS)
def test_to_csr_argument_errors_do_not_need_a_gpu(twin):
    fn = getattr(hs.lib(), "hip_mcsr_to_csr" + twin)
    nnzC = C.c_int(7)

    def call(m=4, n=4, r=2, c=2, brows=2, bcols=3, nnzb=0, IB=ONE, JB=None, B=None, nnzR=0, IR=ONE, JR=None, R=None,
             tol=1e-9, outs=None, count=C.byref(nnzC)):
        o = outs if outs is not None else [C.byref(x) for x in _outs(3)]
        return fn(None, m, n, r, c, brows, bcols, nnzb, IB, JB, B, nnzR, IR, JR, R, tol, *o, count)

    assert call(r=0, brows=0) == ERR_ARG and call(c=0) == ERR_ARG and call(r=-1) == ERR_ARG and call(c=-1) == ERR_ARG
    assert call(r=4097, c=1, brows=0) == ERR_ARG and call(r=1, c=4097) == ERR_ARG and call(r=17, c=241, brows=0) == ERR_ARG
    assert call(brows=-2) == ERR_ARG and call(brows=6, m=5) == ERR_ARG
    assert call(bcols=-1) == ERR_ARG and call(bcols=5) == ERR_ARG
    assert call(brows=3) == ERR_ARG and call(r=3, brows=4) == ERR_ARG
    for k in range(3):
        o = [C.byref(x) for x in _outs(3)]
        o[k] = None
        assert call(outs=o) == ERR_ARG
    assert call(count=None) == ERR_ARG
    assert call(m=-1, brows=0) == ERR_ARG and call(n=-1, bcols=0) == ERR_ARG
    assert call(nnzb=-1) == ERR_ARG and call(nnzR=-1) == ERR_ARG
    assert call(tol=-1e-30) == ERR_ARG and call(tol=float("nan")) == ERR_ARG and call(tol=float("-inf")) == ERR_ARG
    assert call(IB=None) == ERR_ARG and call(IR=None) == ERR_ARG
    assert call(nnzb=3, JB=None, B=ONE) == ERR_ARG and call(nnzb=3, JB=ONE, B=None) == ERR_ARG
    assert call(nnzR=3, JR=None, R=ONE) == ERR_ARG and call(nnzR=3, JR=ONE, R=None) == ERR_ARG
    assert call(brows=0, nnzb=3, JB=ONE, B=ONE) == ERR_ARG                      # tiles in a corner without rows
    assert call(m=0, brows=0, nnzR=3, JR=ONE, R=ONE) == ERR_ARG                 # entries in a matrix without rows
    assert hs.lib().spgemm_hip_last_error()
    outs = _outs(3)
    assert call(tol=-1.0, outs=[C.byref(x) for x in outs]) == ERR_ARG
    assert [x.value for x in outs] == [None, None, None] and nnzC.value == 0


# ---- the mirror refuses before device work ---------------------------------------------------------------------------
def _hollow_mcsr(m, n, r, c, brows, bcols, rest, dtype=np.float32):
    """a hs.MCSR with no memory behind it: anything that reached the device would fail differently"""
    x = hs.MCSR.__new__(hs.MCSR)
    x.m, x.n, x.r, x.c, x.blockRows, x.blockCols, x.nnz, x.nnzb, x.dtype = m, n, r, c, brows, bcols, 7, 4, np.dtype(dtype)
    x.bm, x.bn = brows // r, (bcols + c - 1) // c
    x.rowPtr = x.colInd = x.values = None
    x.remainder = rest
    return x


def test_python_mirror_refuses_mismatches_before_device_work():
    dM = hs.CSR(None, None, None, 5, 6, 12, on_device=True)
    for r, c in ((0, 2), (2, 0), (4097, 1), (64, 65)):
        with pytest.raises(hs.SpgemmError, match="tile"):
            hs.MCSR.from_csr(dM, r, c, 0, 3)
    for brows, bcols in ((-2, 3), (6, 3), (4, -1), (4, 7), (3, 3)):
        with pytest.raises(hs.SpgemmError, match="corner"):
            hs.MCSR.from_csr(dM, 2, 2, brows, bcols)
    with pytest.raises(hs.SpgemmError, match="dtype"):
        hs.MCSR(hs.CSR(None, None, None, 5, 6, 12, on_device=True, dtype=np.int32), 2, 2, 4, 3)
    for rows, cols in ((4, 6), (5, 5)):
        with pytest.raises(hs.SpgemmError, match="shape"):
            _hollow_mcsr(5, 6, 2, 2, 4, 3, hs.CSR(None, None, None, rows, cols, 5, on_device=True)).to_csr()
    with pytest.raises(hs.SpgemmError, match="mixed"):
        _hollow_mcsr(5, 6, 2, 2, 4, 3, hs.CSR(None, None, None, 5, 6, 5, on_device=True, dtype=np.float64)).to_csr()
    with pytest.raises(hs.SpgemmError, match="mixed"):
        _hollow_mcsr(5, 6, 2, 2, 4, 3, hs.CSR(None, None, None, 5, 6, 5, on_device=True), np.float64).to_csr()
    x = _hollow_mcsr(5, 6, 2, 2, 4, 3, None)
    assert x.nonzero_density() == 43.75                       # 7 entries in 4 tiles of 4 cells
    x.nnz = x.nnzb = 0
    assert x.nonzero_density() == 0.0                         # no NaN, no division by zero
