"""CPU: the comparison entry points (hip_csr_diff, hip_csr_differsStats and their _f64 twins) check their arguments
without a GPU, the Python mirror refuses a shape or dtype mismatch before any device work, and the numpy restatement the
GPU tests compare against (tests/compare_ref.py) is pinned: on a hand-worked 3 x 5 pair whose expected report and bucket
counts are written out below, and against the C++ mirror's host CSR::differsStats on one oracle R-MCL iteration of
tests/golden/data/own_graph.snap with the reference's percents (nlibs/qrmcl.cc:17)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compare_ref as cr
from devcsr import built  # noqa: F401
from helpers import DATA, ROOT, po
from sparse_matrix_with_flops_amd import hipspgemm as hs

ERR_ARG = 2
REF_PERCENTS = [-30, -20, -5, 0, 5, 20, 30, 100]


@pytest.mark.parametrize("name", ["hip_csr_diff", "hip_csr_diff_f64"])
def test_diff_argument_errors_do_not_need_a_gpu(name):
    fn = getattr(hs.lib(), name)
    one = C.c_void_p(8)                                     # a non-null "device pointer": never dereferenced
    out = hs.CsrDiff()
    o = C.byref(out)

    def call(m=1, n=1, IA=one, JA=None, A=None, nnzA=0, IB=one, JB=None, B=None, nnzB=0, rel=1e-6, tol=0.0, rep=o):
        return fn(None, m, n, IA, JA, A, nnzA, IB, JB, B, nnzB, rel, tol, rep)

    assert call(rep=None) == ERR_ARG                        # a null report
    assert call(m=-1) == ERR_ARG and call(n=-1) == ERR_ARG and call(nnzA=-1) == ERR_ARG and call(nnzB=-1) == ERR_ARG
    assert call(IA=None) == ERR_ARG and call(IB=None) == ERR_ARG
    assert call(nnzA=3, JA=None, A=one) == ERR_ARG and call(nnzA=3, JA=one, A=None) == ERR_ARG
    assert call(nnzB=3, JB=None, B=one) == ERR_ARG and call(nnzB=3, JB=one, B=None) == ERR_ARG
    assert call(rel=-1e-9) == ERR_ARG and call(tol=-1.0) == ERR_ARG
    assert call(rel=float("nan")) == ERR_ARG and call(tol=float("nan")) == ERR_ARG
    assert hs.lib().spgemm_hip_last_error()
    assert all(getattr(out, f) == 0 for f, _ in hs.CsrDiff._fields_)


@pytest.mark.parametrize("name,ptr,ctype", [("hip_csr_differsStats", hs._F, C.c_float),
                                            ("hip_csr_differsStats_f64", hs._D, C.c_double)])
def test_differs_stats_argument_errors_do_not_need_a_gpu(name, ptr, ctype):
    fn = getattr(hs.lib(), name)
    one = C.c_void_p(8)
    pc = (ctype * 65)()
    counts = (C.c_int * 69)()
    assert fn(None, 4, one, one, pc, 8, None) == ERR_ARG    # null counts
    assert fn(None, -1, one, one, pc, 8, counts) == ERR_ARG
    assert fn(None, 4, None, one, pc, 8, counts) == ERR_ARG
    assert fn(None, 4, one, None, pc, 8, counts) == ERR_ARG
    assert fn(None, 4, one, one, pc, -1, counts) == ERR_ARG
    assert fn(None, 4, one, one, pc, 65, counts) == ERR_ARG
    assert fn(None, 4, one, one, None, 8, counts) == ERR_ARG
    assert hs.lib().spgemm_hip_last_error()


def test_mirror_refuses_mismatches_before_device_work():
    # device CSRs with no memory behind them: anything that reached the device would fail differently
    a32 = hs.CSR(None, None, None, 3, 4, 0, on_device=True, dtype=np.float32)
    a64 = hs.CSR(None, None, None, 3, 4, 0, on_device=True, dtype=np.float64)
    wide = hs.CSR(None, None, None, 3, 5, 0, on_device=True, dtype=np.float32)
    tall = hs.CSR(None, None, None, 4, 4, 0, on_device=True, dtype=np.float32)
    for other in (wide, tall):
        for call in (a32.diff, a32.differs):
            with pytest.raises(hs.SpgemmError, match="shape"):
                call(other)
    with pytest.raises(hs.SpgemmError, match="shape"):
        a32.differsStats(tall, REF_PERCENTS)
    for call in (a32.diff, a32.differs, a32.isEqual, a32.isParityEqual):
        with pytest.raises(hs.SpgemmError, match="mixed"):
            call(a64)
    with pytest.raises(hs.SpgemmError, match="mixed"):
        a32.isRelativeEqual(a64, 1e-6)
    with pytest.raises(hs.SpgemmError, match="mixed"):
        a32.differsStats(a64, REF_PERCENTS)
    # the predicates answer False for another shape, as the reference's do
    assert not a32.isEqual(wide) and not a32.isParityEqual(tall) and not a32.isRelativeEqual(wide, 1e-6)


class _Host:
    def __init__(self, rowPtr, colInd, values, rows, cols):
        self.rowPtr, self.colInd = np.array(rowPtr, np.int32), np.array(colInd, np.int32)
        self.values = np.array(values, np.float64)
        self.rows, self.cols = rows, cols


def _pair():
    """        A                        B
    row 0    (1: 2.0) (3: 4.0)        --                                    emptied: two only-A entries
    row 1    --                       (0: 0.5) (4: 3.0)                     appeared: two only-B entries
    row 2    (0: 1) (2: 2.0) (4: 8)   (0: 1) (2: 2.5) (4: 8 (1 + 2^-30))    unchanged length: identical, beyond, within"""
    A = _Host([0, 2, 2, 5], [1, 3, 0, 2, 4], [2.0, 4.0, 1.0, 2.0, 8.0], 3, 5)
    B = _Host([0, 0, 2, 5], [0, 4, 0, 2, 4], [0.5, 3.0, 1.0, 2.5, 8.0 * (1 + 2.0 ** -30)], 3, 5)
    return A, B


def test_restatement_on_the_hand_worked_pair():
    A, B = _pair()
    rep, terms = cr.report(A, B, rel=1e-6, abs_tol=0.0)
    assert rep == dict(rows_len_differ=2, first_len_row=0, only_a=2, only_b=2, first_only_row=0, beyond=1, first_beyond_row=2,
                       max_abs_err=0.5, max_rel_err=0.2, max_abs_only_a=4.0, max_abs_only_b=3.0)
    # 2^2 + 4^2 + 0.5^2 + 3^2 + 0 + 0.5^2 + (2^-27)^2: the last term is below half an ulp of 29.5
    assert sorted(terms) == [0.0, 2.0 ** -54, 0.25, 0.25, 4.0, 9.0, 16.0] and cr.sum_sq(terms) == 29.5
    assert cr.differs_f32(A, B) == 29.5
    # the other way round B is the reference side: 0.5 / 2.0
    back, _ = cr.report(B, A, rel=1e-6, abs_tol=0.0)
    assert back["max_rel_err"] == 0.25 and (back["only_a"], back["only_b"]) == (2, 2) and back["max_abs_only_a"] == 3.0
    # a tolerance that admits the 0.5: |a - b| <= 0.3 + 0.1 * 2.5
    assert cr.report(A, B, rel=0.1, abs_tol=0.3)[0]["beyond"] == 0
    assert cr.report(A, B, rel=0.1, abs_tol=0.2)[0]["beyond"] == 1
    # percents -30 -20 -5 0 5 20 30 100: row 0 shrank by 100 % = -1.0 -> first threshold above it is 0 (slot 3); row 1
    # appeared (slot n + 1 = 9); row 2 kept its length (slot n + 3 = 11)
    for dt in (np.float32, np.float64):
        assert cr.differs_stats(A.rowPtr, B.rowPtr, REF_PERCENTS, dt) == [0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1]
    assert cr.differs_stats(A.rowPtr, B.rowPtr, [], np.float32) == [1, 1, 0, 1]
    assert cr.differs_stats(A.rowPtr, B.rowPtr, [-1.0], np.float32) == [0, 1, 1, 0, 1]      # strict: -1 < -1 is false
    assert not cr.is_equal(A, B) and not cr.is_relative_equal(A, B, 1e-6)
    assert cr.is_equal(A, A) and cr.is_relative_equal(A, A, 0.0)
    near = _Host(A.rowPtr, A.colInd, A.values + np.array([0, 0, 5e-8, 0, 0]), 3, 5)
    far = _Host(A.rowPtr, A.colInd, A.values + np.array([0, 0, 2e-7, 0, 0]), 3, 5)
    assert cr.is_equal(near, A) and not cr.is_equal(far, A)
    assert cr.is_relative_equal(far, A, 1e-6) and not cr.is_relative_equal(far, A, 1e-7)


def test_nan_in_the_restatement():
    A, B = _pair()
    A.values[4] = np.nan                                    # row 2, column 4: common
    rep, terms = cr.report(A, B)
    assert rep["beyond"] == 2 and rep["max_abs_err"] == 0.5 and rep["max_rel_err"] == 0.2
    assert np.isnan(cr.sum_sq(terms))


def test_restatement_matches_the_mirrors_host_differs_stats(tmp_path):
    """A = own_graph.snap after rmclInit, B = one oracle R-MCL iteration of it; the C++ mirror's host CSR::differsStats
    (tests/cpp/compare_check.cc --host-stats, no device work) gives the counts the restatement gives"""
    A = po.load(os.path.join(DATA, "own_graph.snap"), isTrans=True, mode=1)
    B = po.rmcl_iters(A, A, 1)
    assert A.rows == B.rows and not np.array_equal(A.rowPtr, B.rowPtr)
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp, "compare_check.x"])
    files = []
    for name, M in (("a.txt", A), ("b.txt", B)):
        files.append(str(tmp_path / name))
        with open(files[-1], "w") as fp:
            fp.write(f"{M.rows}\n" + " ".join(str(int(x)) for x in M.rowPtr) + "\n")
    out = subprocess.run([os.path.join(cpp, "compare_check.x"), "--host-stats"] + files, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [int(x) for x in out.stdout.split()]
    want = cr.differs_stats(A.rowPtr, B.rowPtr, REF_PERCENTS, np.float32)
    assert got == want and sum(got) == A.rows
    assert sum(1 for x in want if x) >= 2                   # the iteration moved some rows and left others
