"""CPU: the sparse add / symmetrisation entry points are declared and exported and check their arguments without a GPU,
and the numpy restatement they are held to (symmetrize_ref) is pinned against dense numpy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from devcsr import built  # noqa: F401
from devcsr import _outs
from helpers import ROOT
from sparse_matrix_with_flops_amd import hipspgemm as hs
import symmetrize_ref as sr

ERR_ARG = 2
ONE = C.c_void_p(16)          # a "device pointer" that is never dereferenced
NAN = float("nan")
ENTRIES = ["hip_csr_add", "hip_csr_add_f64", "hip_csr_scale", "hip_csr_scale_f64", "hip_csr_col_counts",
           "hip_degree_factors", "hip_degree_factors_f64", "hip_csr_symmetrize", "hip_csr_symmetrize_f64"]


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spgemm_hip.h")).read()
    L = hs.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/spgemm_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in hs.EXPORTS
    for name, value in (("SUM", hs.SYM_SUM), ("BIBLIOMETRIC", hs.SYM_BIBLIOMETRIC),
                        ("DEGREE_DISCOUNTED", hs.SYM_DEGREE_DISCOUNTED)):
        assert int(re.search(r"#define SPGEMM_SYM_" + name + r"\s+(\d+)", header).group(1)) == value
        assert getattr(sr, "SYM_" + name) == value
    for name in ("csr_add_raw", "csr_scale_raw", "csr_col_counts_raw", "degree_factors_raw", "csr_symmetrize_raw"):
        assert callable(getattr(hs, name))


def test_new_header_is_part_of_the_build():
    info = open(os.path.join(ROOT, "sparse_matrix_with_flops_amd", "libspgemm_hip.so.buildinfo")).read()
    assert re.search(r"^[0-9a-f]{64}\s+symmetrize_device\.hpp$", info, re.M), info


# ---- SPGEMM_ERR_ARG without a device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["hip_csr_add", "hip_csr_add_f64"])
def test_add_argument_errors_do_not_need_a_gpu(entry):
    fn = getattr(hs.lib(), entry)

    def call(m=4, n=4, alpha=1.0, a=(ONE, ONE, ONE), nnzA=3, beta=1.0, b=(ONE, ONE, ONE), nnzB=3, drop=None):
        k, outs = C.c_int(7), _outs(3)
        args = [C.byref(o) for o in outs] + [C.byref(k)]
        if drop is not None:
            args[drop] = None
        return fn(None, m, n, alpha, *a, nnzA, beta, *b, nnzB, *args), k.value, [o.value for o in outs]

    for drop in range(4):
        assert call(drop=drop)[0] == ERR_ARG
    cases = [{"m": -1}, {"n": -1}, {"nnzA": -1}, {"nnzB": -1}, {"alpha": NAN}, {"beta": NAN},
             {"a": (None, ONE, ONE)}, {"a": (ONE, None, ONE)}, {"a": (ONE, ONE, None)},
             {"b": (None, ONE, ONE)}, {"b": (ONE, None, ONE)}, {"b": (ONE, ONE, None)},
             {"m": 0, "nnzA": 1}, {"m": 0, "nnzA": 0, "nnzB": 1}]
    for kw in cases:
        rc, k, outs = call(**kw)
        assert rc == ERR_ARG and k == 0 and outs == [None, None, None], kw
    assert hs.lib().spgemm_hip_last_error()


@pytest.mark.parametrize("entry", ["hip_csr_scale", "hip_csr_scale_f64"])
def test_scale_argument_errors_do_not_need_a_gpu(entry):
    fn = getattr(hs.lib(), entry)

    def call(m=4, n=4, nnz=3, arrays=(ONE, ONE, ONE), scales=(ONE, ONE), out=ONE):
        return fn(None, m, n, nnz, *arrays, *scales, out)

    assert call(m=-1) == ERR_ARG and call(n=-1) == ERR_ARG and call(nnz=-1) == ERR_ARG
    for k in range(3):
        arrays = [ONE, ONE, ONE]
        arrays[k] = None
        assert call(arrays=arrays) == ERR_ARG
    assert call(out=None) == ERR_ARG
    assert call(m=0, nnz=1) == ERR_ARG
    assert call(nnz=0, arrays=(ONE, None, None), out=None) == 0                            # nothing to do: no device


def test_col_counts_and_degree_factors_argument_errors_do_not_need_a_gpu():
    L = hs.lib()
    cc = L.hip_csr_col_counts
    assert cc(None, -1, 3, ONE, ONE) == ERR_ARG and cc(None, 4, -1, ONE, ONE) == ERR_ARG
    assert cc(None, 4, 3, None, ONE) == ERR_ARG and cc(None, 4, 3, ONE, None) == ERR_ARG
    assert cc(None, 0, 0, None, None) == 0
    for entry in ("hip_degree_factors", "hip_degree_factors_f64"):
        df = getattr(L, entry)
        assert df(None, -1, ONE, 0.5, ONE) == ERR_ARG
        assert df(None, 4, None, 0.5, ONE) == ERR_ARG and df(None, 4, ONE, 0.5, None) == ERR_ARG
        assert df(None, 4, ONE, NAN, ONE) == ERR_ARG
        assert df(None, 0, None, 0.5, None) == 0


@pytest.mark.parametrize("entry", ["hip_csr_symmetrize", "hip_csr_symmetrize_f64"])
def test_symmetrize_argument_errors_do_not_need_a_gpu(entry):
    fn = getattr(hs.lib(), entry)

    def call(mode=hs.SYM_SUM, alpha=0.5, beta=0.5, m=4, arrays=(ONE, ONE, ONE), nnz=3, drop=None):
        k, outs = C.c_int(7), _outs(3)
        args = [C.byref(o) for o in outs] + [C.byref(k)]
        if drop is not None:
            args[drop] = None
        return fn(None, mode, alpha, beta, m, *arrays, nnz, *args), k.value, [o.value for o in outs]

    for drop in range(4):
        assert call(drop=drop)[0] == ERR_ARG
    cases = [{"mode": 3}, {"mode": -1}, {"m": -1}, {"nnz": -1}, {"arrays": (None, ONE, ONE)}, {"arrays": (ONE, None, ONE)},
             {"arrays": (ONE, ONE, None)}, {"m": 0, "nnz": 2},
             {"mode": hs.SYM_DEGREE_DISCOUNTED, "alpha": NAN}, {"mode": hs.SYM_DEGREE_DISCOUNTED, "beta": NAN}]
    for kw in cases:
        rc, k, outs = call(**kw)
        assert rc == ERR_ARG and k == 0 and outs == [None, None, None], kw
    assert call(mode=7)[0] == ERR_ARG and b"mode" in hs.lib().spgemm_hip_last_error()
    # alpha and beta are read by the degree-discounted mode only: the other modes get as far as the device with a NaN
    # (not run here), so only the argument order is checked: a NaN with a bad mode is still the mode's error
    assert call(mode=9, alpha=NAN)[0] == ERR_ARG and b"mode" in hs.lib().spgemm_hip_last_error()


def test_python_mirror_refuses_before_device_work():
    a = hs.CSR(16, 16, 16, 4, 5, 3, True, dtype=np.float32)                          # device "pointers" never dereferenced
    b = hs.CSR(16, 16, 16, 5, 4, 3, True, dtype=np.float32)
    d = hs.CSR(16, 16, 16, 4, 5, 3, True, dtype=np.float64)
    with pytest.raises(hs.SpgemmError, match="shape"):
        a.add(b)
    with pytest.raises(hs.SpgemmError, match="mixed"):
        a.add(d)
    with pytest.raises(hs.SpgemmError, match="square"):
        a.symmetrize()


# ---- the restatement against dense numpy -----------------------------------------------------------------------------
def _random(rows, cols, density, rng, dtype):
    P = rng.random((rows, cols)) < density
    D = np.where(P, (rng.random((rows, cols)) + 0.25) * rng.choice([-1.0, 1.0], size=(rows, cols)), 0.0)
    D = D.astype(np.float32).astype(np.float64)
    if np.dtype(dtype) == np.float64:
        D = np.where(P, D + 2.0 ** -40, 0.0)
    return sr.from_dense(D.astype(dtype), P)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref_add_equals_dense_numpy_bit_for_bit(dtype):
    rng = np.random.default_rng(2025)
    coefficients = [(1.0, 1.0), (1.0, -1.0), (0.5, 2.0), (1.0, 0.0), (0.0, 0.0), (0.3, -0.7)]
    for shape in range(40):
        rows, cols = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        A = _random(rows, cols, rng.random() * 0.6, rng, dtype)
        B = _random(rows, cols, rng.random() * 0.6, rng, dtype)
        alpha, beta = coefficients[shape % len(coefficients)]
        got = sr.add(A, B, alpha, beta)
        V = np.dtype(dtype).type
        # dense: every cell alpha*a + beta*b in V; where one operand has no entry the restatement skips its term, which
        # changes no bit: x + (+-0) == x for every x the other term can be but -0.0, and no term here is a zero unless
        # its coefficient is 0 (then both sides hold +-0 and compare equal as numbers; see the structure check below)
        want = V(alpha) * sr.to_dense(A) + V(beta) * sr.to_dense(B)
        dense = sr.to_dense(got)
        assert dense.dtype == np.dtype(dtype)
        assert np.array_equal(dense, want), (shape, rows, cols, alpha, beta)
        nz = want != 0
        assert dense[nz].tobytes() == want[nz].tobytes()
        # structure: the union of the patterns, rows strictly ascending, whatever the sums are
        assert np.array_equal(sr.pattern(got), sr.pattern(A) | sr.pattern(B))
        rp = np.asarray(got.rowPtr, np.int64)
        for r in range(rows):
            assert np.all(np.diff(got.colInd[rp[r]:rp[r + 1]]) > 0)


def test_ref_add_by_hand():
    A = sr.Host([0, 2, 2, 3], [0, 2, 1], np.array([1, 2, 3], np.float32), 3, 3)
    B = sr.Host([0, 2, 3, 3], [1, 2, 0], np.array([10, 20, 30], np.float32), 3, 3)
    S = sr.add(A, B, 1.0, -1.0)
    assert S.rowPtr.tolist() == [0, 3, 4, 5] and S.colInd.tolist() == [0, 1, 2, 0, 1]
    assert S.values.tolist() == [1, -10, -18, -30, 3]
    Z = sr.add(A, A, 1.0, -1.0)                                   # every sum is zero, every entry stays
    assert Z.rowPtr.tolist() == A.rowPtr.tolist() and Z.values.tolist() == [0, 0, 0]


def test_ref_scale_col_counts_and_factors_by_hand():
    A = sr.Host([0, 2, 3], [0, 2, 2], np.array([1, 2, 3], np.float32), 2, 3)
    rs, cs = np.array([2, 3], np.float32), np.array([5, 7, 11], np.float32)
    assert sr.scale(A, rs, cs).tolist() == [10, 44, 99] and sr.scale(A, rs, None).tolist() == [2, 4, 9]
    assert sr.scale(A, None, cs).tolist() == [5, 22, 33] and sr.scale(A).tolist() == [1, 2, 3]
    assert sr.col_counts(A).tolist() == [1, 0, 2]
    assert sr.degree_factors([0, 1, 4], 0.5, np.float32).tolist() == [0, 1, 0.5]


def test_ref_symmetrisations_by_hand():
    # 0 -> 1, 0 -> 2, 1 -> 2, 2 -> 2 (a self loop), 1 -> 0 (0 <-> 1 in both directions)
    A = sr.Host([0, 2, 4, 5], [1, 2, 0, 2, 2], np.array([1, 2, 4, 8, 16], np.float32), 3, 3)
    S = sr.sym_sum(A)
    assert sr.to_dense(S).tolist() == [[0, 5, 2], [5, 0, 8], [2, 8, 32]]
    D = sr.to_dense(A, np.float64)
    assert np.array_equal(sr.to_dense(sr.sym_bibliometric(A)), D @ D.T + D.T @ D)
    dd = sr.to_dense(sr.sym_degree_discounted(A, 0.5, 0.5))
    do, di = np.array([2, 2, 1.0]) ** -0.5, np.array([1, 1, 3.0]) ** -0.5
    Y = do[:, None] * D * di[None, :]
    want = Y @ D.T * do[None, :] + (di[:, None] * D.T * do[None, :]) @ (D * di[None, :])
    assert np.allclose(dd, want, rtol=1e-14, atol=0) and np.array_equal(dd != 0, dd.T != 0)
