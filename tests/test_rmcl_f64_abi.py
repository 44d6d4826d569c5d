"""CPU: the double-precision R-MCL entry points exist with the declared argument types, check their arguments without a
GPU, the Python mirror dispatches on the value type and refuses mixed operands before any device work, and the float64
reference of the row rule (rmcl_f64_ref.py) equals a plain per-row loop of the rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from devcsr import built  # noqa: F401
from rmcl_f64_ref import row_rule64, step64, step_bound
from f64ref import EPS64, Host64
from sparse_matrix_with_flops_amd import hipspgemm as hs

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "spgemm_hip.h")
ERR_ARG = 2

DECLS = {
    "hip_rmcl_prune_f64": "spgemm_handle* h, int m, const int* dIC, const int* dJC, const double* dC, "
                          "int** dIN, int** dJN, double** dCN, int* nnzN",
    "hip_rmcl_prune_n_f64": "spgemm_handle* h, int m, int nnz, const int* dIC, const int* dJC, const double* dC, "
                            "int** dIN, int** dJN, double** dCN, int* nnzN",
    "hip_rmcl_expand_prune_f64": "spgemm_handle* h, const int* dIA, const int* dJA, const double* dA, int nnzA, "
                                 "const int* dIB, const int* dJB, const double* dB, int nnzB, int m, int k, int n, "
                                 "int** dIN, int** dJN, double** dCN, int* nnzN",
    "hip_gpuRmclIter_device_f64": "spgemm_handle* h, int maxIter, int rows, int cols, "
                                  "const int* dgI, const int* dgJ, const double* dgA, int gnnz, "
                                  "const int* dtI, const int* dtJ, const double* dtA, int tnnz, "
                                  "int** oI, int** oJ, double** oA, int* onnz",
    "hip_gpuRmclIter_f64": "int maxIter, int rows, int cols, const int* gIA, const int* gJA, const double* gA, int gnnz, "
                           "const int* tIA, const int* tJA, const double* tA, int tnnz, "
                           "int** oIA, int** oJA, double** oA, int* onnz",
}


def test_the_five_symbols_exist_with_their_argument_types():
    L = hs.lib()
    text = re.sub(r"\s+", " ", open(HEADER).read())
    for name, args in DECLS.items():
        assert hasattr(L, name), name
        assert name in hs.EXPORTS
        assert f"int {name}({args});" in text, f"{name}: the header declares other arguments"
    # the ctypes mirror: same shapes as the float twins, double pointers where the host arrays are typed
    for name in ("hip_rmcl_prune", "hip_rmcl_prune_n", "hip_rmcl_expand_prune", "hip_gpuRmclIter_device"):
        assert getattr(L, name + "_f64").argtypes == getattr(L, name).argtypes
    f64 = L.hip_gpuRmclIter_f64.argtypes
    f32 = L.hip_gpuRmclIter.argtypes
    assert len(f64) == len(f32) == 15
    assert [i for i, (a, b) in enumerate(zip(f64, f32)) if a is not b] == [5, 9, 13]
    assert f64[5] is hs._D and f64[9] is hs._D and f64[13] == C.POINTER(hs._D)
    text_f64 = text[text.index("(5) double values"):]
    assert "Not available in double: R-MCL" not in text_f64


def test_argument_errors_do_not_need_a_gpu():
    L = hs.lib()
    rp = np.zeros(3, np.int32)
    P = rp.ctypes.data_as(C.c_void_p)
    o = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    refs = [C.byref(x) for x in o]
    n = C.c_int(-1)
    # null outputs
    assert L.hip_rmcl_prune_f64(None, 2, P, None, None, None, None, None, None) == ERR_ARG
    assert L.hip_rmcl_prune_n_f64(None, 2, 0, P, None, None, None, None, None, None) == ERR_ARG
    assert L.hip_rmcl_expand_prune_f64(None, P, None, None, 0, P, None, None, 0, 2, 2, 2, None, None, None, None) == ERR_ARG
    assert L.hip_gpuRmclIter_device_f64(None, 1, 2, 2, P, None, None, 0, P, None, None, 0, None, None, None, None) == ERR_ARG
    I0, D0 = hs._I(), hs._D()
    rpi = rp.ctypes.data_as(hs._I)
    assert L.hip_gpuRmclIter_f64(1, 2, 2, rpi, I0, D0, 0, rpi, I0, D0, 0, None, None, None, None) == ERR_ARG
    # a negative nnz, a negative dimension, colInd/values missing
    assert L.hip_rmcl_prune_n_f64(None, 2, -1, P, None, None, *refs, C.byref(n)) == ERR_ARG
    assert L.hip_rmcl_expand_prune_f64(None, P, None, None, 0, P, None, None, 0, -1, 2, 2, *refs, C.byref(n)) == ERR_ARG
    assert L.hip_rmcl_expand_prune_f64(None, P, None, None, 3, P, None, None, 0, 2, 2, 2, *refs, C.byref(n)) == ERR_ARG
    assert b"colInd/values null" in L.spgemm_hip_last_error()
    # not square, negative maxIter: both loops
    oi, oj, ov = hs._I(), hs._I(), hs._D()
    for rows, cols, it in ((2, 3, 1), (2, 2, -1)):
        n.value = 7
        assert L.hip_gpuRmclIter_device_f64(None, it, rows, cols, P, None, None, 0, P, None, None, 0, *refs, C.byref(n)) == ERR_ARG
        assert b"square matrix" in L.spgemm_hip_last_error() and n.value == 0
        n.value = 7
        assert L.hip_gpuRmclIter_f64(it, rows, cols, rpi, I0, D0, 0, rpi, I0, D0, 0, C.byref(oi), C.byref(oj), C.byref(ov),
                                     C.byref(n)) == ERR_ARG
        assert b"square matrix" in L.spgemm_hip_last_error() and n.value == 0
    assert [x.value for x in o] == [None, None, None]


def test_mixed_dtypes_raise_before_device_work():
    a = hs.CSR(None, None, None, 2, 2, 0, on_device=True, dtype=np.float32)   # no device memory behind it: never used
    b = hs.CSR(None, None, None, 2, 2, 0, on_device=True, dtype=np.float64)
    for x, y in ((a, b), (b, a)):
        with pytest.raises(hs.SpgemmError, match="mixed"):
            hs.gpuRmclIter_device(1, x, y)
    ha = hs.CSR.from_arrays([0, 1], [0], [1.0], 1, 1)
    hb = hs.CSR.from_arrays([0, 1], [0], [1.0], 1, 1, dtype=np.float64)
    with pytest.raises(hs.SpgemmError, match="mixed"):
        hs.gpuRmclIter(1, ha, hb)
    for name in ("rmcl_prune_raw_f64", "rmcl_expand_prune_raw_f64", "rmcl_iter_device_raw_f64"):
        assert callable(getattr(hs, name))


# ---- the reference of the row rule -----------------------------------------------------------------------------------
def plain_rule(values):
    """util.cc:4-69 / qrmcl.cc:96-117 on one row, operation by operation -> (kept indices, kept values, th)"""
    v = [float(c) * float(c) for c in values]
    rmax, rsum = 0.0, 0.0
    for x in v:
        if rmax < x:
            rmax = x
    for x in v:
        rsum += x
    avg = rsum / len(v) if len(v) else float("nan")
    th = 0.90 * avg * (1 - 2 * (rmax - avg))
    th = th if th > 1.0e-7 else 1.0e-7
    th = rmax if th > rmax else th
    idx, kept, s = [], [], 0.0
    for i, x in enumerate(v):
        if x >= th:
            s += x
            idx.append(i)
            kept.append(x)
    return idx, [x / s for x in kept], th


def test_row_rule64_equals_a_plain_loop():
    rng = np.random.default_rng(77)
    rows = []
    for i in range(200):
        l = int(rng.integers(1, 90))
        scale = 10.0 ** rng.uniform(-6, 0)
        rows.append(rng.uniform(0.05, 1.0, l) * scale)
    rows[3] = np.zeros(0)                                  # an empty row
    rows[5] = np.array([0.37])                             # one entry
    rows[7] = np.array([4e-4, 1e-4, 1e-4, 1e-4])           # the formula gives 4.3e-8 and mx = 1.6e-7: th is raised to 1e-7
    rows[9] = np.array([1e-4, 2e-4, 3e-4])                 # mx = 9e-8 < 1e-7: th is lowered to mx
    rp = np.zeros(len(rows) + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    ci = np.concatenate([rng.permutation(1000)[:len(r)] for r in rows]).astype(np.int32)
    vals = np.concatenate(rows)
    kept, th, gap = row_rule64(rp, ci, vals)
    assert kept.values.dtype == np.float64 and len(th) == len(gap) == 200
    for i, r in enumerate(rows):
        idx, kv, t = plain_rule(r)
        a, b = kept.rowPtr[i], kept.rowPtr[i + 1]
        assert th[i] == t or (np.isnan(t) and np.isnan(th[i])), i
        assert list(kept.colInd[a:b]) == list(ci[rp[i]:rp[i + 1]][idx]), i          # input order
        assert list(kept.values[a:b]) == kv, i                                      # the same operations: the same bits
        if len(r):
            v = np.asarray(r) ** 2
            assert gap[i] == np.min(np.abs(v - t) / t), i
    # the documented behaviour of the four special rows
    assert kept.rowPtr[4] == kept.rowPtr[3] and th[3] == 0.0 and gap[3] == np.inf           # empty: stays empty
    assert kept.rowPtr[6] - kept.rowPtr[5] == 1 and kept.values[kept.rowPtr[5]] == 1.0      # one entry: kept, becomes 1
    assert th[5] == 0.9 * (0.37 * 0.37)
    assert th[7] == 1.0e-7 and 0 < kept.rowPtr[8] - kept.rowPtr[7] < 4                       # clamped up to 1e-7
    assert th[9] == 3e-4 * 3e-4 and th[9] < 1.0e-7                                           # clamped down to mx
    assert list(kept.colInd[kept.rowPtr[9]:kept.rowPtr[10]]) == [ci[rp[9] + 2]] and kept.values[kept.rowPtr[9]] == 1.0


def test_step64_reports_terms_and_row_length():
    A = Host64([0, 2, 3], [0, 1, 1], [0.5, 0.5, 1.0], 2, 2)
    B = Host64([0, 2, 4], [0, 1, 0, 1], [0.9, 0.1, 0.2, 0.8], 2, 2)
    s = step64(A, B)
    assert (s.N, s.n) == (2, 2) and s.bound == step_bound(2, 2) == (8 * 2 + 2 * 2 + 16) * EPS64
    assert list(s.product.rowPtr) == [0, 2, 4] and s.kept.cols == 2
    assert np.allclose(np.add.reduceat(s.kept.values, s.kept.rowPtr[:-1].astype(np.int64)), 1.0)
