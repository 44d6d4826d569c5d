"""CPU: the selection entry points (hip_csr_row_topk, its limits, the path counters, the R-MCL loop with a row cap) are
declared and exported, check their arguments without a GPU, and the numpy restatement they are held to (topk_ref) gives
the hand-worked answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from devcsr import built  # noqa: F401
from devcsr import _outs
from helpers import ROOT
from sparse_matrix_with_flops_amd import hipspgemm as hs
import topk_ref as tr

ERR_ARG = 2
ONE = C.c_void_p(16)          # a "device pointer" that is never dereferenced
ENTRIES = ["hip_csr_row_topk", "hip_csr_row_topk_f64", "hip_csr_row_topk_limits", "spgemm_hip_debug_topk_paths",
           "hip_gpuRmclIter_device_topk", "hip_gpuRmclIter_device_topk_f64"]


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spgemm_hip.h")).read()
    L = hs.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/spgemm_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in hs.EXPORTS
        assert getattr(L, name).argtypes, f"{name} has no argtypes in lib()"
    assert int(re.search(r"#define SPGEMM_TOPK_NORMALISE (\d+)", header).group(1)) == hs.TOPK_NORMALISE
    assert len(L.hip_csr_row_topk.argtypes) == 14 and len(L.hip_gpuRmclIter_device_topk.argtypes) == 19


def test_new_header_is_part_of_the_build():
    info = open(os.path.join(ROOT, "sparse_matrix_with_flops_amd", "libspgemm_hip.so.buildinfo")).read()
    assert re.search(r"^[0-9a-f]{64}\s+topk_device\.hpp$", info, re.M), info


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_limits_order_the_three_paths(dtype):
    wave, block = hs.row_topk_limits(dtype)
    assert 64 <= wave < block
    assert hs.lib().hip_csr_row_topk_limits(0, None, None) == ERR_ARG
    with pytest.raises(hs.SpgemmError, match="dtype"):
        hs.row_topk_limits(np.float16)


@pytest.mark.parametrize("entry", ["hip_csr_row_topk", "hip_csr_row_topk_f64"])
def test_selection_argument_errors_leave_the_outputs_alone(entry):
    fn = getattr(hs.lib(), entry)

    def call(m=4, n=4, nnz=3, arrays=(ONE, ONE, ONE), k=2, flags=0, drop=None):
        nn, cut, outs = C.c_int(7), C.c_int(7), _outs(3)
        args = [C.byref(o) for o in outs] + [C.byref(nn), C.byref(cut)]
        if drop is not None:
            args[drop] = None
        return fn(None, m, n, nnz, *arrays, k, flags, *args), nn.value, cut.value, [o.value for o in outs]

    for drop in range(4):                                   # rowsCut (slot 4) may be null: not an error by itself
        assert call(drop=drop)[0] == ERR_ARG
    cases = [{"k": 0}, {"k": -3}, {"flags": 2}, {"flags": 3}, {"flags": -1}, {"m": -1}, {"n": -1}, {"nnz": -1},
             {"arrays": (None, ONE, ONE)}, {"arrays": (ONE, None, ONE)}, {"arrays": (ONE, ONE, None)}, {"m": 0, "nnz": 2}]
    for kw in cases:
        rc, nn, cut, outs = call(**kw)
        assert rc == ERR_ARG and nn == 0 and cut == 0 and outs == [None, None, None], kw
    assert call(k=0)[0] == ERR_ARG and b"k=0" in hs.lib().spgemm_hip_last_error()
    assert call(flags=6)[0] == ERR_ARG and b"flag" in hs.lib().spgemm_hip_last_error()
    assert call(k=0, drop=4)[0] == ERR_ARG


@pytest.mark.parametrize("entry", ["hip_gpuRmclIter_device_topk", "hip_gpuRmclIter_device_topk_f64"])
def test_loop_argument_errors_leave_the_outputs_alone(entry):
    fn = getattr(hs.lib(), entry)

    def call(maxIter=2, k=4, rows=4, cols=4, g=(ONE, ONE, ONE), gnnz=3, t=(ONE, ONE, ONE), tnnz=3, drop=None):
        nn, outs = C.c_int(7), _outs(3)
        args = [C.byref(o) for o in outs] + [C.byref(nn)]
        if drop is not None:
            args[drop] = None
        return fn(None, maxIter, k, rows, cols, *g, gnnz, *t, tnnz, *args, None, None), nn.value, [o.value for o in outs]

    for drop in range(4):
        assert call(drop=drop)[0] == ERR_ARG
    cases = [{"k": 0}, {"k": -1}, {"maxIter": -1}, {"cols": 5}, {"rows": -1, "cols": -1}, {"gnnz": -1}, {"tnnz": -1},
             {"g": (None, ONE, ONE)}, {"g": (ONE, None, ONE)}, {"t": (ONE, ONE, None)}, {"t": (None, ONE, ONE)}]
    for kw in cases:
        rc, nn, outs = call(**kw)
        assert rc == ERR_ARG and nn == 0 and outs == [None, None, None], kw


def test_python_mirror_refuses_before_device_work():
    host = hs.CSR.from_arrays([0, 1], [0], [1.0], 1, 1)
    with pytest.raises(hs.SpgemmError, match="device CSR"):
        host.row_topk(1)
    odd = hs.CSR(16, 16, 16, 4, 4, 3, True, dtype=np.float16)
    with pytest.raises(hs.SpgemmError, match="dtype"):
        odd.row_topk(1)
    dev = hs.CSR(16, 16, 16, 4, 4, 3, True, dtype=np.float32)                       # device "pointers" never dereferenced
    with pytest.raises(hs.SpgemmError, match="k=0"):
        dev.row_topk(0)
    with pytest.raises(hs.SpgemmError, match="k=0"):
        hs.gpuRmclIterTopK_device(1, 0, dev, dev)
    with pytest.raises(hs.SpgemmError, match="mixed"):
        hs.gpuRmclIterTopK_device(1, 2, dev, hs.CSR(16, 16, 16, 4, 4, 3, True, dtype=np.float64))


# ---- the restatement, on a 4-row matrix worked by hand ---------------------------------------------------------------
def _csr(rows, dtype=np.float32):
    """rows: list of lists of (col, value)"""
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    v = np.array([x for r in rows for _, x in r], dtype)
    return rp, ci, v


NAN = float("nan")
HAND = [[(5, .5), (1, .25), (3, .5), (0, .5), (2, .125)],     # three values tie at .5: the columns 0 and 3 win over 5
        [(4, .5), (2, .25), (4, .5), (4, .5)],                # value and column tie: the earlier positions win
        [(1, NAN), (0, .25), (2, NAN), (3, -1.)],             # two numbers, k = 3: one NaN is kept, that of the smaller column
        [(3, 0.0), (1, -0.0), (2, -1.), (0, -0.0)]]           # the zeros are equal: columns 0 and 1 win, signs kept


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ref_hand_worked_matrix(dtype):
    rp, ci, v = _csr(HAND, dtype)
    out, cut = tr.row_topk(rp, ci, v, 4, 6, 2)
    assert cut == 4 and out.rowPtr.tolist() == [0, 2, 4, 6, 8]
    assert out.colInd.tolist() == [3, 0, 4, 4, 0, 3, 1, 0]
    assert out.values.dtype == np.dtype(dtype)
    assert out.values[:6].tolist() == [.5, .5, .5, .5, .25, -1.]
    assert np.signbit(out.values[6:]).tolist() == [True, True] and out.values[6:].tolist() == [0.0, 0.0]
    # row 1 kept positions 0 and 2, not 3; row 2 at k = 3 keeps the NaN of column 1 and keeps the storage order
    assert tr.keep_of_row(ci[5:9], v[5:9], 2).tolist() == [0, 2]
    out3, cut3 = tr.row_topk(rp, ci, v, 4, 6, 3)
    assert cut3 == 4 and out3.colInd[6:9].tolist() == [1, 0, 3] and np.isnan(out3.values[6])
    assert out3.colInd[9:12].tolist() == [3, 1, 0]                                  # all three zeros, -1 dropped
    # k >= the longest row: a bit-identical copy, nothing cut
    same, cut5 = tr.row_topk(rp, ci, v, 4, 6, 5)
    assert cut5 == 0 and same.values.tobytes() == v.tobytes() and same.colInd.tolist() == ci.tolist()


def test_ref_nan_ranks_below_minus_infinity_whatever_its_sign():
    neg_nan = np.array([0xffc00001], np.uint32).view(np.float32)[0]
    v = np.array([neg_nan, -np.inf, NAN, -3.0], np.float32)
    assert tr.row_order([0, 1, 2, 3], v).tolist() == [3, 1, 0, 2]
    assert tr.row_order([9, 1, 2, 3], v).tolist() == [3, 1, 2, 0]                   # among NaNs the column decides


def test_ref_normalise_touches_only_the_rows_that_were_cut():
    rp, ci, v = _csr([[(0, .5), (1, .25), (2, .125)], [(0, .5), (1, .25)]])
    out, cut = tr.row_topk(rp, ci, v, 2, 3, 2, normalise=True)
    assert cut == 1 and out.values.tolist() == [np.float32(.5) / np.float32(.75), np.float32(.25) / np.float32(.75), .5, .25]


def test_ref_float64_is_not_compared_in_float():
    a, b = 0.5, 0.5 + 2.0 ** -40
    assert tr.row_order([0, 1], np.array([a, b])).tolist() == [1, 0]
    assert tr.row_order([0, 1], np.array([a, b], np.float32)).tolist() == [0, 1]    # a tie once rounded to float
