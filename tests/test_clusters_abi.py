"""CPU: the clusters entry points (attractors, connected components, labels -> clusters, the chain) are declared and
exported, check their arguments without a GPU, and the numpy restatement they are held to (clusters_ref) gives the
hand-worked answers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from devcsr import built  # noqa: F401
from devcsr import _outs
from helpers import ROOT
from sparse_matrix_with_flops_amd import hipspgemm as hs
import clusters_ref as cr

ERR_ARG = 2
ONE = C.c_void_p(16)          # a "device pointer" that is never dereferenced
ENTRIES = ["hip_rmcl_attractors", "hip_rmcl_attractors_f64", "hip_csr_connected_components", "hip_labels_to_clusters",
           "hip_rmcl_clusters", "hip_rmcl_clusters_f64"]


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spgemm_hip.h")).read()
    L = hs.lib()
    for name in ENTRIES + ["hip_rmcl_attractor_lanes"]:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/spgemm_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in hs.EXPORTS
    assert int(re.search(r"#define SPGEMM_CC_MAX_ROUNDS (\d+)", header).group(1)) == hs.CC_MAX_ROUNDS


def test_new_header_is_part_of_the_build():
    info = open(os.path.join(ROOT, "sparse_matrix_with_flops_amd", "libspgemm_hip.so.buildinfo")).read()
    assert re.search(r"^[0-9a-f]{64}\s+clusters_device\.hpp$", info, re.M), info


def test_lanes_per_row_follow_the_mean_row_length():
    lanes = hs.rmcl_attractor_lanes
    assert [lanes(100, nnz) for nnz in (0, 100, 899, 900, 6499, 6500, 10 ** 6)] == [4, 4, 4, 16, 16, 64, 64]
    assert lanes(0, 0) == 4


@pytest.mark.parametrize("entry", ["hip_rmcl_attractors", "hip_rmcl_attractors_f64"])
def test_attractors_argument_errors_do_not_need_a_gpu(entry):
    fn = getattr(hs.lib(), entry)

    def call(m=4, n=4, nnz=3, arrays=(ONE, ONE, ONE), parent=ONE):
        return fn(None, m, n, nnz, *arrays, parent)

    assert call(n=5) == ERR_ARG and b"square" in hs.lib().spgemm_hip_last_error()          # m != n
    assert call(parent=None) == ERR_ARG
    assert call(m=-1, n=-1) == ERR_ARG and call(nnz=-1) == ERR_ARG
    for k in (1, 2):
        arrays = [ONE, ONE, ONE]
        arrays[k] = None
        assert call(arrays=arrays) == ERR_ARG                                               # nnz > 0 with null arrays
    assert call(arrays=(None, ONE, ONE)) == ERR_ARG
    assert call(m=0, n=0, nnz=2) == ERR_ARG
    assert call(m=0, n=0, nnz=0, arrays=(None, None, None), parent=None) == 0               # nothing to do: no device


def test_components_argument_errors_do_not_need_a_gpu():
    fn = hs.lib().hip_csr_connected_components

    def call(m=4, n=4, nnz=3, ia=ONE, ja=ONE, label=ONE, ncomp="out", rounds="out"):
        nc, rd = C.c_int(7), C.c_int(7)
        rc = fn(None, m, n, nnz, ia, ja, label, C.byref(nc) if ncomp == "out" else ncomp, C.byref(rd) if rounds == "out" else rounds)
        return rc, nc.value, rd.value

    assert call(n=3) == (ERR_ARG, 0, 0)
    assert call(label=None)[0] == ERR_ARG and call(ncomp=None)[0] == ERR_ARG
    assert call(m=-1, n=-1)[0] == ERR_ARG and call(nnz=-1)[0] == ERR_ARG
    assert call(ia=None)[0] == ERR_ARG and call(ja=None)[0] == ERR_ARG
    assert call(m=0, n=0, nnz=1)[0] == ERR_ARG
    assert call(m=0, n=0, nnz=0, ia=None, ja=None, label=None) == (0, 0, 0)


def test_labels_to_clusters_argument_errors_do_not_need_a_gpu():
    fn = hs.lib().hip_labels_to_clusters
    for missing in range(4):
        k, outs = C.c_int(7), _outs(3)
        args = [C.byref(k)] + [C.byref(o) for o in outs]
        args[missing] = None
        assert fn(None, 4, ONE, *args) == ERR_ARG
        assert all(o.value is None for i, o in enumerate(outs) if i + 1 != missing) and (missing == 0 or k.value == 0)
    k, outs = C.c_int(7), _outs(3)
    assert fn(None, -1, ONE, C.byref(k), *[C.byref(o) for o in outs]) == ERR_ARG
    assert fn(None, 4, None, C.byref(k), *[C.byref(o) for o in outs]) == ERR_ARG
    assert k.value == 0 and all(o.value is None for o in outs)


@pytest.mark.parametrize("entry", ["hip_rmcl_clusters", "hip_rmcl_clusters_f64"])
def test_chain_argument_errors_do_not_need_a_gpu(entry):
    fn = getattr(hs.lib(), entry)

    def call(m=4, n=4, nnz=3, arrays=(ONE, ONE, ONE), drop=None):
        k, outs = C.c_int(7), _outs(3)
        args = [C.byref(k)] + [C.byref(o) for o in outs]
        if drop is not None:
            args[drop] = None
        return fn(None, m, n, nnz, *arrays, *args), k.value, [o.value for o in outs]

    for drop in range(4):
        assert call(drop=drop)[0] == ERR_ARG
    for kw in ({"n": 5}, {"m": -1, "n": -1}, {"nnz": -1}, {"arrays": (ONE, None, ONE)}, {"arrays": (ONE, ONE, None)},
               {"arrays": (None, ONE, ONE)}, {"m": 0, "n": 0, "nnz": 1}):
        rc, k, outs = call(**kw)
        assert rc == ERR_ARG and k == 0 and outs == [None, None, None], kw
    assert hs.lib().spgemm_hip_last_error()


def test_python_mirror_refuses_before_device_work():
    host = hs.CSR.from_arrays([0, 1], [0], [1.0], 1, 1)
    wide = hs.CSR(16, 16, 16, 4, 5, 3, True, dtype=np.float32)                      # device "pointers" never dereferenced
    odd = hs.CSR(16, 16, 16, 4, 4, 3, True, dtype=np.float16)
    for f in (hs.rmcl_attractors, hs.connected_components, hs.rmcl_clusters):
        with pytest.raises(hs.SpgemmError, match="device CSR"):
            f(host)
        with pytest.raises(hs.SpgemmError, match="square"):
            f(wide)
        with pytest.raises(hs.SpgemmError, match="dtype"):
            f(odd)


# ---- the restatement, on cases worked by hand ------------------------------------------------------------------------
def _csr(rows, m):
    """rows: list of lists of (col, value)"""
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    v = np.array([x for r in rows for _, x in r], np.float32)
    return rp, ci, v


def test_ref_six_nodes_two_components():
    # edges 5-3, 3-1 and 4-2, 2-0 stored in one direction only, plus a self loop and a repeated entry
    rp, ci, _ = _csr([[], [], [(0, 1)], [(1, 1), (1, 1)], [(2, 1), (4, 1)], [(3, 1)]], 6)
    label, ncomp = cr.components(6, rp, ci)
    assert label.tolist() == [0, 1, 0, 1, 0, 1] and ncomp == 2
    k, cluster, ptr, members = cr.compact(label)
    assert k == 2 and cluster.tolist() == [0, 1, 0, 1, 0, 1]
    assert ptr.tolist() == [0, 3, 6] and members.tolist() == [0, 2, 4, 1, 3, 5]


def test_ref_two_cycle_of_attractors():
    # 0 and 1 send their largest flow to each other, 2 and 3 follow 1, 4 keeps its own
    rows = [[(0, .4), (1, .6)], [(0, .7), (1, .3)], [(1, .9), (2, .1)], [(3, .2), (1, .8)], [(4, 1.)]]
    k, cluster, ptr, members, parent, label = cr.rmcl_clusters(*_csr(rows, 5))
    assert parent.tolist() == [1, 0, 1, 1, 4] and label.tolist() == [0, 0, 0, 0, 4]
    assert k == 2 and cluster.tolist() == [0, 0, 0, 0, 1] and ptr.tolist() == [0, 4, 5] and members.tolist() == [0, 1, 2, 3, 4]


def test_ref_ties_nan_and_empty_rows():
    nan, inf = float("nan"), float("inf")
    rows = [[(3, .5), (1, .5), (2, .25)],            # two equal maxima: the smaller column, whatever the order
            [(1, .5), (3, .5)],
            [],                                      # empty: itself
            [(0, nan), (1, nan)],                    # all NaN: itself
            [(2, nan), (0, .1), (4, nan)],           # NaN beside a finite value
            [(4, -inf), (1, -inf)],                  # only -inf: still an entry, the smaller column
            [(5, -0.0), (2, 0.0), (6, -1.)]]         # -0.0 == +0.0: the smaller column
    rp, ci, v = _csr(rows, 7)
    assert cr.attractors(rp, ci, v).tolist() == [1, 1, 2, 3, 0, 1, 2]
    assert cr.attractors(rp, ci, v.astype(np.float64)).tolist() == [1, 1, 2, 3, 0, 1, 2]
    # a long row takes the vectorised branch: the same answers
    long_ci = np.concatenate([np.arange(100, 0, -1), [7]]).astype(np.int32)
    long_v = np.concatenate([np.full(100, .5), [nan]])
    long_v[[10, 60]] = .75                           # columns 90 and 40
    assert cr.attractors([0, 101], long_ci, long_v).tolist() == [40]
    assert cr.attractors([0, 3], [2, 1, 0], np.array([-inf, nan, -inf])).tolist() == [0]


def test_ref_float64_is_not_compared_in_float():
    a, b = 0.5, 0.5 + 2.0 ** -40
    v = np.array([a, b])
    assert cr.attractors([0, 2], [0, 1], v).tolist() == [1]
    assert cr.attractors([0, 2], [0, 1], v.astype(np.float32)).tolist() == [0]     # a tie once rounded to float


def test_ref_refuses_non_canonical_labels():
    assert cr.is_canonical([0, 0, 2, 2]) and cr.is_canonical([])
    assert not cr.is_canonical([1, 1]) and not cr.is_canonical([0, 0, 1]) and not cr.is_canonical([0, -1])
