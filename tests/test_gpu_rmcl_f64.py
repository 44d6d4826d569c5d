"""GPU: R-MCL in double (hip_rmcl_prune_f64, hip_rmcl_expand_prune_f64, hip_gpuRmclIter_device_f64, hip_gpuRmclIter_f64)
against the float64 reference of rmcl_f64_ref.py.

Every case first asserts, on the reference alone, that every row's gap (min |v^2 - th| / th) is at least 1000 times the
case's value bound; under that precondition the device must keep exactly the reference's entries (row pointer and the
column set of every row), and every value must be within the bound: no tie allowance, no excluded rows.

Inputs: values in [0.3, 1.0), then every row of A scaled so that the largest entry of its product row is 0.7 (without the
scaling the rule keeps everything; with it, a strict subset).  Every case also asserts, on the reference, that a row of
each path it claims has 0 < kept < L."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import clusters_ref as cr
from f64ref import Host64, sorted_rows, spgemm_f64
from rmcl_f64_ref import loop64, row_rule64, step64, step_bound
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
F64 = np.float64
F64_LDS_MAXL = 6144                                  # csrc/spgemm_f64_device.hpp: the last row length the LDS table takes in one pass
EDGES = [1, 2, 4, 5, 16, 17, 64, 65, 512, 513, 2048, 2049, 4096, 4097]
# product counts of the rows each numeric launch takes: 16 lanes per row (two table sizes), one block per row (four sizes)
PATHS = [(1, 16), (17, 64), (65, 512), (513, 2048), (2049, 4096), (4097, 1 << 30)]
# the launches in which a row of the case keeps a strict subset (the folded rows of 65 and 512 products fold onto 13 and
# 102 columns of nearly equal sums, and the rule keeps them all: that launch is claimed by the flat case only)
CLAIMED_PATHS = {"flat": PATHS, "folded": PATHS[:2] + PATHS[3:]}


@pytest.fixture(scope="module")
def handle():
    if hs.device_count() < 1:
        pytest.fail("GPU test without a HIP device")
    return hs.Handle(0)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def rows_csr(rows_cols, ncols, seed):
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(rows_cols) + 1, np.int32)
    np.cumsum([len(c) for c in rows_cols], out=rp[1:])
    ci = np.concatenate([np.asarray(c, np.int32) for c in rows_cols]) if len(rows_cols) else np.zeros(0, np.int32)
    return Host64(rp, ci, rng.uniform(0.3, 1.0, len(ci)), len(rows_cols), ncols)


def scaled(A, B):
    """A with every row scaled so that the largest entry of its row of A*B is 0.7"""
    ref = spgemm_f64(A, B)
    lens = np.diff(ref.rowPtr)
    mx = np.ones(A.rows)
    live = lens > 0
    if ref.nnz:
        mx[live] = np.maximum.reduceat(ref.values, ref.rowPtr[:-1][live].astype(np.int64))
    row_of = np.repeat(np.arange(A.rows), np.diff(A.rowPtr))
    return Host64(A.rowPtr, A.colInd, A.values * (0.7 / mx)[row_of], A.rows, A.cols)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (A, B, Step64 of A*B): built once, shared, never modified"""
    n = 9000
    lens = sorted(set(EDGES)) + [0]
    if name in ("flat", "folded"):
        if name == "flat":
            brows = [np.arange(l, dtype=np.int32) * 2 % n for l in lens]
        else:
            brows = [np.arange(l, dtype=np.int32) % max(3, l // 5) for l in lens]
        B = rows_csr(brows, n, 5)
        # one A entry per row; then a row whose only B row is empty, an empty row, and one more short row behind them
        A = rows_csr([[lens.index(e)] for e in EDGES] + [[lens.index(0)], [], [lens.index(2)]], len(lens), 6)
    elif name == "wide":
        rng = np.random.default_rng(7)
        k, n = 3000, 700000
        B = rows_csr([np.sort(rng.choice(n, size=int(rng.integers(40, 120)), replace=False)) for _ in range(k)], n, 1)
        A = rows_csr([rng.choice(k, size=s, replace=False) for s in (400, 90, 1, 0, 700, 64, 65, 2500)], k, 2)
    elif name == "seam":
        rng = np.random.default_rng(11)
        n = 20000
        B = rows_csr([rng.permutation(n)[:F64_LDS_MAXL], rng.permutation(n)[:F64_LDS_MAXL + 1]], n, 3)
        A = rows_csr([[0], [1]], 2, 4)
    elif name == "graph":
        A = B = power_law_graph(2000, 21)
        return A, B, step64(A, B)
    else:
        raise KeyError(name)
    A = scaled(A, B)
    return A, B, step64(A, B)


def power_law_graph(n, seed):
    """what rmclInit makes of a symmetric power-law edge list: self loops, rows 1/deg (float64)"""
    rng = np.random.default_rng(seed)
    deg = np.minimum((rng.pareto(1.6, n) * 3 + 2).astype(np.int64), n // 8)
    src = np.repeat(np.arange(n), deg)
    dst = rng.integers(0, n, len(src))
    r = np.concatenate([src, dst, np.arange(n)])
    c = np.concatenate([dst, src, np.arange(n)])
    key = np.unique(r * n + c)
    r, c = key // n, key % n
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=rp[1:])
    d = np.diff(rp)
    return Host64(rp, c, (1.0 / d)[r], n, n)


def strict_subset_rows(step, lo, hi):
    """rows of the reference whose product row has lo <= L <= hi entries and 0 < kept < L"""
    L = np.diff(step.product.rowPtr)
    kept = np.diff(step.kept.rowPtr)
    return np.flatnonzero((L >= lo) & (L <= hi) & (kept > 0) & (kept < L))


def precondition(steps, bound, what):
    for s in steps:
        g = float(np.min(s.gap)) if len(s.gap) else np.inf
        assert g >= 1000.0 * bound, f"{what}: bad input, smallest gap {g:.3e} < 1000 * bound {bound:.3e}"


# ---- device calls ----------------------------------------------------------------------------------------------------
def dev(M):
    return hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols, dtype=F64).toGpuCSR()


def take(out, rows, cols):
    """(I, J, V, nnz) of pool arrays -> host CSR; the device arrays are released"""
    i_, j_, v_, n_ = out
    d = hs.CSR(v_, j_, i_, rows, cols, n_, True, dtype=F64)
    try:
        return d.toCpuCSR()
    finally:
        d.deviceDispose()


def fused(handle, A, B):
    dA = dev(A)
    dB = dA if B is A else dev(B)
    try:
        return take(hs.rmcl_expand_prune_raw_f64(handle, dA.rowPtr, dA.colInd, dA.values, dA.nnz, dB.rowPtr, dB.colInd,
                                                 dB.values, dB.nnz, A.rows, A.cols, B.cols), A.rows, B.cols)
    finally:
        dA.deviceDispose()
        if dB is not dA:
            dB.deviceDispose()


def assert_structure(got, want, what):
    assert got.values.dtype == F64, what
    assert np.array_equal(np.asarray(got.rowPtr), want.rowPtr), f"{what}: row pointer"
    gc, gv = sorted_rows(got.rowPtr, got.colInd, got.values)
    wc, wv = sorted_rows(want.rowPtr, want.colInd, want.values)
    assert np.array_equal(gc, wc), f"{what}: kept columns"
    return gv, wv


def assert_step(got, want, bound, what):
    """the kept structure exactly, every value within bound * reference"""
    gv, wv = assert_structure(got, want, what)
    err = np.abs(gv - wv)
    bad = np.flatnonzero(err > bound * wv)
    worst = float((err / wv).max()) if len(wv) else 0.0
    print(f"{what}: kept {want.nnz} entries, worst relative error {worst:.3e}, bound {bound:.3e}")
    assert len(bad) == 0, f"{what}: {len(bad)} values beyond the bound, first {gv[bad[0]]!r} vs {wv[bad[0]]!r}"


# ---- 1. every kernel path of the fused step ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat", "folded"])
def test_fused_step_every_bin(handle, name):
    A, B, step = case(name)
    precondition([step], step.bound, name)
    L = np.diff(step.product.rowPtr)
    assert list(L[:len(EDGES)]) == (EDGES if name == "flat" else [min(e, max(3, e // 5)) for e in EDGES])
    kept = np.diff(step.kept.rowPtr)
    for lo, hi in CLAIMED_PATHS[name]:                           # a row of every claimed launch loses entries
        rows = [r for r, e in enumerate(EDGES) if lo <= e <= hi]
        assert any(0 < kept[r] < L[r] for r in rows), (name, lo, hi)
    assert L[len(EDGES)] == 0 and L[len(EDGES) + 1] == 0 and L[len(EDGES) + 2] > 0    # the rows without products
    assert_step(fused(handle, A, B), step.kept, step.bound, name)


def test_fused_step_without_rows_and_without_entries(handle):
    B5 = rows_csr([[0, 1]] * 5, 3, 1)
    E = Host64(np.zeros(1), np.zeros(0), np.zeros(0), 0, 5)      # m = 0
    got = fused(handle, E, B5)
    assert got.nnz == 0 and list(got.rowPtr) == [0]
    Z = Host64(np.zeros(4), np.zeros(0), np.zeros(0), 3, 5)      # nnz = 0
    got = fused(handle, Z, B5)
    assert got.nnz == 0 and list(got.rowPtr) == [0, 0, 0, 0]


def test_fused_step_wide_rows(handle):
    A, B, step = case("wide")
    precondition([step], step.bound, "wide")
    L = np.diff(step.product.rowPtr)
    assert len(strict_subset_rows(step, 4097, F64_LDS_MAXL)) > 0          # one LDS pass of bin 8
    assert len(strict_subset_rows(step, F64_LDS_MAXL + 1, 65536)) > 0     # several passes: k_rmcl_fix_rows<double>
    assert len(strict_subset_rows(step, 65537, 1 << 30)) > 0              # device-memory table: k_rmcl_fix_rows<double>
    assert L.max() > 65536
    assert_step(fused(handle, A, B), step.kept, step.bound, "wide")


def test_fused_step_lds_seam(handle):
    A, B, step = case("seam")
    precondition([step], step.bound, "seam")
    assert list(np.diff(step.product.rowPtr)) == [F64_LDS_MAXL, F64_LDS_MAXL + 1]
    assert len(strict_subset_rows(step, F64_LDS_MAXL, F64_LDS_MAXL)) == 1
    assert len(strict_subset_rows(step, F64_LDS_MAXL + 1, F64_LDS_MAXL + 1)) == 1
    assert_step(fused(handle, A, B), step.kept, step.bound, "seam")


# ---- 2. prune of a C in device memory ------------------------------------------------------------------------------------
def random_unsorted_c(seed=31):
    rng = np.random.default_rng(seed)
    rows, cols = 300, 517
    lens = rng.integers(0, 200, rows)
    lens[:4] = [0, 1, 16, 17]
    rc = [rng.permutation(cols)[:l] for l in lens]
    C0 = rows_csr(rc, cols, seed + 1)
    mx = np.ones(rows)
    live = lens > 0
    mx[live] = np.maximum.reduceat(C0.values, C0.rowPtr[:-1][live].astype(np.int64))
    return Host64(C0.rowPtr, C0.colInd, C0.values * np.repeat(0.7 / mx, lens), rows, cols)


def prune_inputs(name):
    if name == "random":
        return random_unsorted_c()
    p = case(name)[2].product
    return Host64(p.rowPtr, p.colInd, p.values, p.rows, p.cols)


@pytest.mark.parametrize("name", ["flat", "wide", "random"])
def test_prune_f64(handle, name):
    Cm = prune_inputs(name)
    want, _, gap = row_rule64(Cm.rowPtr, Cm.colInd, Cm.values)
    bound = step_bound(0, int(np.diff(Cm.rowPtr).max()))
    assert float(gap.min()) >= 1000.0 * bound, f"{name}: bad input, gap {gap.min():.3e}"
    assert np.any((np.diff(want.rowPtr) > 0) & (np.diff(want.rowPtr) < np.diff(Cm.rowPtr)))
    dC = dev(Cm)
    try:
        a = take(hs.rmcl_prune_raw_f64(handle, Cm.rows, dC.rowPtr, dC.colInd, dC.values), Cm.rows, Cm.cols)
        b = take(hs.rmcl_prune_raw_f64(handle, Cm.rows, dC.rowPtr, dC.colInd, dC.values, nnz=Cm.nnz), Cm.rows, Cm.cols)
        back = dC.toCpuCSR()
    finally:
        dC.deviceDispose()
    assert np.array_equal(back.values, Cm.values) and np.array_equal(back.colInd, Cm.colInd)      # the input is left alone
    assert np.array_equal(a.rowPtr, want.rowPtr)
    assert np.array_equal(a.colInd, want.colInd), f"{name}: kept entries are not in input order"   # stable compaction
    err = np.abs(a.values - want.values)
    assert np.all(err <= bound * want.values), f"{name}: worst {float((err / want.values).max()):.3e} bound {bound:.3e}"
    for x, y in ((a.rowPtr, b.rowPtr), (a.colInd, b.colInd), (a.values, b.values)):
        assert np.array_equal(x, y), f"{name}: hip_rmcl_prune_f64 and hip_rmcl_prune_n_f64 differ"


# ---- 3. fused equals two-step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["folded", "wide"])
def test_fused_equals_two_steps(handle, name):
    A, B, step = case(name)
    precondition([step], step.bound, name)
    one = fused(handle, A, B)
    dA, dB = dev(A), dev(B)
    try:
        ic, jc, vc, nnz = hs.gpu_spmm_raw_f64(handle, dA.rowPtr, dA.colInd, dA.values, dA.nnz, dB.rowPtr, dB.colInd, dB.values,
                                              dB.nnz, A.rows, A.cols, B.cols)
        try:
            two = take(hs.rmcl_prune_raw_f64(handle, A.rows, ic, jc, vc, nnz=nnz), A.rows, B.cols)
        finally:
            for p in (ic, jc, vc):
                hs.dev_free(p)
    finally:
        dA.deviceDispose()
        dB.deviceDispose()
    gv, wv = assert_structure(one, two, name)
    assert np.all(np.abs(gv - wv) <= 2.0 * step.bound * wv)


# ---- 4. the loop -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loop_case():
    M = case("graph")[0]
    final, steps = loop64(M, M, 3)
    return M, final, steps, 3 * max(s.bound for s in steps)


def device_loop(handle, M, iters, dtype=F64):
    dM = hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols, dtype=dtype).toGpuCSR()
    try:
        dOut = hs.gpuRmclIter_device(iters, dM, dM, handle)
        assert dOut.dtype == dtype
        try:
            return dOut.toCpuCSR(), dM.toCpuCSR()
        finally:
            dOut.deviceDispose()
    finally:
        dM.deviceDispose()


def test_loop_f64(handle):
    M, final, steps, bound = loop_case()
    precondition(steps, bound, "loop")
    for s in steps:
        assert len(strict_subset_rows(s, 2, 1 << 30)) > 0
    got, back = device_loop(handle, M, 3)
    assert np.array_equal(back.values, M.values) and np.array_equal(back.colInd, M.colInd) and np.array_equal(back.rowPtr, M.rowPtr)
    assert_step(got, final, bound, "loop of 3")
    copy, _ = device_loop(handle, M, 0)                             # maxIter = 0: a copy
    assert np.array_equal(copy.rowPtr, M.rowPtr) and np.array_equal(copy.colInd, M.colInd) and np.array_equal(copy.values, M.values)
    # host arrays in, malloc()ed arrays out: the device loop's structure, values within twice the bound
    hM = hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols, dtype=F64)
    keep = (hM.rowPtr.copy(), hM.colInd.copy(), hM.values.copy())
    host = hs.gpuRmclIter(3, hM, hM)
    assert host.values.dtype == F64
    assert all(np.array_equal(x, y) for x, y in zip(keep, (hM.rowPtr, hM.colInd, hM.values)))
    gv, wv = assert_structure(host, got, "host loop")
    assert np.all(np.abs(gv - wv) <= 2.0 * bound * wv)


# ---- 5. not float in disguise --------------------------------------------------------------------------------------------
def test_loop_f64_is_not_the_float_loop(handle):
    M, final, steps, bound = loop_case()
    got32, _ = device_loop(handle, M, 3, np.float32)
    same = np.array_equal(got32.rowPtr, final.rowPtr)
    if same:
        gc, gv = sorted_rows(got32.rowPtr, got32.colInd, got32.values.astype(F64))
        wc, wv = sorted_rows(final.rowPtr, final.colInd, final.values)
        same = np.array_equal(gc, wc) and bool(np.all(np.abs(gv - wv) <= bound * wv))
    assert not same, "the float loop meets the f64 bound: the test has no teeth"


# ---- 6. end to end in double: file -> loop -> clusters -------------------------------------------------------------------
def test_file_to_clusters_f64(handle):
    dM = hs.read_edge_file(os.path.join(DATA, "own_graph.snap"), True, hs.COO_SELF_LOOPS | hs.COO_ROW_NORMALISE, handle, dtype=F64)
    try:
        h = dM.toCpuCSR()
        M = Host64(h.rowPtr, h.colInd, h.values, h.rows, h.cols)
        final, steps = loop64(M, M, 3)
        bound = 3 * max(s.bound for s in steps)
        precondition(steps, bound, "own_graph")
        want = cr.rmcl_clusters(final.rowPtr, final.colInd, final.values)
        # the attractor of every row is decided by more than the bound (or by the tie rule on equal bits on both sides)
        for i in range(final.rows):
            v = np.sort(final.values[final.rowPtr[i]:final.rowPtr[i + 1]])
            assert len(v) < 2 or v[-1] == v[-2] or v[-1] - v[-2] > 1000.0 * bound * v[-1], f"row {i}: attractor too close to call"
        dOut = hs.gpuRmclIter_device(3, dM, dM, handle)
        try:
            assert dOut.dtype == F64
            cl = hs.rmcl_clusters(dOut, handle)
            try:
                got = (cl.k,) + cl.to_host()
            finally:
                cl.dispose()
        finally:
            dOut.deviceDispose()
    finally:
        dM.deviceDispose()
    k, cluster, ptr, members = got
    assert k == want[0] and np.array_equal(cluster, want[1]) and np.array_equal(ptr, want[2]) and np.array_equal(members, want[3])


# ---- 7. error path ---------------------------------------------------------------------------------------------------
def test_fused_step_after_a_forced_failure(handle):
    A, B, step = case("folded")
    dA, dB = dev(A), dev(B)
    try:
        handle.fail_next(1)
        o = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        n = C.c_int(7)
        rc = hs.lib().hip_rmcl_expand_prune_f64(handle.ptr, C.c_void_p(dA.rowPtr), C.c_void_p(dA.colInd), C.c_void_p(dA.values),
                                                dA.nnz, C.c_void_p(dB.rowPtr), C.c_void_p(dB.colInd), C.c_void_p(dB.values),
                                                dB.nnz, A.rows, A.cols, B.cols, *[C.byref(x) for x in o], C.byref(n))
        assert rc == 6 and b"forced failure" in hs.lib().spgemm_hip_last_error()          # SPGEMM_ERR_INTERNAL
        assert [x.value for x in o] == [None, None, None] and n.value == 0
    finally:
        dA.deviceDispose()
        dB.deviceDispose()
    assert_step(fused(handle, A, B), step.kept, step.bound, "after a forced failure")
