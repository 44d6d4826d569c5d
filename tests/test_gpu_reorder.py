"""GPU (-m gpu): device CSR reordering -- hip_csr_permute (PM / MP / PMPt / PtMP), hip_permutation_transpose,
hip_csr_row_descending_permutation, hip_csr_transpose -- in float32 and float64 against the numpy restatement
tests/reorder_ref.py (pinned to the reference in tests/test_reorder_abi.py).  No arithmetic is involved, so every
comparison is on bits, in-row order included; float64 values carry bits beyond float32 (x + 2^-40), so a pass through
float would show.  The last tests run the reference's ordering experiment (correctTests/permuTest.cc) through the product
path, in Python and through the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import f64ref
import reorder_ref as rr
from devcsr import built_gpu, handle  # noqa: F401
from devcsr import assert_bits, one_long_row, take, typed, typed_plain, with_nnz
from helpers import DATA, ROOT, assert_parity, po, random_csr, synth_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
ERR_INPUT = 5
CP_TILE = 1024          # entries per block of the permute copy / transpose key kernels (csr_common_device.hpp)
RS_TILE = 2048          # keys per block of the radix kernels (csr_common_device.hpp)


# ---- inputs (made once, never modified) ------------------------------------------------------------------------------
def _shapes():
    out = {"0x0": rr.Host(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 0, 0),
           "5x7 empty": rr.Host(np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 7),
           "1000x257": random_csr(1000, 257, 0.02, 1, sorted_rows=False),
           "257x1000": random_csr(257, 1000, 0.02, 2, sorted_rows=False),
           "long row": one_long_row()}
    for nnz in (CP_TILE - 1, CP_TILE, CP_TILE + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1):
        out[f"nnz {nnz}"] = with_nnz(61, 97, nnz, nnz)
    return out


SHAPES = _shapes()


def perms(n, seed):
    """identity, reversal, seeded random"""
    return {"identity": np.arange(n, dtype=np.int32), "reversal": np.arange(n, dtype=np.int32)[::-1].copy(),
            "random": np.random.default_rng(seed).permutation(n).astype(np.int32)}


def permute_raw(handle, dM, rowSrc, colMap):
    ups = [hs.h2d(p) if p is not None else None for p in (rowSrc, colMap)]
    raw = hs.csr_permute_raw_f64 if dM.dtype == np.float64 else hs.csr_permute_raw
    try:
        ib, jb, vb = raw(handle, dM.rows, dM.cols, dM.nnz, dM.rowPtr, dM.colInd, dM.values, ups[0], ups[1])
    finally:
        for p in ups:
            hs.dev_free(p)
    return take(hs.CSR(vb, jb, ib, dM.rows, dM.cols, dM.nnz, True, dtype=dM.dtype))


# ---- permute ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_permute_matches_the_restatement(handle, name, dtype):
    """rowSrc / colMap each NULL or identity / reversal / random: all four combinations of given and NULL"""
    M = typed(SHAPES[name], dtype)
    dM = M.toGpuCSR()
    try:
        assert_bits(permute_raw(handle, dM, None, None), M, f"{name}: deep copy")
        rows, cols = perms(M.rows, 11), perms(M.cols, 12)
        for kind in rows:
            P, Q = rows[kind], cols[kind]
            assert_bits(permute_raw(handle, dM, P, None), rr.PM(M, P), f"{name}: rowSrc {kind}")
            assert_bits(permute_raw(handle, dM, None, Q), rr.MP(M, Q), f"{name}: colMap {kind}")
            assert_bits(permute_raw(handle, dM, P, Q), rr.MP(rr.PM(M, P), Q), f"{name}: both {kind}")
    finally:
        dM.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
def test_csr_methods_host_and_device_resident(handle, dtype):
    M = typed(random_csr(300, 300, 0.03, 5, sorted_rows=False), dtype)
    P = np.random.default_rng(5).permutation(300).astype(np.int32)
    want = {"PM": rr.PM(M, P), "MP": rr.MP(M, P), "PMPt": rr.PMPt(M, P), "PtMP": rr.PtMP(M, P)}
    dM = M.toGpuCSR()
    try:
        for name, w in want.items():
            h = getattr(M, name)(P, handle)
            assert not h.on_device and h.dtype == np.dtype(dtype)
            assert_bits(h, w, name + " host")
            d = getattr(dM, name)(P, handle)
            assert d.on_device and d.dtype == np.dtype(dtype)
            assert_bits(take(d), w, name + " device")
        assert_bits(M.PMPt(P, handle).PtMP(P, handle), M, "PtMP undoes PMPt")
    finally:
        dM.deviceDispose()
    assert np.array_equal(hs.permutation_transpose(P, handle), rr.permutation_transpose(P))


def test_product_with_a_permutation_matrix_is_the_permutation(handle):
    """the reference's own identity (tests/CSR_test.cc:14-29, 41-61) through the device product: Pmat * M == PM(M, P) and
    M * Qmat == MP(M, Q), rows sorted on the device on both sides; one term times 1.0 per entry, so bit-exact"""
    M = typed(SHAPES["1000x257"], np.float32)
    P = np.random.default_rng(21).permutation(M.rows).astype(np.int32)
    Q = np.random.default_rng(22).permutation(M.cols).astype(np.int32)
    dM = M.toGpuCSR()
    dP = typed(rr.perm_matrix(P), np.float32).toGpuCSR()
    dQ = typed(rr.perm_matrix(Q), np.float32).toGpuCSR()
    try:
        for prod, perm in ((hs.gpuSpMMWrapper(dP, dM, handle), dM.PM(P, handle)),
                           (hs.gpuSpMMWrapper(dM, dQ, handle), dM.MP(Q, handle))):
            hs.sort_rows_device(prod, handle)
            hs.sort_rows_device(perm, handle)
            assert_bits(take(prod), take(perm))
    finally:
        for d in (dM, dP, dQ):
            d.deviceDispose()


# ---- permutation helpers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 257, 70001])
def test_permutation_transpose(handle, n):
    P = np.random.default_rng(n).permutation(n).astype(np.int32)
    Pt = hs.permutation_transpose(P, handle)
    assert Pt.dtype == np.int32 and np.array_equal(Pt, rr.permutation_transpose(P))


def _row_lengths():
    rng = np.random.default_rng(3)
    long_row = rng.integers(0, 40, size=257)
    long_row[100] = 70000                                   # above 65 535: a third radix pass
    return {"m=0": np.zeros(0, np.int64), "m=1": np.array([3]), "all equal": np.full(257, 7), "all empty": np.zeros(257, np.int64),
            "two values": rng.choice([2, 9], size=70001), "mixed": rng.integers(0, 300, size=70001),
            "one long row": long_row, "255|256": rng.choice([0, 255, 256], size=5000)}


LENGTHS = _row_lengths()


@pytest.mark.parametrize("name", list(LENGTHS))
def test_row_descending_permutation(handle, name):
    lens = LENGTHS[name]
    rp = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=rp[1:])
    M = hs.CSR(None, None, rp, len(lens), 1, int(rp[-1]))   # only rowPtr is read
    want = rr.row_descending(rp)
    assert np.array_equal(M.rowDescendingOrderPermutation(handle), want), "host resident"
    drp = hs.h2d(rp)
    try:
        D = hs.CSR(None, None, drp, len(lens), 1, int(rp[-1]), on_device=True)
        assert np.array_equal(D.rowDescendingOrderPermutation(handle), want), "device resident"
    finally:
        hs.dev_free(drp)


# ---- transpose -------------------------------------------------------------------------------------------------------
def _transpose_shapes():
    out = dict(SHAPES)
    rng = np.random.default_rng(9)
    wide = with_nnz(64, (1 << 20) + 3, 500, 9)              # 21 column bits: every radix pass, few entries
    wide.colInd[:3] = [(1 << 20) + 2, 0, 1 << 20]
    out["64 x (2^20+3)"] = wide
    inner = random_csr(200, 150, 0.05, 10, sorted_rows=False)
    out["empty first and last column"] = rr.Host(inner.rowPtr, inner.colInd + 1, inner.values, 200, 152)
    out["many rows"] = with_nnz(70001, 300, 5000, 13)       # 17 row bits under the column bits
    del rng
    return out


TSHAPES = _transpose_shapes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(TSHAPES))
def test_transpose_matches_the_stable_restatement(handle, name, dtype):
    M = typed(TSHAPES[name], dtype)
    want = rr.transpose(M)
    T = M.transpose(handle)
    assert (T.rows, T.cols, T.nnz) == (M.cols, M.rows, M.nnz) and not T.on_device
    assert_bits(T, want, name)                              # stability included: repeated columns keep storage order
    rp = np.asarray(M.rowPtr, np.int64)
    row_of = np.repeat(np.arange(M.rows), np.diff(rp))
    if len(np.unique(row_of * max(M.cols, 1) + M.colInd)) == M.nnz:      # no row repeats a column
        dM = M.toGpuCSR()
        try:
            dT = dM.transpose(handle)
            back = dT.transpose(handle)
            dT.deviceDispose()
            assert_bits(take(back), rr.sort_rows(M), name + ": transpose twice = rows sorted")
        finally:
            dM.deviceDispose()


# ---- bad input -------------------------------------------------------------------------------------------------------
def test_bad_input_is_an_error_not_a_fault(handle):
    L = hs.lib()
    M = typed(SHAPES["1000x257"], np.float32)
    dM = M.toGpuCSR()
    m, n = M.rows, M.cols
    good_r, good_c = np.arange(m, dtype=np.int32), np.arange(n, dtype=np.int32)

    def bad(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    def permute_rc(rowSrc, colMap):
        ups = [hs.h2d(p) if p is not None else None for p in (rowSrc, colMap)]
        o = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        rc = L.hip_csr_permute(handle.ptr, m, n, M.nnz, C.c_void_p(dM.rowPtr), C.c_void_p(dM.colInd), C.c_void_p(dM.values),
                               C.c_void_p(ups[0]), C.c_void_p(ups[1]), *[C.byref(x) for x in o])
        for p in ups:
            hs.dev_free(p)
        return rc, [x.value for x in o], L.spgemm_hip_last_error()

    try:
        for rowSrc, colMap, word in ((bad(good_r, 3, 4), None, b"rowSrc"), (bad(good_r, 500, -1), None, b"rowSrc"),
                                     (bad(good_r, 999, m), None, b"rowSrc"), (None, bad(good_c, 0, 5), b"colMap")):
            rc, outs, msg = permute_rc(rowSrc, colMap)
            assert rc == ERR_INPUT and outs == [None, None, None] and word in msg, (rc, outs, msg)
        # a column equal to n handed to the transpose
        dJ = hs.h2d(bad(M.colInd, 7, n))
        o = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        rc = L.hip_csr_transpose(handle.ptr, m, n, M.nnz, C.c_void_p(dM.rowPtr), C.c_void_p(dJ), C.c_void_p(dM.values),
                                 *[C.byref(x) for x in o])
        hs.dev_free(dJ)
        assert rc == ERR_INPUT and [x.value for x in o] == [None, None, None] and b"column" in L.spgemm_hip_last_error()
        # a dP that is no permutation: error, and dPt is not written
        dP, dPt = hs.h2d(bad(good_r, 10, 11)), hs.h2d(np.full(m, -7, np.int32))
        rc = L.hip_permutation_transpose(handle.ptr, m, C.c_void_p(dP), C.c_void_p(dPt))
        untouched = hs.d2h(dPt, m, np.int32)
        hs.dev_free(dP)
        hs.dev_free(dPt)
        assert rc == ERR_INPUT and np.all(untouched == -7)
        with pytest.raises(hs.SpgemmError):
            hs.permutation_transpose(bad(good_r, 10, 11), handle)
        # the handle is still good
        P = good_r[::-1].copy()
        assert_bits(take(dM.PM(P, handle)), rr.PM(M, P), "valid call after the errors")
        assert_bits(take(dM.transpose(handle)), rr.transpose(M), "valid transpose after the errors")
    finally:
        dM.deviceDispose()


def test_device_synchronize_waits_for_a_d2d_copy(handle):
    src = np.arange(1 << 20, dtype=np.int32)
    d_src, d_dst = hs.h2d(src), hs.dev_alloc(src.nbytes)
    try:
        hs.d2d(d_dst, d_src, src.nbytes)
        assert hs.lib().spgemm_hip_device_synchronize() == 0
        hs.device_synchronize()
        assert np.array_equal(hs.d2h(d_dst, len(src), np.int32), src)
    finally:
        hs.dev_free(d_src)
        hs.dev_free(d_dst)


# ---- pool ------------------------------------------------------------------------------------------------------------
def test_pool_does_not_grow(handle):
    M = typed(SHAPES["1000x257"], np.float64)
    P = np.random.default_rng(1).permutation(M.rows).astype(np.int32)
    dM = M.toGpuCSR()

    def rounds(k):
        for _ in range(k):
            dM.PM(P, handle).deviceDispose()
            dM.transpose(handle).deviceDispose()
            dM.rowDescendingOrderPermutation(handle)
    try:
        rounds(20)
        before = hs.pool_cached_bytes(handle.device)
        rounds(5)
        assert hs.pool_cached_bytes(handle.device) == before
    finally:
        dM.deviceDispose()


# ---- the ordering experiment through the product path ----------------------------------------------------------------
@pytest.fixture(scope="module")
def experiment():
    A = synth_csr(4096, 7)
    return A, po.omp_spmm(A, A)


def _permuted_product(A, P, dtype, handle):
    dA = typed_plain(A, dtype).toGpuCSR()
    dAp = dA.PMPt(P, handle)
    dCp = hs.gpuSpMMWrapper(dAp, dAp, handle)
    dC = dCp.PtMP(P, handle)
    for d in (dA, dAp, dCp):
        d.deviceDispose()
    return take(dC)


@pytest.mark.parametrize("order", ["random", "descending"])
def test_product_does_not_depend_on_the_ordering(handle, experiment, order):
    A, want = experiment
    if order == "random":
        P = np.random.default_rng(4096).permutation(A.rows).astype(np.int32)
    else:
        P = typed_plain(A, np.float32).rowDescendingOrderPermutation(handle)
        assert np.array_equal(P, rr.row_descending(A.rowPtr))
    got = _permuted_product(A, P, np.float32, handle)
    assert_parity(got, want, accum=(A, A), what=f"PtMP(PMPt(A)^2), {order} P")


def test_product_does_not_depend_on_the_ordering_f64(handle, experiment):
    A, _ = experiment
    P = np.random.default_rng(4097).permutation(A.rows).astype(np.int32)
    got = _permuted_product(A, P, np.float64, handle)
    A64 = f64ref.Host64(A.rowPtr, A.colInd, A.values, A.rows, A.cols)
    ref = f64ref.spgemm_f64(A64, A64)
    assert np.array_equal(np.asarray(got.rowPtr), ref.rowPtr)
    gc, gv = f64ref.sorted_rows(got.rowPtr, got.colInd, got.values)
    assert np.array_equal(gc, ref.colInd)
    bad = f64ref.bound_violations(gv, ref)
    assert len(bad) == 0, f"{len(bad)} values beyond 2 N 2^-53 S, first {gv[bad[0]]!r} vs {ref.values[bad[0]]!r}"


def test_cpp_mirror_runs_the_ordering_experiment():
    """tests/cpp/permu_check.cc: the flow of the reference's correctTests/permuTest.cc on the C++ mirror"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-B", "-C", cpp, "permu_check.x"])
    out = subprocess.run([os.path.join(cpp, "permu_check.x"), os.path.join(DATA, "own_graph.snap")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Same" in out.stdout and "Diffs" not in out.stdout
