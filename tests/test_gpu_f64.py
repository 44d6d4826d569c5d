"""GPU: double-precision SpGEMM (hip_gpuSpMM_f64 and its twins) against the float64 reference of f64ref.py.

Values: |x - ref| <= 2 * N * 2^-53 * S per entry (N terms, S = sum of their magnitudes).  Structure: rowPtr bit-equal and
per-row-sorted colInd bit-equal to the float32 oracle on the same pattern (the structure depends on the pattern only)."""
import ctypes as C

import numpy as np
import pytest

from f64ref import Host64, bound_violations, sorted_rows, spgemm_f64
from helpers import po, synth_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    if hs.device_count() < 1:
        pytest.fail("GPU test without a HIP device")
    return hs.Handle(0)


def as64(M, values=None):
    v = np.asarray(M.values if values is None else values, np.float64)
    return Host64(M.rowPtr, M.colInd, v, M.rows, M.cols)


def as32(M):
    return po.CSRHost(M.rowPtr, M.colInd, np.asarray(M.values, np.float32), M.rows, M.cols)


def to_hs(M, dtype=np.float64):
    return hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols, dtype=dtype)


def gpu_mul(A, B, handle, dtype=np.float64, sort=False):
    dA = to_hs(A, dtype).toGpuCSR()
    dB = dA if B is A else to_hs(B, dtype).toGpuCSR()
    try:
        dC = hs.gpuSpMMWrapper(dA, dB, handle)
        assert dC.dtype == dtype
        if sort:
            hs.sort_rows_device(dC, handle)
        out = dC.toCpuCSR()
        dC.deviceDispose()
        return out
    finally:
        dA.deviceDispose()
        if dB is not dA:
            dB.deviceDispose()


def check_f64(got, A, B, what=""):
    """got (float64 host CSR) against the float64 reference and the float32 oracle's structure"""
    assert got.values.dtype == np.float64, what
    ref = spgemm_f64(A, B)
    want32 = po.sequential_spmm(as32(A), as32(B)).canonical()
    assert np.array_equal(np.asarray(got.rowPtr), want32.rowPtr), f"{what}: rowPtr"
    assert np.array_equal(np.asarray(got.rowPtr), ref.rowPtr), f"{what}: rowPtr vs float64 reference"
    gc, gv = sorted_rows(got.rowPtr, got.colInd, got.values)
    assert np.array_equal(gc, want32.colInd), f"{what}: sorted colInd"
    bad = bound_violations(gv, ref)
    assert len(bad) == 0, f"{what}: {len(bad)} values beyond the f64 bound, first {gv[bad[0]]!r} vs {ref.values[bad[0]]!r}"
    return ref


def rows_csr(rows_cols, ncols, seed, signed=True):
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(rows_cols) + 1, np.int32)
    np.cumsum([len(c) for c in rows_cols], out=rp[1:])
    ci = np.concatenate([np.asarray(c, np.int32) for c in rows_cols]) if len(rows_cols) else np.zeros(0, np.int32)
    v = rng.random(len(ci)) + 0.5
    if signed:
        v *= rng.choice(np.array([-1.0, 1.0]), size=len(ci))
    return Host64(rp, ci, v, len(rows_cols), ncols)


def random64(rows, cols, density, seed, sorted_rows_=False):
    rng = np.random.default_rng(seed)
    mask = rng.random((rows, cols)) < density
    rp = np.zeros(rows + 1, np.int32)
    np.cumsum(mask.sum(axis=1), out=rp[1:])
    ci = np.nonzero(mask)[1].astype(np.int32)
    v = (rng.random(len(ci)) + 0.25) * rng.choice(np.array([-1.0, 1.0]), size=len(ci))
    if not sorted_rows_:
        for i in range(rows):
            p = rng.permutation(rp[i + 1] - rp[i]) + rp[i]
            ci[rp[i]:rp[i + 1]] = ci[p]
            v[rp[i]:rp[i + 1]] = v[p]
    return Host64(rp, ci, v, rows, cols)


# ---- 1. the f64 path is not float in disguise --------------------------------------------------------------------
def test_precision_beyond_float(handle):
    """Every entry sums 1.0, many terms of ~1e-9 and -1.0 (cancellation): float32 loses the small terms."""
    rng = np.random.default_rng(3)
    m, k, n = 64, 300, 8
    A_rows, vals = [], []
    for _ in range(m):
        cols = rng.permutation(k)
        A_rows.append(cols)
        v = 1e-9 * (1.0 + rng.random(k)) * rng.choice([-1.0, 1.0], size=k)
        v[0], v[1] = 1.0, -1.0                              # the big pair cancels; the sum is carried by the small terms
        vals.append(v)
    A = rows_csr(A_rows, k, 1)
    A = Host64(A.rowPtr, A.colInd, np.concatenate(vals), m, k)
    B = rows_csr([np.arange(n)] * k, n, 2, signed=False)
    B = Host64(B.rowPtr, B.colInd, np.ones(B.nnz), k, n)
    got = gpu_mul(A, B, handle)
    ref = check_f64(got, A, B, "precision")
    g32 = gpu_mul(A, B, handle, dtype=np.float32)
    _, v32 = sorted_rows(g32.rowPtr, g32.colInd, g32.values)
    assert len(bound_violations(v32.astype(np.float64), ref)) > 0, "the float path meets the f64 bound: test has no teeth"


# ---- 2. bins and degenerate shapes -------------------------------------------------------------------------------
def test_every_bin_boundary_f64(handle):
    edges = [0, 1, 2, 4, 5, 16, 17, 64, 65, 512, 513, 4096, 4097]
    n = 9000
    lens = sorted(set(edges))
    B = rows_csr([np.arange(l, dtype=np.int32) * 2 % n if l else [] for l in lens], n, 5)
    A = rows_csr([[lens.index(e)] for e in edges] + [[lens.index(2)]], len(lens), 6)
    got = gpu_mul(A, B, handle)
    assert list(np.diff(got.rowPtr))[:len(edges)] == edges
    check_f64(got, A, B, "bin-edges")
    # the same products folded onto few columns: every bin through its hash table
    Bf = rows_csr([np.arange(l, dtype=np.int32) % 7 if l else [] for l in lens], n, 7)
    check_f64(gpu_mul(A, Bf, handle), A, Bf, "bin-edges folded")


def test_zero_products_and_degenerate_inputs(handle):
    A = Host64([0, 2, 3], [1, 2, 1], [1.0, 2.0, 3.0], 2, 3)
    B = Host64([0, 1, 1, 1], [0], [5.0], 3, 4)
    got = gpu_mul(A, B, handle)
    assert got.nnz == 0 and list(got.rowPtr) == [0, 0, 0]
    E = Host64(np.zeros(1), np.zeros(0), np.zeros(0), 0, 5)      # m = 0
    B5 = rows_csr([[0, 1]] * 5, 3, 1)
    got = gpu_mul(E, B5, handle)
    assert got.nnz == 0 and list(got.rowPtr) == [0]
    Z = Host64(np.zeros(4), np.zeros(0), np.zeros(0), 3, 5)      # nnz = 0
    got = gpu_mul(Z, B5, handle)
    assert got.nnz == 0 and list(got.rowPtr) == [0, 0, 0, 0]


# ---- 3. big rows: one-pass LDS, multi-pass LDS and device-memory tables ------------------------------------------
def test_big_rows_multi_window_f64(handle):
    rng = np.random.default_rng(7)
    k, n = 3000, 700000
    B = rows_csr([np.sort(rng.choice(n, size=int(rng.integers(40, 120)), replace=False)) for _ in range(k)], n, 1)
    A = rows_csr([rng.choice(k, size=s, replace=False) for s in (400, 90, 1, 0, 700, 64, 65, 2500)], k, 2)
    got = gpu_mul(A, B, handle)
    assert np.diff(got.rowPtr).max() > 18432
    check_f64(got, A, B, "big-rows")


def test_big_rows_wider_than_lds_f64(handle):
    rng = np.random.default_rng(17)
    k, n = 4000, 2500000
    B = rows_csr([np.sort(rng.choice(n, size=int(rng.integers(30, 90)), replace=False)) for _ in range(k)], n, 5)
    A = rows_csr([rng.choice(k, size=s, replace=False) for s in (120, 300, 0, 1100, 75, 3900)], k, 6)
    got = gpu_mul(A, B, handle)
    assert np.diff(got.rowPtr).max() > 16 * 10240          # beyond the multi-pass LDS kernel: device-memory tables
    check_f64(got, A, B, "wide big rows")


def test_duplicate_columns_inside_A_and_B_rows_f64(handle):
    rng = np.random.default_rng(5)
    k, n = 2000, 300000
    brows = []
    for _ in range(k):
        c = rng.integers(0, n, size=int(rng.integers(5, 80)))
        brows.append(np.concatenate([c, c[:len(c) // 3]]))
    B = rows_csr(brows, n, 1)
    arows = []
    for s_ in (3, 10, 40, 100, 300, 900, 1800):
        c = rng.choice(k, size=s_, replace=False)
        arows.append(np.concatenate([c, c[:s_ // 4]]))
    arows += [rng.choice(k, size=int(rng.integers(1, 30)), replace=False) for _ in range(500)]
    A = rows_csr(arows, k, 2)
    got = gpu_mul(A, B, handle)
    assert np.diff(got.rowPtr).max() > 4096
    check_f64(got, A, B, "duplicates")


def test_long_A_rows_and_empty_B_rows_f64(handle):
    rng = np.random.default_rng(11)
    k, n = 6000, 5000
    lens = rng.integers(0, 4, size=k)
    lens[rng.integers(0, k, size=50)] = 300
    B = rows_csr([np.sort(rng.choice(n, size=int(l), replace=False)) for l in lens], n, 3)
    A = rows_csr([rng.choice(k, size=s, replace=False) for s in (3000, 1500, 700, 130, 66, 20, 5800)], k, 4)
    check_f64(gpu_mul(A, B, handle), A, B, "long A rows")


# ---- 4. random shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_random_rectangular_unsorted_f64(handle, seed):
    rng = np.random.default_rng(100 + seed)
    r, k, c = (int(x) for x in rng.integers(1, 400, size=3))
    A = random64(r, k, float(rng.uniform(0.0, 0.2)), seed)
    B = random64(k, c, float(rng.uniform(0.0, 0.2)), seed + 50)
    check_f64(gpu_mul(A, B, handle), A, B, f"rand{seed}")


# ---- 5. exact identities ------------------------------------------------------------------------------------------
def test_identity_exact_f64(handle):
    S = synth_csr(262144, 42, 2)
    rng = np.random.default_rng(9)
    v = S.values.astype(np.float64) * (1.0 + rng.random(S.nnz) * 2.0 ** -30)       # not representable in float32
    assert np.any(v.astype(np.float32).astype(np.float64) != v)
    A = as64(S, v)
    m = A.rows
    Id = Host64(np.arange(m + 1), np.arange(m), np.ones(m), m, m)
    want_c, want_v = sorted_rows(A.rowPtr, A.colInd, A.values)
    for got in (gpu_mul(A, Id, handle), gpu_mul(Id, A, handle)):
        assert np.array_equal(got.rowPtr, A.rowPtr)
        gc, gv = sorted_rows(got.rowPtr, got.colInd, got.values)
        assert np.array_equal(gc, want_c) and np.array_equal(gv, want_v)


# ---- 6. two phases ------------------------------------------------------------------------------------------------
def test_two_phase_f64(handle):
    A = random64(300, 250, 0.08, 21)
    B = random64(250, 280, 0.08, 22)
    one = gpu_mul(A, B, handle, sort=True)
    dA, dB = to_hs(A).toGpuCSR(), to_hs(B).toGpuCSR()
    IC = hs.dev_alloc(4 * (A.rows + 1))
    JC = VC = J32 = V32 = 0
    try:
        nnz = hs.spgemm_symbolic_raw(handle, dA.rowPtr, dA.colInd, A.nnz, dB.rowPtr, dB.colInd, B.nnz, A.rows, A.cols,
                                     B.cols, IC)
        assert nnz == one.nnz
        JC, VC = hs.dev_alloc(4 * nnz), hs.dev_alloc(8 * nnz)
        hs.spgemm_numeric_raw_f64(handle, dA.rowPtr, dA.colInd, dA.values, A.nnz, dB.rowPtr, dB.colInd, dB.values, B.nnz,
                                  A.rows, A.cols, B.cols, IC, JC, VC)
        two = hs.CSR(VC, JC, IC, A.rows, B.cols, nnz, True, dtype=np.float64)
        hs.sort_rows_device(two, handle)
        h2 = two.toCpuCSR()
        assert np.array_equal(h2.rowPtr, one.rowPtr) and np.array_equal(h2.colInd, one.colInd)
        check_f64(h2, A, B, "two-phase")
        # the same symbolic phase followed by the float numeric phase: the same structure
        d32A, d32B = to_hs(A, np.float32).toGpuCSR(), to_hs(B, np.float32).toGpuCSR()
        try:
            nnz2 = hs.spgemm_symbolic_raw(handle, dA.rowPtr, dA.colInd, A.nnz, dB.rowPtr, dB.colInd, B.nnz, A.rows,
                                          A.cols, B.cols, IC)
            J32, V32 = hs.dev_alloc(4 * nnz2), hs.dev_alloc(4 * nnz2)
            hs.spgemm_numeric_raw(handle, d32A.rowPtr, d32A.colInd, d32A.values, A.nnz, d32B.rowPtr, d32B.colInd,
                                  d32B.values, B.nnz, A.rows, A.cols, B.cols, IC, J32, V32)
            f32 = hs.CSR(V32, J32, IC, A.rows, B.cols, nnz2, True, dtype=np.float32)
            hs.sort_rows_device(f32, handle)
            h32 = f32.toCpuCSR()
            assert np.array_equal(h32.rowPtr, one.rowPtr) and np.array_equal(h32.colInd, one.colInd)
        finally:
            d32A.deviceDispose()
            d32B.deviceDispose()
        # numeric without a symbolic phase on the handle
        rc = hs.lib().hip_spgemm_numeric_f64(handle.ptr, C.c_void_p(dA.rowPtr), C.c_void_p(dA.colInd), C.c_void_p(dA.values),
                                             A.nnz, C.c_void_p(dB.rowPtr), C.c_void_p(dB.colInd), C.c_void_p(dB.values),
                                             B.nnz, A.rows, A.cols, B.cols, C.c_void_p(IC), C.c_void_p(JC), C.c_void_p(VC))
        assert rc == 2
    finally:
        for p in (IC, JC, VC, J32, V32):
            hs.dev_free(p)
        dA.deviceDispose()
        dB.deviceDispose()


# ---- 7. host arrays in / out --------------------------------------------------------------------------------------
def test_host_api_f64(handle):
    A = random64(500, 400, 0.03, 31)
    B = random64(400, 450, 0.03, 32)
    hA, hB = to_hs(A), to_hs(B)
    got = hA.hip_spmm(hB)                                   # malloc()ed outputs, free()d by the wrapper
    assert got.values.dtype == np.float64
    dev = gpu_mul(A, B, handle)
    gc, gv = sorted_rows(got.rowPtr, got.colInd, got.values)
    dc, dv = sorted_rows(dev.rowPtr, dev.colInd, dev.values)
    assert np.array_equal(got.rowPtr, dev.rowPtr) and np.array_equal(gc, dc)
    check_f64(got, A, B, "host api")
    ref = spgemm_f64(A, B)
    assert np.all(np.abs(gv - dv) <= 4.0 * ref.nterms * 2.0 ** -53 * ref.absSum)
    st = hs.HostApiStats()
    assert hs.lib().spgemm_hip_host_api_stats(C.byref(st)) == 0
    assert st.bytes_d2h == 4 * (A.rows + 1) + 12 * got.nnz


# ---- 8. row sort --------------------------------------------------------------------------------------------------
def test_sort_rows_f64(handle):
    rng = np.random.default_rng(41)
    n = 50000
    A = rows_csr([rng.permutation(n)[:s] for s in (3, 100, 4096, 4097, 9000, 0, 20000)], n, 42)
    dA = to_hs(A).toGpuCSR()
    try:
        hs.sort_rows_device(dA, handle)
        got = dA.toCpuCSR()
    finally:
        dA.deviceDispose()
    want_c, want_v = sorted_rows(A.rowPtr, A.colInd, A.values)
    assert np.array_equal(got.colInd, want_c) and np.array_equal(got.values, want_v)   # values travel with their columns


# ---- 9. stats -----------------------------------------------------------------------------------------------------
def test_stats_match_the_float_call(handle):
    A = synth_csr(65536, 17, 2)
    gpu_mul(A, A, handle, dtype=np.float32)
    s32 = handle.stats()
    gpu_mul(as64(A), as64(A), handle)
    s64 = handle.stats()
    for key in ("total_flops", "nnzC", "bin_rows"):
        assert s64[key] == s32[key], key
    assert s64["ms_numeric"] > 0 and s64["ms_total"] >= s64["ms_numeric"]


# ---- 10. the bench headline matrix in f64 -------------------------------------------------------------------------
def test_full_size_headline_f64(handle):
    S = synth_csr(1 << 20, 43, 2)
    A64 = as64(S)
    dA32 = to_hs(S, np.float32).toGpuCSR()
    dA64 = to_hs(A64).toGpuCSR()
    try:
        c32 = hs.gpuSpMMWrapper(dA32, dA32, handle)
        c64 = hs.gpuSpMMWrapper(dA64, dA64, handle)
        for c in (c32, c64):
            hs.sort_rows_device(c, handle)
        h32, h64 = c32.toCpuCSR(), c64.toCpuCSR()
        c32.deviceDispose()
        c64.deviceDispose()
    finally:
        dA32.deviceDispose()
        dA64.deviceDispose()
    assert np.array_equal(h64.rowPtr, h32.rowPtr)
    assert np.array_equal(h64.colInd, h32.colInd)
    v32 = h32.values.astype(np.float64)
    assert np.all(np.abs(h64.values - v32) <= 1e-6 * np.maximum(np.abs(h64.values), np.abs(v32)))
    # 4096 sampled rows against the float64 reference
    rng = np.random.default_rng(5)
    rows = np.sort(rng.choice(S.rows, size=4096, replace=False))
    rp = np.asarray(S.rowPtr, np.int64)
    lens = rp[rows + 1] - rp[rows]
    sub_rp = np.zeros(len(rows) + 1, np.int32)
    np.cumsum(lens, out=sub_rp[1:])
    idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows])
    Asub = Host64(sub_rp, S.colInd[idx], A64.values[idx], len(rows), S.cols)
    ref = spgemm_f64(Asub, A64)
    crp = np.asarray(h64.rowPtr, np.int64)
    cidx = np.concatenate([np.arange(crp[r], crp[r + 1]) for r in rows])
    assert np.array_equal(h64.colInd[cidx], ref.colInd)
    assert len(bound_violations(h64.values[cidx], ref)) == 0
