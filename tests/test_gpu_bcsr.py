"""GPU (-m gpu): the blocked CSR -- hip_csr_to_bcsr, hip_bcsr_to_csr and their _f64 twins -- against the restatement
tests/bcsr_ref.py (pinned by hand in tests/test_bcsr_abi.py).  Both directions move values and compute nothing, so every
comparison is on bits: rowPtr, colInd and the value bytes, tile order and in-row order included; float64 values carry
bits beyond float32 (x + 2^-40), so a pass through float would show.  The last tests run the reference's tests/BCSR_test.cc
scenarios through the C++ mirror and through the Python BCSR class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bcsr_ref as br
import reorder_ref as rr
from devcsr import built_gpu, handle  # noqa: F401
from devcsr import _plain, _special, _strided_tiles, assert_bits, one_long_row, take, typed, with_nnz
from helpers import ROOT, random_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
ERR_OVERFLOW, ERR_INPUT = 3, 5
CP_TILE = 1024          # entries per block of the key kernel (csr_common_device.hpp, bcsr_device.hpp)
RS_TILE = 2048          # keys per block of the radix kernels (csr_common_device.hpp)
SHAPES = [(1, 1), (2, 2), (3, 5), (64, 64), (1, 4096), (4096, 1)]


# ---- inputs (made once, never modified) ------------------------------------------------------------------------------
# this format's own edge: the tile boundaries b * c (pcsr: its block stride; mcsr: the corner's last column)
def boundary_columns(rows, n, c):
    """every row holds the columns b * c - 1 and b * c for each b: the last column of one block and the first of the
    next, in descending order"""
    cols = np.array([x for b in range(1, (n + c - 1) // c) for x in (b * c - 1, b * c) if x < n][::-1], np.int32)
    rp = np.arange(rows + 1, dtype=np.int32) * len(cols)
    v = (np.arange(rows * len(cols)) % 97 + 1).astype(np.float32)
    return rr.Host(rp, np.tile(cols, rows), v, rows, n)


# per format: the second member is this format's parameter list (tile shapes; pcsr: block counts)
def _cases():
    """name -> (matrix, tile shapes)"""
    out = {"0x0": (rr.Host(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 0, 0), SHAPES),
           "5x7 empty": (rr.Host(np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 7), SHAPES),
           "1000x257": (_plain(random_csr(1000, 257, 0.02, 1, sorted_rows=False)), SHAPES),
           "257x1000": (_plain(random_csr(257, 1000, 0.02, 2, sorted_rows=False)), SHAPES),
           "long row": (one_long_row(), SHAPES)}
    for nnz in (CP_TILE - 1, CP_TILE, CP_TILE + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1):
        out[f"nnz {nnz}"] = (with_nnz(61, 97, nnz, nnz), SHAPES)
    out["7x5 in one ragged 16x16 tile"] = (_plain(random_csr(7, 5, 0.6, 3, sorted_rows=False)), [(16, 16)])
    for r, c in ((2, 2), (3, 5), (1, 64)):
        out[f"boundary columns c={c}"] = (boundary_columns(50, 200, c), [(r, c)])
    return out


CASES = _cases()
REPEATS = ["long row"] + [f"nnz {x}" for x in (CP_TILE + 1, RS_TILE + 1)]


# per format: what is downloaded and the restatement's type differ (here bcsr_ref.Blocked)
def downloaded(b):
    """the three arrays of a hs.BCSR as a bcsr_ref.Blocked"""
    return br.Blocked(hs.d2h(b.rowPtr, b.bm + 1, np.int32), hs.d2h(b.colInd, b.nnzb, np.int32),
                      hs.d2h(b.values, b.nnzb * b.r * b.c, b.dtype), b.m, b.n, b.r, b.c, b.nnz)


def assert_blocked_bits(got, want, what):
    assert (got.m, got.n, got.r, got.c, got.bm, got.bn, got.nnz) == (want.m, want.n, want.r, want.c, want.bm, want.bn, want.nnz), what
    assert np.array_equal(got.rowPtr, want.rowPtr), f"{what}: block rowPtr"
    assert np.array_equal(got.colInd, want.colInd), f"{what}: block columns"
    assert got.values.dtype == want.values.dtype and got.values.tobytes() == want.values.tobytes(), f"{what}: value bits"


# ---- forward and inverse ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_both_directions_match_the_restatement(handle, name, dtype):
    M0, shapes = CASES[name]
    M = typed(M0, dtype)
    dM = M.toGpuCSR()
    try:
        for r, c in shapes:
            what = f"{name} r={r} c={c}"
            want = br.to_bcsr(M, r, c)
            b = hs.BCSR(dM, r, c, handle)
            try:
                assert (b.m, b.n, b.r, b.c, b.bm, b.bn, b.nnz, b.nnzb) == (M.rows, M.cols, r, c, want.bm, want.bn, M.nnz, want.nnzb), what
                assert_blocked_bits(downloaded(b), want, what + ": forward")
                assert b.nonzero_density() == br.density(want)
                assert_bits(take(b.to_csr(1e-9, handle)), br.to_csr(want, 1e-9), what + ": inverse")
            finally:
                b.dispose()
    finally:
        dM.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", REPEATS)
def test_repeated_columns_give_the_same_bytes_twice(handle, name, dtype):
    M = typed(CASES[name][0], dtype)
    dM = M.toGpuCSR()
    try:
        for r, c in ((1, 1), (3, 5), (64, 64)):
            runs = []
            for _ in range(2):
                b = hs.BCSR(dM, r, c, handle)
                got = downloaded(b)
                back = take(b.to_csr(0.0, handle))
                b.dispose()
                runs.append((got.rowPtr.tobytes(), got.colInd.tobytes(), got.values.tobytes(), back.rowPtr.tobytes(),
                             back.colInd.tobytes(), back.values.tobytes()))
            assert runs[0] == runs[1], f"{name} r={r} c={c}"
    finally:
        dM.deviceDispose()


# ---- bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_keep_their_bits_and_the_tolerance_is_applied_in_double(handle, dtype):
    sp = _special(dtype)
    # what the contract says of each value, from the number formats alone
    assert np.isnan(sp["nan"]) and float(sp["denormal"]) > 0.0 and float(sp["1e-9"]) <= 1e-9 < float(sp["above"])
    names = list(sp)
    rows, cols = 9, 11
    rng = np.random.default_rng(5)
    rp, ci, v, kind = [0], [], [], []
    for i in range(rows):
        js = rng.permutation(cols)[:7]
        for q, j in enumerate(js):
            ci.append(int(j))
            k = names[(i + q) % 5] if q < 5 else "plain"
            kind.append(k)
            v.append(sp[k] if k != "plain" else np.dtype(dtype).type(1.5 + i))
        rp.append(len(ci))
    M = hs.CSR.from_arrays(rp, ci, np.array(v, dtype), rows, cols, dtype=dtype)
    kind = np.array(kind)
    dM = M.toGpuCSR()
    try:
        for r, c in ((1, 1), (2, 2), (3, 5)):
            want = br.to_bcsr(M, r, c)
            b = hs.BCSR(dM, r, c, handle)
            try:
                got = downloaded(b)
                assert_blocked_bits(got, want, f"special r={r} c={c}")
                # forward keeps all of them: every source value's bits are in the tiles
                have = set(got.values.view(np.uint32 if np.dtype(dtype) == np.float32 else np.uint64).tolist())
                assert set(M.values.view(np.uint32 if np.dtype(dtype) == np.float32 else np.uint64).tolist()) <= have
                for tol, dropped in ((1e-9, {"nan", "-0", "denormal", "1e-9"}), (0.0, {"nan", "-0"})):
                    back = take(b.to_csr(tol, handle))
                    assert_bits(back, br.to_csr(want, tol), f"special r={r} c={c} tol={tol}")
                    keep = ~np.isin(kind, list(dropped))
                    row_of = np.repeat(np.arange(rows), np.diff(M.rowPtr))
                    survivors = rr.sort_rows(rr.Host(np.concatenate([[0], np.cumsum(np.bincount(row_of[keep], minlength=rows))]),
                                                     M.colInd[keep], M.values[keep], rows, cols))
                    assert_bits(rr.sort_rows(back), survivors, f"special r={r} c={c} tol={tol}: exactly those are dropped")
            finally:
                b.dispose()
    finally:
        dM.deviceDispose()


# ---- round trip ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["1000x257", "257x1000", "7x5 in one ragged 16x16 tile"])
def test_round_trip_of_a_sorted_matrix_is_the_matrix(handle, name, dtype):
    S = typed(rr.sort_rows(CASES[name][0]), dtype)
    dS = S.toGpuCSR()
    raw = hs.csr_diff_raw_f64 if np.dtype(dtype) == np.float64 else hs.csr_diff_raw
    try:
        for r, c in SHAPES:
            b = hs.BCSR.from_csr(dS, r, c, handle)
            back = b.to_csr(1e-9, handle)
            try:
                hs.sort_rows_device(back, handle)
                d = raw(handle, S.rows, S.cols, back.rowPtr, back.colInd, back.values, back.nnz, dS.rowPtr, dS.colInd, dS.values,
                        dS.nnz, 0.0, 0.0)
                assert (d.rows_len_differ, d.only_a, d.only_b, d.beyond) == (0, 0, 0, 0), (r, c, d.as_dict())
                assert_bits(back.toCpuCSR(), S, f"{name} r={r} c={c}: sort_rows(to_csr(to_bcsr(A)))")
            finally:
                back.deviceDispose()
                b.dispose()
    finally:
        dS.deviceDispose()


# ---- bad input -------------------------------------------------------------------------------------------------------
def test_bad_input_is_an_error_not_a_fault(handle):
    L = hs.lib()
    M = typed(CASES["1000x257"][0], np.float32)
    dM = M.toGpuCSR()
    m, n, r, c = M.rows, M.cols, 3, 5
    good = br.to_bcsr(M, r, c)
    good_back = br.to_csr(good, 1e-9)
    dev = hs.BCSR(dM, r, c, handle)
    ups = []

    def forward_rc(IA, JA, VA, rows, cols, nnz, tr=r, tc=c):
        o = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        cnt = C.c_int(9)
        rc = L.hip_csr_to_bcsr(handle.ptr, rows, cols, nnz, C.c_void_p(IA), C.c_void_p(JA), C.c_void_p(VA), tr, tc,
                               *[C.byref(x) for x in o], C.byref(cnt))
        return rc, [x.value for x in o] + [cnt.value], L.spgemm_hip_last_error()

    def inverse_rc(IB, JB, nnzb):
        o = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        cnt = C.c_int(9)
        rc = L.hip_bcsr_to_csr(handle.ptr, m, n, r, c, nnzb, C.c_void_p(IB), C.c_void_p(JB), C.c_void_p(dev.values), 1e-9,
                               *[C.byref(x) for x in o], C.byref(cnt))
        return rc, [x.value for x in o] + [cnt.value], L.spgemm_hip_last_error()

    def valid_call(what):
        b = hs.BCSR(dM, r, c, handle)
        try:
            assert_blocked_bits(downloaded(b), good, what)
            assert_bits(take(b.to_csr(1e-9, handle)), good_back, what)
        finally:
            b.dispose()

    def refused(call, status, word, what):
        """the error twice from an empty cache: the second call must give back exactly what it took; then a valid call
        on the same handle, and after a trim nothing is left"""
        hs.pool_trim(handle.device)
        rc, outs, msg = call()
        assert rc == status and outs == [None, None, None, 0] and word in msg, (what, rc, outs, msg)
        balance = hs.pool_cached_bytes(handle.device)
        rc, outs, msg = call()
        assert rc == status and outs == [None, None, None, 0], (what, rc, outs, msg)
        assert hs.pool_cached_bytes(handle.device) == balance, what
        valid_call("valid call after " + what)
        hs.pool_trim(handle.device)
        assert hs.pool_cached_bytes(handle.device) == 0, what

    try:
        falling = M.rowPtr.copy()
        falling[500] = falling[499] - 1 if falling[499] > 0 else falling[501] + 1
        ups.append(hs.h2d(falling))
        refused(lambda: forward_rc(ups[0], dM.colInd, dM.values, m, n, M.nnz), ERR_INPUT, b"rowPtr", "a decreasing rowPtr")
        bad_cols = M.colInd.copy()
        bad_cols[7] = n
        ups.append(hs.h2d(bad_cols))
        refused(lambda: forward_rc(dM.rowPtr, ups[1], dM.values, m, n, M.nnz), ERR_INPUT, b"column", "a column equal to n")
        bad_bcols = good.colInd.copy()
        bad_bcols[11] = good.bn
        ups.append(hs.h2d(bad_bcols))
        refused(lambda: inverse_rc(dev.rowPtr, ups[2], dev.nnzb), ERR_INPUT, b"block column", "a block column equal to bn")
        refused(lambda: inverse_rc(dev.rowPtr, dev.colInd, dev.nnzb - 1), ERR_INPUT, b"rowPtr", "a block rowPtr not ending at nnzb")
        # 524 289 tiles of 64 x 64 = 2^31 + 4096 values: known only after the count pass
        side, ntiles = 46400, 524289
        assert ntiles * 4096 > 2 ** 31 - 1 >= (ntiles - 2) * 4096 and ntiles <= ((side + 63) // 64) ** 2
        big = _strided_tiles(ntiles, side, 64)
        ups.extend([hs.h2d(big.rowPtr), hs.h2d(big.colInd), hs.h2d(big.values)])
        refused(lambda: forward_rc(ups[3], ups[4], ups[5], side, side, ntiles, 64, 64), ERR_OVERFLOW, b"int32",
                "more than INT32_MAX tile values")
    finally:
        for ptr in ups:
            hs.dev_free(ptr)
        dev.dispose()
        dM.deviceDispose()


def test_pool_does_not_grow(handle):
    M = typed(CASES["1000x257"][0], np.float64)
    dM = M.toGpuCSR()

    def rounds(k):
        for _ in range(k):
            b = hs.BCSR(dM, 3, 5, handle)
            b.to_csr(1e-9, handle).deviceDispose()
            b.dispose()
    try:
        rounds(20)
        before = hs.pool_cached_bytes(handle.device)
        rounds(5)
        assert hs.pool_cached_bytes(handle.device) == before
    finally:
        dM.deviceDispose()


# ---- the mirrors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_python_bcsr_round_trip_and_is_equal(handle, dtype):
    """the ragged 5 x 5 of the reference's tests/BCSR_test.cc through the Python class: equal to itself, not equal after a
    value changed, not equal with one entry fewer"""
    rp, ci, v = [0, 1, 3, 4, 6, 7], [1, 1, 4, 0, 1, 3, 0], [2, 3, 3, 4, 1, 5, 2]
    A = hs.CSR.from_arrays(rp, ci, v, 5, 5, dtype=dtype)
    changed = hs.CSR.from_arrays(rp, ci, v[:6] + [5], 5, 5, dtype=dtype)
    fewer = hs.CSR.from_arrays([0, 1, 2, 3, 5, 6], ci[:2] + ci[3:], v[:2] + v[3:], 5, 5, dtype=dtype)
    dA, dChanged, dFewer = A.toGpuCSR(), changed.toGpuCSR(), fewer.toGpuCSR()
    b = hs.BCSR.from_csr(dA, 2, 2, handle)
    try:
        assert (b.m, b.n, b.r, b.c, b.bm, b.bn, b.nnzb, b.nnz) == (5, 5, 2, 2, 3, 3, 5, 7)
        assert b.nonzero_density() == 35.0
        got = downloaded(b)
        assert got.rowPtr.tolist() == [0, 2, 4, 5] and got.colInd.tolist() == [0, 2, 0, 1, 0]
        assert got.values.tolist() == [0, 2, 0, 3, 0, 0, 3, 0, 4, 0, 0, 1, 0, 0, 0, 5, 2, 0, 0, 0]
        assert_bits(take(b.to_csr(handle=handle)), A, "5x5: sorted rows come back as they were")
        before = dA.toCpuCSR()
        assert b.is_equal(dA, handle)
        assert_bits(dA.toCpuCSR(), before, "is_equal leaves its argument alone")
        assert not b.is_equal(dChanged, handle)
        assert not b.is_equal(dFewer, handle)
    finally:
        b.dispose()
        for d in (dA, dChanged, dFewer):
            d.deviceDispose()


def test_cpp_mirror_runs_the_blocked_scenarios():
    """tests/cpp/bcsr_check.cc: the two scenarios of the reference's tests/BCSR_test.cc on the C++ mirror"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-B", "-C", cpp, "bcsr_check.x"])
    out = subprocess.run([os.path.join(cpp, "bcsr_check.x")], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    for scenario in ("4x4", "5x5"):
        for check in ("shape", "rowPtr", "colInd", "values", "density", "equal to itself", "not equal after a value changed",
                      "not equal with one entry fewer"):
            assert f"{scenario} {check}: ok" in lines, (scenario, check)
    assert "Pass" in lines and "FAILED" not in out.stdout
