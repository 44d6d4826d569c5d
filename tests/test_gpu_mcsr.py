"""GPU (-m gpu): the mixed CSR -- hip_csr_to_mcsr, hip_mcsr_to_csr and their _f64 twins -- against the restatement
tests/mcsr_ref.py (pinned in tests/test_mcsr_abi.py).  Both directions move values and compute nothing, so every
comparison is on bits: rowPtr, colInd and the value bytes, tile order and in-row order included; float64 values carry
bits beyond float32 (x + 2^-40), so a pass through float would show.  The last tests run the reference's
tests/MCSR_test.cc vectors (tests/golden/mcsr_kat.json) through the Python MCSR class and through the C++ mirror."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import mcsr_ref as mr
import bcsr_ref as br
import reorder_ref as rr
from devcsr import built_gpu, handle  # noqa: F401
from devcsr import _plain, _special, _strided_tiles, assert_bits, one_long_row, take, typed
from helpers import ROOT, random_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
ERR_OVERFLOW, ERR_INPUT = 3, 5
CP_TILE = 1024          # entries per block of the flag / scatter / copy kernels (csr_common_device.hpp, mcsr_device.hpp)
SCAN_TILE = 4096        # ints per block of the library's scan (spgemm_device.hpp; checked against the source below)
RS_TILE = 2048          # keys per block of the radix kernels the corner's tiling runs (csr_common_device.hpp)
TILES = [(1, 1), (2, 2), (3, 5), (64, 64)]


def test_the_tile_sizes_are_the_ones_in_the_code():
    csrc = os.path.join(ROOT, "sparse_matrix_with_flops_amd", "csrc")

    def const(path, name):
        with open(os.path.join(csrc, path)) as f:
            return int(re.search(r"constexpr int (?:\w+ = \w+, )*" + name + r" = (\d+)", f.read()).group(1))
    assert const("spgemm_device.hpp", "SCAN_THREADS") * const("spgemm_device.hpp", "SCAN_ITEMS") == SCAN_TILE
    assert const("csr_common_device.hpp", "CP_THREADS") * const("csr_common_device.hpp", "CP_ITEMS") == CP_TILE
    assert const("csr_common_device.hpp", "RS_THREADS") * const("csr_common_device.hpp", "RS_ITEMS") == RS_TILE


# ---- inputs (made once, never modified) ------------------------------------------------------------------------------
def top_heavy(rows, cols, top_rows, n_top, n_rest, seed):
    """exactly n_top entries over the first top_rows rows and n_rest over the others; random columns (repeats allowed),
    some rows empty"""
    rng = np.random.default_rng(seed)
    owner = np.concatenate([np.sort(rng.integers(0, top_rows, size=n_top)), np.sort(rng.integers(top_rows, rows, size=n_rest))])
    rp = np.zeros(rows + 1, np.int32)
    np.cumsum(np.bincount(owner, minlength=rows), out=rp[1:])
    nnz = n_top + n_rest
    return rr.Host(rp, rng.integers(0, cols, size=nnz), (rng.random(nnz) + 0.25).astype(np.float32), rows, cols)


# this format's own edge: the one boundary between corner and remainder (bcsr, pcsr: every tile / block boundary)
def boundary_columns(rows, n, block_cols):
    """every row holds the columns n - 1, block_cols, block_cols - 1 and 0 in this (descending) order: the first column
    of the remainder stands before the last column of the corner"""
    cols = np.array([n - 1, block_cols, block_cols - 1, 0], np.int32)
    rp = np.arange(rows + 1, dtype=np.int32) * len(cols)
    v = (np.arange(rows * len(cols)) % 97 + 1).astype(np.float32)
    return rr.Host(rp, np.tile(cols, rows), v, rows, n)


EMPTY0 = rr.Host(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 0, 0)
EMPTY57 = rr.Host(np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 7)
TALL = _plain(random_csr(1000, 257, 0.02, 1, sorted_rows=False))
WIDE = _plain(random_csr(257, 1000, 0.02, 2, sorted_rows=False))
MATRICES = {"0x0": EMPTY0, "5x7 empty": EMPTY57, "1000x257": TALL, "257x1000": WIDE}
LONG = one_long_row(400, 300, 192)          # 192 is a multiple of every r in TILES


def corners(m, n, r, c):
    """blockRows in {0, r, the largest multiple of r <= m} x blockCols in {0, 1, c, n // 2, n}, those inside the matrix"""
    rows = sorted({x for x in (0, r, m // r * r) if x <= m})
    cols = sorted({x for x in (0, 1, c, n // 2, n) if x <= n})
    return [(a, b) for a in rows for b in cols]


# per format: what is downloaded and the restatement's type differ (here mcsr_ref.Mixed)
def downloaded(x):
    """the arrays of a hs.MCSR as a mcsr_ref.Mixed"""
    corner = br.Blocked(hs.d2h(x.rowPtr, x.bm + 1, np.int32), hs.d2h(x.colInd, x.nnzb, np.int32),
                        hs.d2h(x.values, x.nnzb * x.r * x.c, x.dtype), x.blockRows, x.blockCols, x.r, x.c, x.nnz)
    return mr.Mixed(corner, x.remainder.toCpuCSR(), x.m, x.n, x.blockRows, x.blockCols)


def assert_mixed_bits(got, want, what):
    g, w = got.corner, want.corner
    assert (got.m, got.n, got.blockRows, got.blockCols) == (want.m, want.n, want.blockRows, want.blockCols), what
    assert (g.m, g.n, g.r, g.c, g.bm, g.bn, g.nnz, g.nnzb) == (w.m, w.n, w.r, w.c, w.bm, w.bn, w.nnz, w.nnzb), what
    assert np.array_equal(g.rowPtr, w.rowPtr), f"{what}: block rowPtr"
    assert np.array_equal(g.colInd, w.colInd), f"{what}: block columns"
    assert g.values.dtype == w.values.dtype and g.values.tobytes() == w.values.tobytes(), f"{what}: tile bits"
    assert_bits(got.rest, want.rest, what + ": remainder")


def all_bytes(got, back):
    return (got.corner.rowPtr.tobytes(), got.corner.colInd.tobytes(), got.corner.values.tobytes(),
            np.asarray(got.rest.rowPtr).tobytes(), np.asarray(got.rest.colInd).tobytes(), np.asarray(got.rest.values).tobytes(),
            np.asarray(back.rowPtr).tobytes(), np.asarray(back.colInd).tobytes(), np.asarray(back.values).tobytes())


def check_both_directions(handle, M, dM, r, c, brows, bcols, what, tol=1e-9):
    want = mr.to_mcsr(M, r, c, brows, bcols)
    x = hs.MCSR(dM, r, c, brows, bcols, handle)
    try:
        assert (x.m, x.n, x.r, x.c, x.blockRows, x.blockCols, x.bm, x.bn) == (M.rows, M.cols, r, c, brows, bcols, brows // r, -(-bcols // c)), what
        assert x.nnzb == want.corner.nnzb and x.nnz == want.corner.nnz and x.remainder.nnz == want.rest.nnz, what
        got = downloaded(x)
        assert_mixed_bits(got, want, what + ": forward")
        assert x.nonzero_density() == mr.density(want), what
        back = take(x.to_csr(tol, handle))
        assert_bits(back, mr.to_csr(want, tol), what + ": inverse")
        return got, back
    finally:
        x.dispose()


# ---- forward and inverse ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(MATRICES))
def test_both_directions_match_the_restatement(handle, name, dtype):
    M = typed(MATRICES[name], dtype)
    dM = M.toGpuCSR()
    try:
        for r, c in TILES:
            for brows, bcols in corners(M.rows, M.cols, r, c):
                check_both_directions(handle, M, dM, r, c, brows, bcols, f"{name} r={r} c={c} corner {brows}x{bcols}")
    finally:
        dM.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_top", [t + d for t in (CP_TILE, RS_TILE, SCAN_TILE) for d in (-1, 0, 1)])
def test_tile_edges_of_the_entry_dealt_kernels_and_of_the_scan(handle, n_top, dtype):
    """61 x 97 with exactly n_top entries in its top 30 rows: the last block of k_flags / k_scatter and the last tile of
    the scan are full, one short, or hold a single entry"""
    M0 = top_heavy(61, 97, 30, n_top, 777, n_top)
    assert M0.rowPtr[30] == n_top and M0.nnz == n_top + 777
    M = typed(M0, dtype)
    dM = M.toGpuCSR()
    try:
        for r, c in ((1, 1), (2, 2), (3, 5)):
            check_both_directions(handle, M, dM, r, c, 30, 50, f"n_top={n_top} r={r} c={c}")
        check_both_directions(handle, M, dM, 2, 2, 30, 97, f"n_top={n_top}: all of the top rows in the corner")
    finally:
        dM.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_corner_boundary(handle, dtype):
    """columns blockCols - 1 and blockCols in every row, in descending order; rows blockRows - 1 and blockRows populated"""
    for (r, c), brows, bcols in (((2, 2), 24, 77), ((3, 5), 24, 75), ((3, 5), 24, 77), ((1, 64), 25, 64), ((1, 64), 25, 65)):
        M0 = boundary_columns(50, 200, bcols)
        M = typed(M0, dtype)
        dM = M.toGpuCSR()
        try:
            got, _ = check_both_directions(handle, M, dM, r, c, brows, bcols, f"boundary r={r} c={c} corner {brows}x{bcols}")
            # from the definition alone: above blockRows a row keeps {n - 1, blockCols}, below it all four
            assert np.diff(got.rest.rowPtr).tolist() == [2] * brows + [4] * (50 - brows)
            assert got.rest.colInd[:2 * brows].tolist() == [199, bcols] * brows and got.corner.nnz == 2 * brows
        finally:
            dM.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["inside the corner's rows", "the first row below the corner"])
def test_one_long_row_gives_the_same_bytes_twice(handle, where, dtype):
    brows = 384 if where.startswith("inside") else 192          # the long row is row 192
    M = typed(LONG, dtype)
    dM = M.toGpuCSR()
    try:
        for r, c in TILES:
            runs = [all_bytes(*check_both_directions(handle, M, dM, r, c, brows, 150, f"long row, {where}, r={r} c={c}", 0.0))
                    for _ in range(2)]
            assert runs[0] == runs[1], f"{where} r={r} c={c}"
    finally:
        dM.deviceDispose()


# ---- bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_values_keep_their_bits_and_only_the_corner_drops_them(handle, dtype):
    sp = _special(dtype)
    assert np.isnan(sp["nan"]) and float(sp["denormal"]) > 0.0 and float(sp["1e-9"]) <= 1e-9 < float(sp["above"])
    names = list(sp)
    rows, cols, brows, bcols = 9, 11, 6, 6
    rng = np.random.default_rng(6)          # a layout that puts every kind of value into both parts (asserted below)
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
    row_of = np.repeat(np.arange(rows), np.diff(M.rowPtr))
    inside = (row_of < brows) & (np.asarray(M.colInd) < bcols)
    bits = np.uint32 if np.dtype(dtype) == np.float32 else np.uint64
    # every kind of value lands in both parts
    assert all((kind[inside] == k).any() and (kind[~inside] == k).any() for k in names)
    dM = M.toGpuCSR()
    try:
        for r, c in ((1, 1), (2, 2), (3, 5)):
            for tol, dropped in ((1e-9, {"nan", "-0", "denormal", "1e-9"}), (0.0, {"nan", "-0"})):
                what = f"special r={r} c={c} tol={tol}"
                got, back = check_both_directions(handle, M, dM, r, c, brows, bcols, what, tol)
                # forward keeps all of them: every source value's bits are in the tiles or in the remainder
                have = set(got.corner.values.view(bits).tolist()) | set(np.asarray(got.rest.values).view(bits).tolist())
                assert set(M.values.view(bits).tolist()) <= have, what
                # back: the corner drops as hip_bcsr_to_csr does, the remainder drops nothing
                keep = ~inside | ~np.isin(kind, list(dropped))
                survivors = rr.sort_rows(rr.Host(np.concatenate([[0], np.cumsum(np.bincount(row_of[keep], minlength=rows))]),
                                                 M.colInd[keep], M.values[keep], rows, cols))
                assert_bits(rr.sort_rows(back), survivors, what + ": exactly those are dropped")
    finally:
        dM.deviceDispose()


# ---- round trip ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["1000x257", "257x1000"])
def test_round_trip_of_a_sorted_matrix_is_the_matrix(handle, name, dtype):
    S = typed(rr.sort_rows(MATRICES[name]), dtype)
    dS = S.toGpuCSR()
    raw = hs.csr_diff_raw_f64 if np.dtype(dtype) == np.float64 else hs.csr_diff_raw
    try:
        for r, c in [(1, 5)] + TILES:
            for brows, bcols in ((S.rows // 2 // r * r, S.cols // 2), (S.rows // r * r, S.cols)):
                what = f"{name} r={r} c={c} corner {brows}x{bcols}"
                x = hs.MCSR.from_csr(dS, r, c, brows, bcols, handle)
                back = x.to_csr(1e-9, handle)
                try:
                    if r > 1:
                        hs.sort_rows_device(back, handle)
                    d = raw(handle, S.rows, S.cols, back.rowPtr, back.colInd, back.values, back.nnz, dS.rowPtr, dS.colInd,
                            dS.values, dS.nnz, 0.0, 0.0)
                    assert (d.rows_len_differ, d.only_a, d.only_b, d.beyond) == (0, 0, 0, 0), (what, d.as_dict())
                    assert_bits(back.toCpuCSR(), S, what)
                finally:
                    back.deviceDispose()
                    x.dispose()
    finally:
        dS.deviceDispose()


# ---- bad input -------------------------------------------------------------------------------------------------------
def test_bad_input_is_an_error_not_a_fault(handle):
    L = hs.lib()
    M = typed(TALL, np.float32)
    dM = M.toGpuCSR()
    m, n, r, c, brows, bcols = M.rows, M.cols, 3, 5, 501, 128
    good = mr.to_mcsr(M, r, c, brows, bcols)
    good_back = mr.to_csr(good, 1e-9)
    dev = hs.MCSR(dM, r, c, brows, bcols, handle)
    ups = []

    def forward_rc(IA, JA, VA, rows, cols, nnz, tr=r, tc=c, trows=brows, tcols=bcols):
        o = [C.c_void_p(1) for _ in range(6)]
        cnt = [C.c_int(9), C.c_int(9)]
        rc = L.hip_csr_to_mcsr(handle.ptr, rows, cols, nnz, C.c_void_p(IA), C.c_void_p(JA), C.c_void_p(VA), tr, tc, trows, tcols,
                               C.byref(o[0]), C.byref(o[1]), C.byref(o[2]), C.byref(cnt[0]),
                               C.byref(o[3]), C.byref(o[4]), C.byref(o[5]), C.byref(cnt[1]))
        return rc, [x.value for x in o] + [x.value for x in cnt], L.spgemm_hip_last_error()

    def inverse_rc(IB, JB, nnzb, IR, nnzR):
        o = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        cnt = C.c_int(9)
        rest = dev.remainder
        rc = L.hip_mcsr_to_csr(handle.ptr, m, n, r, c, brows, bcols, nnzb, C.c_void_p(IB), C.c_void_p(JB), C.c_void_p(dev.values),
                               nnzR, C.c_void_p(IR), C.c_void_p(rest.colInd), C.c_void_p(rest.values), 1e-9,
                               *[C.byref(x) for x in o], C.byref(cnt))
        return rc, [x.value for x in o] + [cnt.value], L.spgemm_hip_last_error()

    def valid_call(what):
        x = hs.MCSR(dM, r, c, brows, bcols, handle)
        try:
            assert_mixed_bits(downloaded(x), good, what)
            assert_bits(take(x.to_csr(1e-9, handle)), good_back, what)
        finally:
            x.dispose()

    def refused(call, status, word, what):
        """the error twice from an empty cache: the second call must give back exactly what it took; then a valid call
        on the same handle, and after a trim nothing is left"""
        hs.pool_trim(handle.device)
        nothing = [None] * 6 + [0, 0] if call.__name__ == "forward" else [None] * 3 + [0]
        rc, outs, msg = call()
        assert rc == status and outs == nothing and word in msg, (what, rc, outs, msg)
        balance = hs.pool_cached_bytes(handle.device)
        rc, outs, msg = call()
        assert rc == status and outs == nothing, (what, rc, outs, msg)
        assert hs.pool_cached_bytes(handle.device) == balance, what
        valid_call("valid call after " + what)
        hs.pool_trim(handle.device)
        assert hs.pool_cached_bytes(handle.device) == 0, what

    def forward(*a):
        def forward():
            return forward_rc(*a)
        return forward

    def inverse(*a):
        def inverse():
            return inverse_rc(*a)
        return inverse

    try:
        rest = dev.remainder
        falling = M.rowPtr.copy()
        falling[500] = falling[499] - 1 if falling[499] > 0 else falling[501] + 1
        ups.append(hs.h2d(falling))
        refused(forward(ups[0], dM.colInd, dM.values, m, n, M.nnz), ERR_INPUT, b"rowPtr", "a decreasing rowPtr")
        bad_cols = M.colInd.copy()
        bad_cols[7] = n
        ups.append(hs.h2d(bad_cols))
        refused(forward(dM.rowPtr, ups[1], dM.values, m, n, M.nnz), ERR_INPUT, b"column", "a column equal to n")
        assert good.corner.nnzb > 11
        bad_bcols = good.corner.colInd.copy()
        bad_bcols[11] = good.corner.bn
        ups.append(hs.h2d(bad_bcols))
        refused(inverse(dev.rowPtr, ups[2], dev.nnzb, rest.rowPtr, rest.nnz), ERR_INPUT, b"block column",
                "a block column equal to bn")
        refused(inverse(dev.rowPtr, dev.colInd, dev.nnzb - 1, rest.rowPtr, rest.nnz), ERR_INPUT, b"rowPtr",
                "a block rowPtr not ending at nnzb")
        refused(inverse(dev.rowPtr, dev.colInd, dev.nnzb, rest.rowPtr, rest.nnz - 1), ERR_INPUT, b"remainder",
                "a remainder rowPtr not ending at nnzR")
        # 524 289 tiles of 64 x 64 = 2^31 + 4096 values with the corner covering the whole matrix: known only after the
        # corner's count pass
        side, ntiles = 46400, 524289
        assert ntiles * 4096 > 2 ** 31 - 1 >= (ntiles - 2) * 4096 and ntiles <= ((side + 63) // 64) ** 2 and side % 64 == 0
        big = _strided_tiles(ntiles, side, 64)
        ups.extend([hs.h2d(big.rowPtr), hs.h2d(big.colInd), hs.h2d(big.values)])
        refused(forward(ups[3], ups[4], ups[5], side, side, ntiles, 64, 64, side, side), ERR_OVERFLOW, b"int32",
                "more than INT32_MAX tile values")
    finally:
        for ptr in ups:
            hs.dev_free(ptr)
        dev.dispose()
        dM.deviceDispose()


def test_pool_does_not_grow(handle):
    M = typed(TALL, np.float64)
    dM = M.toGpuCSR()

    def rounds(k):
        for _ in range(k):
            x = hs.MCSR(dM, 3, 5, 501, 128, handle)
            x.to_csr(1e-9, handle).deviceDispose()
            x.dispose()
    try:
        rounds(20)
        before = hs.pool_cached_bytes(handle.device)
        rounds(5)
        assert hs.pool_cached_bytes(handle.device) == before
    finally:
        dM.deviceDispose()


# ---- the mirrors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_python_mcsr_on_the_reference_vectors(handle, dtype):
    """tests/golden/mcsr_kat.json (the reference's tests/MCSR_test.cc:9-33) through the Python class"""
    with open(os.path.join(ROOT, "tests", "golden", "mcsr_kat.json")) as f:
        k = json.load(f)
    e = k["expected"]
    A = hs.CSR.from_arrays(k["rowPtr"], k["colInd"], k["values"], k["rows"], k["cols"], dtype=dtype)
    dA = A.toGpuCSR()
    x = hs.MCSR.from_csr(dA, k["r"], k["c"], k["blockRows"], k["blockCols"], handle)
    try:
        assert (x.m, x.n, x.r, x.c, x.blockRows, x.blockCols, x.bm, x.bn, x.nnzb, x.nnz) == (7, 7, 1, 2, 4, 4, 4, 2, 4, 6)
        assert (x.remainder.rows, x.remainder.cols, x.remainder.nnz) == (7, 7, 11) and x.nonzero_density() == 75.0
        got = downloaded(x)
        assert got.rest.rowPtr.tolist() == e["remainder_rowPtr"] and got.rest.colInd.tolist() == e["remainder_colInd"]
        assert got.rest.values.tolist() == e["remainder_values"] and got.rest.values.dtype == np.dtype(dtype)
        assert got.corner.rowPtr.tolist() == e["block_rowPtr"] and got.corner.colInd.tolist() == e["block_colInd"]
        assert got.corner.values.tolist() == e["tiles"] and got.corner.values.dtype == np.dtype(dtype)
        assert_bits(take(x.to_csr(handle=handle)), A, "7x7: r == 1 and sorted rows come back as they were")
    finally:
        x.dispose()
        dA.deviceDispose()
    assert x.remainder is None and x.rowPtr is None


def test_cpp_mirror_runs_the_reference_scenario():
    """tests/cpp/mcsr_check.cc: the scenario of the reference's tests/MCSR_test.cc on the C++ mirror"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-B", "-C", cpp, "mcsr_check.x"])
    out = subprocess.run([os.path.join(cpp, "mcsr_check.x")], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    for check in ("shape", "remainder rowPtr", "remainder colInd", "remainder values", "block rowPtr", "block colInd", "tiles",
                  "density", "round trip shape", "round trip rowPtr", "round trip colInd", "round trip values"):
        assert f"7x7 {check}: ok" in lines, check
    assert "Pass" in lines and "FAILED" not in out.stdout
