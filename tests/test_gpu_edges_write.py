"""GPU: a device CSR written as edge-list text on the device (hip_format_csr_edges / hip_csr_to_edge_text /
hip_write_edge_file, float and double).  Expected bytes come from tests/edges_write_ref.py (Python's %-formatting of the
host arrays, the C library's snprintf for nan and inf); every comparison is on bytes.  The shapes are the smallest at
which placement can go wrong: a write-pass block is EPB entries, a slab of the file entry SLAB // LINE_MAX entries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edges_write_ref as ref
from devcsr import built_gpu, handle  # noqa: F401
from devcsr import assert_bits, take
from helpers import DATA, ROOT, po, random_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu

EPB = 256                      # entries per block of the length and write passes
LINE_MAX = 49
CPP = os.path.join(ROOT, "tests", "cpp")
DTYPES = [np.float32, np.float64]
FMTS = [ref.FIXED6, ref.ROUNDTRIP]


def test_the_block_and_line_sizes_are_the_ones_in_the_code():
    csrc = os.path.join(ROOT, "sparse_matrix_with_flops_amd", "csrc")
    with open(os.path.join(csrc, "edges_write_device.hpp")) as f:
        assert int(re.search(r"constexpr int EW_THREADS = (\d+)", f.read()).group(1)) == EPB
    with open(os.path.join(csrc, "edge_print.hpp")) as f:
        src = f.read()
    assert 2 * int(re.search(r"INDEX_MAX = (\d+);", src).group(1)) + int(re.search(r"VALUE_MAX = (\d+);", src).group(1)) + 3 == LINE_MAX


# ---- inputs (made once, never modified) ------------------------------------------------------------------------------
class Host:
    def __init__(self, rowPtr, colInd, values, rows, cols):
        self.rowPtr = np.ascontiguousarray(rowPtr, np.int32)
        self.colInd = np.ascontiguousarray(colInd, np.int32)
        self.values = np.ascontiguousarray(values)
        self.rows, self.cols, self.nnz = int(rows), int(cols), len(self.colInd)

    def device(self):
        return hs.CSR.from_arrays(self.rowPtr, self.colInd, self.values, self.rows, self.cols, dtype=self.values.dtype).toGpuCSR()


def fast_values(n, seed, dtype):
    """both signs, magnitudes 1e-6 .. 1e6: inside the class of both formats, line lengths mixed"""
    rng = np.random.default_rng(seed)
    v = 10.0 ** rng.uniform(-6, 6, n) * rng.choice([-1.0, 1.0], n)
    v[rng.random(n) < 0.1] = 0.0
    whole = rng.random(n) < 0.1
    v[whole] = np.round(v[whole])                          # a few integers, -0 among them
    return v.astype(dtype)


def by_lengths(lengths, cols, seed, dtype):
    lengths = np.asarray(lengths, np.int64)
    rp = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=rp[1:])
    rng = np.random.default_rng(seed)
    ci = np.concatenate([np.sort(rng.integers(0, cols, n)) for n in lengths]) if len(lengths) else np.zeros(0, np.int64)
    return Host(rp, ci, fast_values(int(rp[-1]), seed + 1, dtype), len(lengths), cols)


def structure_inputs(dtype):
    out = {
        # empty rows first, in the middle and last; one row longer than two write-pass blocks
        "empty rows, a long row": by_lengths([0, 0, 5, 0, 0, 2 * EPB + 88, 3, 1, 0, 0], 100000, 1, dtype),
        "one row": by_lengths([7], 50, 2, dtype),
        "no entries": by_lengths([0, 0, 0], 9, 3, dtype),
        "no rows": by_lengths([], 9, 4, dtype),
    }
    for k in (1, 2):
        for d in (-1, 0, 1):
            nnz = k * EPB + d
            lens = np.bincount(np.random.default_rng(10 * k + d).integers(0, 37, nnz), minlength=37)
            out[f"nnz = {k} blocks {d:+d}"] = by_lengths(lens, 1000, 20 + 3 * k + d, dtype)
    return out


@pytest.fixture(scope="module")
def structures():
    return {np.dtype(dt): structure_inputs(dt) for dt in DTYPES}


def text_of(handle, d, **kw):
    data, st = hs.csr_to_edge_text(d, handle=handle, **kw)
    return data, st


def device_text_of(handle, d, **kw):
    """hip_format_csr_edges: the text stays on the device; brought down with a plain copy"""
    p, n, st = hs.format_csr_edges(d, handle=handle, **kw)
    try:
        return hs.d2h(p, n, np.uint8).tobytes(), st
    finally:
        hs.dev_free(p)


def assert_text(got, want, what):
    if got == want:
        return
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    lo = max(0, at - 40)
    raise AssertionError(f"{what}: {len(got)} bytes, want {len(want)}; first difference at byte {at}: "
                         f"{got[lo:at + 40]!r} vs {want[lo:at + 40]!r}")


# ---- structure -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, ref.ONE_BASED, ref.TRANSPOSE, ref.ONE_BASED | ref.TRANSPOSE])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_structure(handle, structures, dtype, fmt, flags):
    for name, M in structures[np.dtype(dtype)].items():
        want = ref.Text(M, fmt, flags).data
        d = M.device()
        try:
            got, st = text_of(handle, d, fmt=fmt, flags=flags)
            assert_text(got, want, f"{name}: host text")
            assert (st["entries"], st["bytes"], st["slow_entries"], st["slabs"]) == (M.nnz, len(want), 0, 1), name   # all fast
            got, st = device_text_of(handle, d, fmt=fmt, flags=flags)
            assert_text(got, want, f"{name}: device text")
            assert st["slow_entries"] == 0, name
        finally:
            d.deviceDispose()


# ---- line lengths ----------------------------------------------------------------------------------------------------
def wide_columns(dtype):
    """n = 2147483647; columns of every width from 1 to 10 digits, 9 / 10 / 99999 / 2147483646 among them; 64 blocks (the
    seed is one at which the blocks' spans start at all 16 alignments in every format: asserted below)"""
    rng = np.random.default_rng(8)
    pool = np.array([0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000,
                     99999999, 100000000, 999999999, 1000000000, 2147483646], np.int64)
    lens = np.bincount(rng.integers(0, 50, 64 * EPB), minlength=50)
    rp = np.zeros(51, np.int64)
    np.cumsum(lens, out=rp[1:])
    ci = np.concatenate([np.sort(rng.choice(pool, n)) for n in lens])
    return Host(rp, ci, fast_values(64 * EPB, 9, dtype), 50, 2147483647)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_index_widths_and_every_span_alignment(handle, dtype, fmt):
    M = wide_columns(dtype)
    for flags in (0, ref.ONE_BASED):                       # ONE_BASED prints 2147483647
        t = ref.Text(M, fmt, flags)
        widths = {len(b"%d" % c) for c in (M.colInd.astype(np.int64) + (1 if flags else 0)).tolist()}
        assert widths == set(range(1, 11))
        starts = t.offsets[np.arange(0, M.nnz, EPB)]
        assert set((starts % 16).tolist()) == set(range(16)), "the fixture must start a block's span at every alignment"
        d = M.device()
        try:
            got, st = device_text_of(handle, d, fmt=fmt, flags=flags)
        finally:
            d.deviceDispose()
        assert_text(got, t.data, f"wide columns flags={flags}")
        assert st["slow_entries"] == 0


# ---- slow entries ----------------------------------------------------------------------------------------------------
def slow_table(dtype, fmt):
    """values the device need not format (and some it must), for the first and last entry of blocks and in between"""
    if np.dtype(dtype) == np.float64:
        t = [np.inf, -np.inf, np.nan, -np.nan, 1e300, -1e300, 1e-300, 5e-324, 1e15, -1e17, 1e-16, 123.5, 1e14, 1e-15]
    else:
        t = [np.inf, -np.inf, np.nan, -np.nan, 3e38, -3e38, 1e-38, 1e-45, 1e15, -1e17, 1e-16, 123.5, 1e14, 2e-15]
    return np.array(t, dtype)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_slow_entries_between_fast_ones(handle, dtype, fmt):
    nnz = 3 * EPB + 5
    M = by_lengths(np.bincount(np.random.default_rng(8).integers(0, 20, nnz), minlength=20), 5000, 9, dtype)
    v = M.values.copy()
    table = slow_table(dtype, fmt)
    at = [0, EPB - 1, EPB, 2 * EPB - 1, 2 * EPB, 3 * EPB - 1, 3 * EPB, nnz - 1, 17, 300, 301, 302, 600, 700]
    v[at] = table
    M = Host(M.rowPtr, M.colInd, v, M.rows, M.cols)
    t = ref.Text(M, fmt)
    bound = ref.outside_class(v, fmt)
    assert 0 < bound <= len(table)
    d = M.device()
    try:
        got, st = text_of(handle, d, fmt=fmt)
        assert_text(got, t.data, "slow entries: host text")
        assert 0 < st["slow_entries"] <= bound and st["bytes"] == len(t.data)     # inf and nan are slow for certain
        got, st = device_text_of(handle, d, fmt=fmt, flags=ref.ONE_BASED | ref.TRANSPOSE)
        assert_text(got, ref.Text(M, fmt, ref.ONE_BASED | ref.TRANSPOSE).data, "slow entries: device text, both flags")
        assert st["slow_entries"] <= bound
    finally:
        d.deviceDispose()


def test_a_block_whose_slow_lines_outgrow_the_stage(handle):
    """40 values of 1e300 in FIXED6 are 40 lines of more than 300 bytes: the span of the second block no longer fits the
    LDS stage (EPB * LINE_MAX + 16 bytes) and is written by the other path; its neighbours are staged"""
    nnz = 3 * EPB
    M = by_lengths(np.bincount(np.random.default_rng(11).integers(0, 10, nnz), minlength=10), 5000, 12, np.float64)
    v = M.values.copy()
    v[EPB + 3:EPB + 3 + 40] = 1e300
    v[EPB] = -1e300
    v[2 * EPB - 1] = 1e299
    M = Host(M.rowPtr, M.colInd, v, M.rows, M.cols)
    t = ref.Text(M, ref.FIXED6)
    assert t.offsets[2 * EPB] - t.offsets[EPB] > EPB * LINE_MAX + 16 > t.offsets[EPB] - t.offsets[0]
    d = M.device()
    try:
        got, st = text_of(handle, d, fmt=ref.FIXED6)
    finally:
        d.deviceDispose()
    assert_text(got, t.data, "long slow lines")
    assert st["slow_entries"] == 42


# ---- row ranges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_ranges_are_slices_of_the_whole_text(handle, structures, dtype):
    M = structures[np.dtype(dtype)]["empty rows, a long row"]
    t = ref.Text(M, ref.ROUNDTRIP)
    d = M.device()
    try:
        whole, _ = text_of(handle, d, fmt=ref.ROUNDTRIP)
        assert_text(whole, t.data, "whole")
        for row0, row1 in [(0, 0), (4, 4), (M.rows, M.rows), (0, 2), (5, 6), (2, 3), (6, M.rows), (5, M.rows), (9, M.rows)]:
            got, st = text_of(handle, d, row0=row0, row1=row1, fmt=ref.ROUNDTRIP)
            lo, hi = t.offsets[t.rowPtr[row0]], t.offsets[t.rowPtr[row1]]
            assert_text(got, whole[lo:hi], f"rows [{row0}, {row1})")
            assert st["entries"] == t.rowPtr[row1] - t.rowPtr[row0]
            got, _ = device_text_of(handle, d, row0=row0, row1=row1, fmt=ref.ROUNDTRIP)
            assert_text(got, t.rows(row0, row1), f"device text of rows [{row0}, {row1})")
    finally:
        d.deviceDispose()


# ---- slabs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_many_slabs_write_the_file_of_one_slab(handle, dtype, tmp_path, monkeypatch):
    slab = 4096
    per = slab // LINE_MAX                                  # entries per slab
    # slab boundaries are the entries per, 2 per, ...: 3 per is made a row end, per and 2 per lie inside the long first row
    M = by_lengths([3 * per, 3, 0, 400, per - 3, 11, 700, 2, 250, 420], 100000, 13, dtype)
    assert M.rowPtr[1] == 3 * per
    t = ref.Text(M, ref.FIXED6)
    cuts = np.arange(per, M.nnz, per)
    on_row_end = np.isin(cuts, M.rowPtr)
    assert on_row_end.any() and (~on_row_end).any()
    assert 35000 < len(t.data) < 50000 and t.offsets[M.rowPtr[1]] > slab      # roughly 40 KB; one row's text exceeds a slab
    want = ref.header(1, M.rows, M.cols, M.nnz) + t.data
    d = M.device()
    try:
        one, many = tmp_path / "one.txt", tmp_path / "many.txt"
        monkeypatch.delenv("SPGEMM_EDGE_SLAB", raising=False)
        st1 = hs.write_edge_file(d, one, fmt=ref.FIXED6, header=1, handle=handle)
        monkeypatch.setenv("SPGEMM_EDGE_SLAB", str(slab))
        stn = hs.write_edge_file(d, many, fmt=ref.FIXED6, header=1, handle=handle)
    finally:
        d.deviceDispose()
    assert_text(one.read_bytes(), want, "one slab")
    assert_text(many.read_bytes(), want, "many slabs")
    assert st1["slabs"] == 1 and stn["slabs"] == len(cuts) + 1 > 8
    assert stn["entries"] == M.nnz and stn["bytes"] == len(want) == st1["bytes"]


# ---- round trip ------------------------------------------------------------------------------------------------------
def clustered_own_graph():
    """own_graph.snap after rmclInit and two R-MCL iterations on the device, rows column-sorted (a host CSR, float32)"""
    M0 = po.load(os.path.join(DATA, "own_graph.snap"), True, mode=1)
    d0 = hs.CSR.from_arrays(M0.rowPtr, M0.colInd, M0.values, M0.rows, M0.cols).toGpuCSR()
    try:
        Mt = take(hs.gpuRmclIter_device(2, d0, d0))
    finally:
        d0.deviceDispose()
    Mt.makeOrdered()
    return Mt


def wide_range_values(dtype):
    """a seeded synthetic matrix, rows column-sorted, values random floats of both signs in [1e-12, 1e12]"""
    M = random_csr(200, 300, 0.05, 21)
    rng = np.random.default_rng(22)
    v = 10.0 ** rng.uniform(-12, 12, len(M.colInd)) * rng.choice([-1.0, 1.0], len(M.colInd))
    return Host(M.rowPtr, M.colInd, v.astype(dtype), M.rows, M.cols)


@pytest.mark.parametrize("header", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["own_graph after two R-MCL iterations", "synthetic, 1e-12 .. 1e12"])
def test_round_trip_through_a_file_is_exact(handle, which, dtype, header, tmp_path):
    if which.startswith("own"):
        Mt = clustered_own_graph()
        M = Host(Mt.rowPtr, Mt.colInd, Mt.values.astype(dtype), Mt.rows, Mt.cols)
    else:
        M = wide_range_values(dtype)
    path = tmp_path / "m.txt"
    d = M.device()
    try:
        st = hs.write_edge_file(d, path, fmt=ref.ROUNDTRIP, header=header, handle=handle)
    finally:
        d.deviceDispose()
    flags = ref.ONE_BASED if header == 2 else 0
    assert_text(path.read_bytes(), ref.header(header, M.rows, M.cols, M.nnz) + ref.Text(M, ref.ROUNDTRIP, flags).data, which)
    assert st["slow_entries"] == 0
    want = hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols, dtype=dtype)
    back = take(hs.read_edge_file(str(path), False, hs.COO_DEDUPE, handle, dtype=dtype))
    assert_bits(back, want, f"{which}: the device parser reads back what the device writer wrote")
    if np.dtype(dtype) == np.float32:                      # the project's host loader holds float values
        assert_bits(po.load(str(path), False, mode=0), want, f"{which}: the host loader")


# ---- the C++ mirror --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("header", [1, 2])
def test_cpp_mirror_writes_what_the_host_loader_reads(header, tmp_path):
    subprocess.check_call(["make", "-s", "-f", "edges_write.mk", "-C", CPP, "edges_write_check.x"])
    out = tmp_path / "mt.txt"
    r = subprocess.run([os.path.join(CPP, "edges_write_check.x"), "check", os.path.join(DATA, "own_graph.snap"), str(out),
                        str(ref.ROUNDTRIP), str(header)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Same" in r.stdout, r.stdout + r.stderr
    head = hs.edge_text_header(out.read_bytes())
    assert head["one_based"] == (header == 2) and head["declared"] > 0


# ---- a text above INT32_MAX bytes ------------------------------------------------------------------------------------
def test_a_text_above_int32_max_bytes_is_refused_as_one_piece(handle):
    """one row of 58.1 M entries "0 2147483646 -1.2345678901234567e-05": 37 bytes each, 2^31 + 2.6 M bytes in all.  The
    offsets of one text are 32-bit: SPGEMM_ERR_OVERFLOW, from the 64-bit total of the scan, before a byte is written
    (hip_write_edge_file cuts such a matrix into slabs instead); one entry fewer than 2^31 / 37 fits and is sized."""
    line = len(b"0 2147483646 -1.2345678901234567e-05\n")
    assert line == 37
    nnz = 2 ** 31 // line + 70000
    d = hs.CSR.from_arrays(np.array([0, nnz], np.int32), np.full(nnz, 2147483646, np.int32),
                           np.full(nnz, -1.2345678901234567e-05, np.float64), 1, 2147483647, dtype=np.float64).toGpuCSR()
    try:
        with pytest.raises(hs.SpgemmError, match="status 3"):
            hs.format_csr_edges(d, fmt=ref.ROUNDTRIP, handle=handle)
        with pytest.raises(hs.SpgemmError, match="status 3"):
            hs.csr_to_edge_text(d, fmt=ref.ROUNDTRIP, handle=handle)
        fits = hs.CSR(d.values, d.colInd, hs.h2d(np.array([0, 2 ** 31 // line], np.int32)), 1, d.cols, 2 ** 31 // line, True,
                      dtype=np.float64)
        try:
            n, st = C.c_size_t(), hs.EdgeWriteStats()
            hs._call("hip_csr_to_edge_text", np.float64, None, 1, fits.cols, *hs._ptrs(fits.rowPtr, fits.colInd, fits.values),
                     0, 1, ref.ROUNDTRIP, 0, None, 0, C.byref(n), C.byref(st))
            assert n.value == st.bytes == (2 ** 31 // line) * line <= 2 ** 31 - 1 and st.slow_entries == 0
        finally:
            hs.dev_free(fits.rowPtr)
    finally:
        d.deviceDispose()


# ---- errors leave nothing behind -------------------------------------------------------------------------------------
def test_handle_is_usable_after_an_error_and_calls_repeat(handle, structures, tmp_path):
    M = structures[np.dtype(np.float32)]["nnz = 2 blocks +1"]
    want = ref.Text(M, ref.FIXED6).data
    d = M.device()
    try:
        with pytest.raises(hs.SpgemmError, match="cannot open"):
            hs.write_edge_file(d, tmp_path / "absent" / "x.txt", handle=handle)
        rp = np.array(M.rowPtr)
        rp[3], rp[4] = rp[4] + 1, rp[3]                     # not monotone
        drp = hs.h2d(rp)
        try:
            with pytest.raises(hs.SpgemmError, match="rowPtr"):
                hs.csr_to_edge_text(hs.CSR(d.values, d.colInd, drp, M.rows, M.cols, M.nnz, True, dtype=np.float32), handle=handle)
        finally:
            hs.dev_free(drp)
        for _ in range(3):
            got, _ = text_of(handle, d)
            assert_text(got, want, "after the errors")
    finally:
        d.deviceDispose()
