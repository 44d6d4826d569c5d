"""GPU (-m gpu): double-valued edge-list text parsed on the device -- hip_parse_edge_text_f64 / hip_parse_edge_lines_f64 /
hip_read_edge_file_f64.  Every comparison is on bits (indices, the 64 bits of each double, rowPtr).  The texts are at most
four tiles of the count / starts kernels (EDGE_TILE bytes): what can go wrong is where a line lies relative to a tile, to a
block of the parse kernel (256 lines), to the LDS stage and to the end of the text, and whether a value takes the device
conversion or the host's strtod.  Expected triplets come from the generator that wrote the text, value bits from Python's
float(token), which is correctly rounded like strtod; the files' from tests/edges_f64_ref.py."""
import os

import numpy as np
import pytest

import edges_f64_ref as er
import f64ref
from devcsr import built_gpu, handle  # noqa: F401
from helpers import DATA
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu
EDGE_TILE, BLOCK_LINES, EDGE_STAGE = 4096, 256, 8192      # edges_device.hpp; tests/test_gpu_edges_parse.py checks them
T = EDGE_TILE
F64 = np.float64
FILES = ["test.mtx", "test2.mtx", "t2.snap", "tdata.snap", "own_graph.snap", "own_dups.mtx"]
SLOW = ["inf", "1e300", "1e-300", "12345678901234567890"]   # by text, by exponent (twice), by 20 digits


def parse(handle, text, declared, **kw):
    t = hs.parse_edge_text(bytes(text), declared, handle=handle, dtype=F64, **kw)
    try:
        assert t.dtype == F64
        r, c, v = t.download()
    finally:
        t.dispose()
    assert v.dtype == F64
    return r, c, v.view(np.uint64), t.entries, t.stats


def parse_on_device(handle, text, declared, flags=0):
    d = hs.h2d(np.frombuffer(bytes(text), np.uint8))             # a pool block: aligned far beyond 16 bytes
    try:
        r, c, v, n, st = hs.parse_edge_lines_raw_f64(handle, d, len(text), declared, flags)
    finally:
        hs.dev_free(d)
    try:
        return hs.d2h(r, n, np.int32), hs.d2h(c, n, np.int32), hs.d2h(v, n, np.uint64), n, st
    finally:
        for p in (r, c, v):
            hs.dev_free(p)


def assert_triplets(got, want, what):
    assert len(got[0]) == len(want[0]), f"{what}: {len(got[0])} entries, expected {len(want[0])}"
    for g, w, name in zip(got[:3], want, ("row", "col", "value bits")):
        assert np.array_equal(g, w), f"{what}: {name} differ first at {int(np.nonzero(g != w)[0][0])}"


def check_gen(handle, g, what, declared=None, slow=0, **kw):
    n = len(g.rows)
    got = parse(handle, g.text, n if declared is None else declared, **kw)
    assert_triplets(got, g.expected(), what)
    assert got[3] == n and got[4]["lines"] == n and got[4]["first_bad_line"] == -1 and got[4]["slow_lines"] == slow, (what, got[4])


# ---- values ------------------------------------------------------------------------------------------------------------
def test_mixed_values_every_line_fast(handle):
    g = er.Gen64(1)
    for tok in ("0.30000000000000004", "3.141592653589793", "9007199254740993", "4503599627370496.5", "1e27", "1e-27",
                "9999999999999999999e27", "-0.0", "0e999", "5.", ".5"):
        g.line(tok)
    g.fill_to(3 * T + 517)
    assert 3 * T <= len(g.text) <= 4 * T and len(g.rows) > BLOCK_LINES
    vals = np.array(g.vals)
    with np.errstate(over="ignore"):                            # 9999999999999999999e27 is beyond the float range
        assert np.any(vals != vals.astype(np.float32)), "the text holds values no float holds"
    check_gen(handle, g, "mixed values")                        # slow_lines == 0: nothing went to the host


def slow_text(seed=8, n=600):
    g = er.Gen64(seed)
    for k in range(n):
        g.line(SLOW[(k // 4) % 4]) if k % 4 == 1 else g.mixed()
    return g


def test_slow_lines_are_merged_in_place(handle):
    g = slow_text()
    assert len(g.text) <= 4 * T
    check_gen(handle, g, "every fourth line slow", slow=150)
    v = g.expected()[2]
    assert np.count_nonzero(v == er.bits64([np.inf])[0]) == 38 and np.count_nonzero(v == er.bits64([1e-300])[0]) == 37


def test_a_bad_line_in_the_middle(handle):
    g = er.Gen64(6)
    for _ in range(300):
        g.mixed()
    lines = bytes(g.text).split(b"\n")[:-1]
    lines[170] = b"this is not an edge"
    got = parse(handle, b"\n".join(lines) + b"\n", 300)
    assert got[3] == 170 and got[4]["first_bad_line"] == 170 and got[4]["lines"] == 300
    assert_triplets(got, g.expected(170), "bad line at 170")
    lines[40] = b"99999999999999999999"                          # a slow line that turns out bad joins the minimum
    got = parse(handle, b"\n".join(lines) + b"\n", 300)
    assert got[3] == 40 and got[4]["first_bad_line"] == 40 and got[4]["slow_lines"] == 1
    assert_triplets(got, g.expected(40), "slow bad line at 40")


# ---- where a line lies -------------------------------------------------------------------------------------------------
def test_newline_is_the_last_byte_of_tile_0(handle):
    g = er.Gen64(2).fill_to(T).fill_to(3 * T + 700)
    assert g.text[T - 1] == 10 and 3 * T <= len(g.text) <= 4 * T
    check_gen(handle, g, "newline at T - 1")


def test_a_line_longer_than_the_stage(handle):
    g = er.Gen64(3).fill_to(300)
    g.line("0.10000000000000001", lead=EDGE_STAGE + 100, a=7, b=8)     # its block's span does not fit the LDS stage
    g.fill_to(3 * T + 900)
    assert bytes(g.text).find(b"7 8 0.10000000000000001\n") > EDGE_STAGE and len(g.text) <= 4 * T
    check_gen(handle, g, "a line of EDGE_STAGE + 100 bytes")


def test_no_final_newline_and_declared_below_the_lines(handle):
    g = er.Gen64(5).fill_to(2 * T + 50)
    g.line("0.30000000000000004", a=41, b=42, eol=b"")
    assert g.text[-1] != 10
    check_gen(handle, g, "no final newline")
    check_gen(handle, g, "no final newline, declared beyond the lines", declared=len(g.rows) + 5)
    n = len(g.rows)
    got = parse(handle, g.text, n - 7)
    assert got[3] == n - 7 and got[4]["lines"] == n and got[4]["first_bad_line"] == -1
    assert_triplets(got, g.expected(n - 7), "declared below the line count")


def test_crlf_and_one_based_transposed(handle):
    g = er.Gen64(7)
    for k in range(2 * BLOCK_LINES + 1):
        g.line(SLOW[k % 4], eol=b"\r\n") if k % 50 == 9 else g.mixed(eol=b"\r\n")
    assert len(g.text) <= 4 * T
    nslow = len(range(9, 2 * BLOCK_LINES + 1, 50))
    check_gen(handle, g, "CRLF", slow=nslow)
    r, c, v = g.expected()
    got = parse(handle, g.text, len(r), one_based=True, transpose=True)
    assert_triplets(got, (c - 1, r - 1, v), "ONE_BASED | TRANSPOSE")
    assert got[4]["slow_lines"] == nslow                         # the host's lines take the same flags


def test_device_text_entry_equals_the_host_text_entry(handle):
    g = er.Gen64(9).fill_to(3 * T + 333)
    a, b = parse(handle, g.text, len(g.rows)), parse_on_device(handle, g.text, len(g.rows))
    assert_triplets(b, g.expected(), "device text")
    assert [x.tobytes() for x in a[:3]] == [x.tobytes() for x in b[:3]] and a[3] == b[3]
    s = slow_text(seed=10)
    b = parse_on_device(handle, s.text, 600, hs.EDGES_TRANSPOSE)
    want = s.expected()
    assert b[4]["slow_lines"] == 150 and b[3] == 600             # only those lines were copied back
    assert_triplets(b, (want[1], want[0], want[2]), "slow lines, device text")


# ---- files -------------------------------------------------------------------------------------------------------------
def write_g17(path, n=20000, rows=2000, seed=11):
    """n lines "from to %.17g" of doubles in (0, 1), some pairs repeated, behind comments and a "rows declared" line"""
    rng = np.random.default_rng(seed)
    fr, to = rng.integers(0, rows, n), rng.integers(0, rows, n)
    fr[n // 2:n // 2 + 500], to[n // 2:n // 2 + 500] = fr[:500], to[:500]
    val = rng.random(n)
    with open(path, "w") as f:
        f.write(f"# generated\n# {n} lines\n{rows} {n}\n")
        f.write("".join(f"{a} {b} {x:.17g}\n" for a, b, x in zip(fr.tolist(), to.tolist(), val.tolist())))


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    p = tmp_path_factory.mktemp("edge_lists_f64") / "g17.snap"
    write_g17(p)
    return str(p)


def file_path(name, generated):
    return generated if name == "g17.snap" else os.path.join(DATA, name)


@pytest.mark.parametrize("isTrans", [False, True])
@pytest.mark.parametrize("name", FILES + ["g17.snap"])
def test_files_against_the_python_reference(handle, generated, name, isTrans):
    path = file_path(name, generated)
    for flags in (hs.COO_DEDUPE, hs.COO_SELF_LOOPS | hs.COO_ROW_NORMALISE):
        want, entries = er.load(path, isTrans, flags)
        d = hs.read_edge_file(path, isTrans, flags, handle, dtype=F64)
        try:
            assert d.dtype == F64 and d.edge_stats["entries"] == entries
            if name == "g17.snap":
                assert d.edge_stats["slow_lines"] == 0           # 17 digits, |e10| far below 27: the device converts them all
            er.assert_bits64(d.toCpuCSR(), want, f"{name} isTrans={isTrans} flags={flags}")
        finally:
            d.deviceDispose()


def test_loaded_csr_through_the_double_product(handle, generated):
    """the file's CSR is a double device CSR the _f64 calls accept: A * A against the float64 reference, every value
    within the bound of tests/f64ref.py (two summation orders of the same N terms)"""
    want, _ = er.load(generated, True, hs.COO_DEDUPE)
    d = hs.read_edge_file(generated, True, hs.COO_DEDUPE, handle, dtype=F64)
    try:
        ic, jc, cv, nnz = hs.gpu_spmm_raw_f64(handle, d.rowPtr, d.colInd, d.values, d.nnz, d.rowPtr, d.colInd, d.values, d.nnz,
                                              d.rows, d.cols, d.cols)
        try:
            rp, ci, v = hs.d2h(ic, d.rows + 1, np.int32), hs.d2h(jc, nnz, np.int32), hs.d2h(cv, nnz, F64)
        finally:
            for p in (ic, jc, cv):
                hs.dev_free(p)
        dC = hs.gpuSpMMWrapper(d, d, handle)                     # and through the wrapper, which reads the CSR's dtype
        assert dC.dtype == F64 and dC.nnz == nnz
        dC.deviceDispose()
    finally:
        d.deviceDispose()
    ref = f64ref.spgemm_f64(want, want)
    assert want.rows == 2000 and nnz == ref.nnz and np.array_equal(rp, ref.rowPtr)
    cols, vals = f64ref.sorted_rows(rp, ci, v)
    assert np.array_equal(cols, ref.colInd)
    assert len(f64ref.bound_violations(vals, ref)) == 0


def test_failure_then_success_and_the_float_loader_is_unmoved(handle, generated, tmp_path):
    def floats():
        d = hs.read_edge_file(generated, True, hs.COO_DEDUPE, handle)
        try:
            assert d.dtype == np.float32
            m = d.toCpuCSR()
            return m.rowPtr.tobytes(), m.colInd.tobytes(), m.values.tobytes()
        finally:
            d.deviceDispose()

    before = floats()
    bad = tmp_path / "outside.snap"
    bad.write_bytes(b"3 2\n0 1 0.5\n2 7 0.25\n")                # the second entry lies outside the 3 x 3 matrix
    with pytest.raises(hs.SpgemmError, match="outside"):
        hs.read_edge_file(str(bad), False, hs.COO_DEDUPE, handle, dtype=F64)
    want, _ = er.load(generated, False, hs.COO_DEDUPE)
    d = hs.read_edge_file(generated, False, hs.COO_DEDUPE, handle, dtype=F64)
    try:
        er.assert_bits64(d.toCpuCSR(), want, "after a failed call")
    finally:
        d.deviceDispose()
    assert floats() == before
