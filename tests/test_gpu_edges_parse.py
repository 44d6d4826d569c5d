"""GPU (-m gpu): edge-list text parsed on the device -- hip_parse_edge_text / hip_parse_edge_lines / hip_read_edge_file and
the C++ mirror's COO::readSNAPFileToGpuCSR.  Every comparison is on bits (indices, float bits, rowPtr).  The texts are a
few tiles each: what can go wrong is where a line lies relative to a tile of the count / starts kernels (EDGE_TILE
bytes), to a block of the parse kernel (256 lines) and to the end of the text, not how much text there is.
Expected triplets come from the generator that wrote the text; the crafted table's from what strtol / strtol / strtof
make of it on the host (tests/cpp/edge_scan_check.cc --table); the files' from the oracle's loader."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from devcsr import built_gpu, handle  # noqa: F401
from devcsr import assert_bits
from helpers import DATA, ROOT, po
from sparse_matrix_with_flops_amd import hipspgemm as hs
from test_loader import _edge_file

pytestmark = pytest.mark.gpu
EDGE_TILE = 4096           # bytes of text per block of k_edges_count / k_edges_starts (edges_device.hpp; checked below)
BLOCK_LINES = 256          # lines per block of k_edges_parse
EDGE_STAGE = 8192          # bytes of text a block of k_edges_parse stages in LDS; a longer span is read from global memory
T = EDGE_TILE
ERR_ARG, ERR_INPUT = 2, 5
CPP = os.path.join(ROOT, "tests", "cpp")
FILES = ["test.mtx", "test2.mtx", "t2.snap", "tdata.snap", "own_graph.snap", "own_dups.mtx"]


def test_the_tile_size_is_the_one_in_the_code():
    with open(os.path.join(ROOT, "sparse_matrix_with_flops_amd", "csrc", "edges_device.hpp")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int EDGE_TILE = (\d+)", src).group(1)) == EDGE_TILE
    assert int(re.search(r"constexpr int EDGE_THREADS = (\d+)", src).group(1)) == BLOCK_LINES
    assert int(re.search(r"constexpr int EDGE_STAGE = (\d+)", src).group(1)) == EDGE_STAGE


# ---- the generator: a line and the triplet it stands for ---------------------------------------------------------------
class Gen:
    """lines "from to [value]" with values k / 8 (exact in every format on the way), some without a value; builds the
    text and the triplets it must give"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.text = bytearray()
        self.rows, self.cols, self.bits = [], [], []

    def line(self, lead=0, width=0, a=None, b=None, v="rand", eol=b"\n"):
        """lead blanks in front; padded behind with blanks to at least `width` bytes (without the eol)"""
        a = int(self.rng.integers(0, 100000)) if a is None else a
        b = int(self.rng.integers(0, 100000)) if b is None else b
        if v == "rand":
            v = None if self.rng.integers(0, 3) else f"{int(self.rng.integers(0, 4000)) / 8:g}"
        body = b" " * lead + f"{a} {b}".encode() + (b" " + v.encode() if v is not None else b"")
        body += b" " * max(0, width - len(body))
        self.text += body + eol
        self.rows.append(a); self.cols.append(b)
        self.bits.append(np.float32(1.0 if v is None else float(v)).view(np.uint32))
        return self

    def fill_to(self, nbytes, width=0):
        """whole lines until the text is nbytes long: the last one is padded so that its '\n' is byte nbytes - 1"""
        while len(self.text) + 40 + width < nbytes:
            self.line(width=width)
        return self.line(width=nbytes - len(self.text) - 1)

    def expected(self, n=None):
        n = len(self.rows) if n is None else n
        return (np.array(self.rows[:n], np.int32), np.array(self.cols[:n], np.int32), np.array(self.bits[:n], np.uint32))


def parse(handle, text, declared, **kw):
    t = hs.parse_edge_text(bytes(text), declared, handle=handle, **kw)
    try:
        r, c, v = t.download()
    finally:
        t.dispose()
    return r, c, v.view(np.uint32), t.entries, t.stats


def assert_triplets(got, want, what):
    assert len(got[0]) == len(want[0]), f"{what}: {len(got[0])} entries, expected {len(want[0])}"
    for g, w, name in zip(got[:3], want, ("row", "col", "value bits")):
        assert np.array_equal(g, w), f"{what}: {name} differ first at {int(np.nonzero(g != w)[0][0])}"


def check_gen(handle, g, what, declared=None, text=None):
    text = g.text if text is None else text
    n = len(g.rows)
    got = parse(handle, text, n if declared is None else declared)
    assert_triplets(got, g.expected(), what)
    assert got[3] == n and got[4]["lines"] == n and got[4]["first_bad_line"] == -1 and got[4]["slow_lines"] == 0, (what, got[4])


# ---- tile boundaries ---------------------------------------------------------------------------------------------------
def test_newline_is_the_last_byte_of_tile_0(handle):
    g = Gen(1).fill_to(T).fill_to(3 * T + 700)
    assert g.text[T - 1] == 10 and 3 * T <= len(g.text) <= 4 * T
    check_gen(handle, g, "newline at T - 1")


def test_newline_is_the_first_byte_of_tile_1(handle):
    g = Gen(2).fill_to(T + 1).fill_to(3 * T + 1234)
    assert g.text[T] == 10 and g.text[T - 1] != 10 and 3 * T <= len(g.text) <= 4 * T
    check_gen(handle, g, "newline at T")


def test_a_line_longer_than_two_tiles(handle):
    g = Gen(3).fill_to(300)
    g.line(lead=2 * T + 100, a=7, b=8, v=".25")                # blank-padded in front, ends in "7 8 .25"
    g.fill_to(3 * T + 900)
    assert bytes(g.text).find(b"7 8 .25\n") > 2 * T and 3 * T <= len(g.text) <= 4 * T
    check_gen(handle, g, "a line of 2T + 100 bytes")            # its block's span does not fit the LDS stage
    k = [i for i, (a, b) in enumerate(zip(g.rows, g.cols)) if (a, b) == (7, 8)][0]
    assert g.bits[k] == np.float32(0.25).view(np.uint32)


@pytest.mark.parametrize("nbytes", [EDGE_STAGE, EDGE_STAGE + 1])
def test_one_block_at_the_limit_of_the_stage(handle, nbytes):
    """fewer than 256 lines and no final newline: the block's span is the whole text, EDGE_STAGE bytes (the last size
    that is staged) or one more (the first that is read from global memory)"""
    g = Gen(13).fill_to(nbytes - 10, width=60)
    g.line(a=1, b=2, v=None, width=10, eol=b"")
    assert len(g.text) == nbytes and len(g.rows) < BLOCK_LINES
    check_gen(handle, g, f"one block of {nbytes} bytes")


@pytest.mark.parametrize("nlines", [2 * BLOCK_LINES - 1, 2 * BLOCK_LINES, 2 * BLOCK_LINES + 1])
def test_line_count_around_a_multiple_of_the_block(handle, nlines):
    g = Gen(4)
    for _ in range(nlines):
        g.line(width=26)
    assert 3 * T <= len(g.text) <= 4 * T and len(g.rows) == nlines
    check_gen(handle, g, f"{nlines} lines")


def test_no_final_newline(handle):
    g = Gen(5).fill_to(3 * T + 50)
    g.line(a=41, b=42, v="3.5", eol=b"")
    assert g.text[-1] != 10
    check_gen(handle, g, "no final newline")
    check_gen(handle, g, "no final newline, declared beyond the lines", declared=len(g.rows) + 5)


@pytest.mark.parametrize("text, want", [
    (b"", []), (b"7", None), (b"\n", None),
    (b"1 2\n3 4\n5 6 .5\n", [(1, 2, 1.0), (3, 4, 1.0), (5, 6, .5)]),                     # 15 bytes
    (b"1 2\n3 4\n5 6 .25\n", [(1, 2, 1.0), (3, 4, 1.0), (5, 6, .25)]),                   # 16
    (b"1 2\n3 4\n5 6 .125\n", [(1, 2, 1.0), (3, 4, 1.0), (5, 6, .125)]),                 # 17
    (b"1 2\n3 4\n5 6 .125", [(1, 2, 1.0), (3, 4, 1.0), (5, 6, .125)]),                   # 16, the tail open
], ids=["0", "1", "1 newline", "15", "16", "17", "16 open"])
def test_texts_around_one_load(handle, text, want):
    r, c, v, n, st = parse(handle, text, 10)
    if want is None:                                             # one line, not an edge
        assert (n, st["lines"], st["first_bad_line"]) == (0, 1, 0)
        return
    assert st["lines"] == len(want) and st["first_bad_line"] == -1 and n == len(want)
    assert list(zip(r.tolist(), c.tolist(), v.view(np.float32).tolist())) == want


# ---- the counting rule -------------------------------------------------------------------------------------------------
def ten_lines(bad=(), slow_bad=()):
    g = Gen(6)
    lines = []
    for k in range(10):
        g.line()
        lines.append(bytes(g.text).split(b"\n")[k])
    for k in bad:
        lines[k] = b"this is not an edge"
    for k in slow_bad:
        lines[k] = b"99999999999999999999"                       # 20 digits: the host's strtol clamps, and a second field is missing
    return g, b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("declared", [0, 9, 10, 15, -3])
def test_declared_caps_the_entries(handle, declared):
    g, text = ten_lines()
    got = parse(handle, text, declared)
    n = min(max(declared, 0), 10)
    assert got[3] == n and got[4]["lines"] == 10 and got[4]["first_bad_line"] == -1
    assert_triplets(got, g.expected(n), f"declared={declared}")


def test_reading_stops_at_the_first_bad_line(handle):
    g, text = ten_lines(bad=(6,))
    got = parse(handle, text, 10)
    assert got[3] == 6 and got[4]["first_bad_line"] == 6
    assert_triplets(got, g.expected(6), "bad line at 6")
    g, text = ten_lines(bad=(6, 2))
    got = parse(handle, text, 10)
    assert got[3] == 2 and got[4]["first_bad_line"] == 2
    assert_triplets(got, g.expected(2), "bad lines at 6 and 2")
    g, text = ten_lines(bad=(7,))                                # beyond declared: never parsed, not seen
    got = parse(handle, text, 5)
    assert got[3] == 5 and got[4]["first_bad_line"] == -1
    assert_triplets(got, g.expected(5), "bad line beyond declared")


def test_a_slow_line_that_is_bad_joins_the_minimum(handle):
    g, text = ten_lines(bad=(6,), slow_bad=(3,))
    got = parse(handle, text, 10)
    assert got[4]["slow_lines"] == 1 and got[4]["first_bad_line"] == 3 and got[3] == 3
    assert_triplets(got, g.expected(3), "slow bad line at 3, bad line at 6")
    g, text = ten_lines(bad=(2,), slow_bad=(8,))                 # the other way round
    got = parse(handle, text, 10)
    assert got[4]["slow_lines"] == 1 and got[4]["first_bad_line"] == 2 and got[3] == 2


# ---- the crafted table -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """[(line bytes, fields, from, to, value bits, slow)] as the host program's strtol / strtol / strtof see the lines"""
    subprocess.check_call(["make", "-s", "-f", "edges.mk", "-C", CPP, "edge_scan_check.x"])
    out = tmp_path_factory.mktemp("edges") / "table.txt"
    subprocess.check_call([os.path.join(CPP, "edge_scan_check.x"), "--table", str(out)])
    rows = []
    for ln in out.read_text().splitlines():
        hexline, fields, a, b, bits, slow = ln.split()
        rows.append((b"" if hexline == "-" else bytes.fromhex(hexline), int(fields), int(a), int(b), int(bits), int(slow)))
    assert len(rows) == 39 and sum(r[5] for r in rows) == 11
    return rows


def test_crafted_table_line_by_line(handle, table):
    for line, fields, a, b, bits, slow in table:
        r, c, v, n, st = parse(handle, line + b"\n", 1)
        what = repr(line)
        assert st["slow_lines"] == slow and st["lines"] == 1, what
        if fields < 2:
            assert n == 0 and st["first_bad_line"] == 0, what
        else:
            want_bits = bits if fields == 3 else int(np.float32(1.0).view(np.uint32))
            assert n == 1 and st["first_bad_line"] == -1, what
            assert (int(r[0]), int(c[0]), int(v[0])) == (a, b, want_bits), what


def test_crafted_table_as_one_text(handle, table):
    text = b"\n".join(row[0] for row in table) + b"\n"
    *_, n, st = parse(handle, text, len(table))
    first_bad = [k for k, row in enumerate(table) if row[1] < 2][0]
    assert st["slow_lines"] == sum(row[5] for row in table) == 11            # every line up to declared is looked at
    assert (n, st["first_bad_line"], st["lines"]) == (first_bad, first_bad, len(table))
    good = [row for row in table if row[1] >= 2]
    r, c, v, n, st = parse(handle, b"\n".join(row[0] for row in good), len(good), one_based=True, transpose=True)
    assert n == len(good) and st["slow_lines"] == sum(row[5] for row in good) and st["first_bad_line"] == -1
    one = int(np.float32(1.0).view(np.uint32))
    want_r = np.array([row[3] for row in good], np.int64) - 1                 # transposed: row = second number, minus 1
    want_c = np.array([row[2] for row in good], np.int64) - 1
    assert np.array_equal(r, want_r.astype(np.int32)) and np.array_equal(c, want_c.astype(np.int32))
    assert v.tolist() == [row[4] if row[1] == 3 else one for row in good]


# ---- files -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    d = tmp_path_factory.mktemp("edge_lists")
    _edge_file(d / "lf.snap", n=20000, declared=20000, rows=5000, seed=11)
    _edge_file(d / "crlf.snap", n=20000, declared=20000, rows=5000, seed=12, crlf=True, three=True)
    return {"lf.snap": str(d / "lf.snap"), "crlf.snap": str(d / "crlf.snap")}


def file_path(name, generated):
    return generated[name] if name in generated else os.path.join(DATA, name)


@pytest.mark.parametrize("isTrans", [False, True])
@pytest.mark.parametrize("name", FILES + ["lf.snap", "crlf.snap"])
def test_files_against_the_oracle_loader(handle, generated, name, isTrans):
    path = file_path(name, generated)
    data = open(path, "rb").read()
    h = hs.edge_text_header(data)
    rows, cols, ri, ci, v = po.read_snap(path, isTrans)
    assert (h["rows"], h["cols"]) == (rows, cols) and not h["symmetric"]
    got = parse(handle, data[h["data_offset"]:], h["declared"], one_based=h["one_based"], transpose=isTrans)
    assert_triplets(got, (ri, ci, v.view(np.uint32)), f"{name} isTrans={isTrans}")
    for flags, mode in ((hs.COO_DEDUPE, 0), (hs.COO_SELF_LOOPS | hs.COO_ROW_NORMALISE, 1)):
        d = hs.read_edge_file(path, isTrans, flags, handle)
        try:
            assert d.edge_stats["entries"] == len(ri)
            assert_bits(d.toCpuCSR(), po.load(path, isTrans, mode=mode), f"{name} isTrans={isTrans} mode={mode}")
        finally:
            d.deviceDispose()


def mirror_load(path, isTrans, flags, out):
    subprocess.check_call(["make", "-s", "-f", "edges.mk", "-C", CPP, "edges_check.x"])
    r = subprocess.run([os.path.join(CPP, "edges_check.x"), "load", path, str(int(isTrans)), str(flags), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(out, dtype=np.int32)
    rows, cols, nnz = (int(x) for x in raw[:3])
    rp = raw[3:4 + rows]
    return po.CSRHost(rp, raw[4 + rows:4 + rows + nnz], raw[4 + rows + nnz:4 + rows + 2 * nnz].view(np.float32), rows, cols), r.stdout


def test_symmetric_file_is_refused_by_the_abi_and_loaded_by_the_mirror(handle, tmp_path):
    path = os.path.join(DATA, "own_sym.mtx")
    with pytest.raises(hs.SpgemmError, match="host loader"):
        hs.read_edge_file(path, False, hs.COO_DEDUPE, handle)
    got, _ = mirror_load(path, False, hs.COO_DEDUPE, tmp_path / "sym.bin")          # the host path behind the same call
    assert_bits(got, po.load(path, False, mode=0), "own_sym.mtx through the mirror")


@pytest.mark.parametrize("name, isTrans, flags, mode", [("test2.mtx", True, 1, 0), ("own_graph.snap", True, 6, 1),
                                                       ("lf.snap", False, 1, 0)])
def test_cpp_mirror_loads_what_the_oracle_loads(generated, tmp_path, name, isTrans, flags, mode):
    path = file_path(name, generated)
    got, out = mirror_load(path, isTrans, flags, tmp_path / "m.bin")
    assert_bits(got, po.load(path, isTrans, mode=mode), name)
    assert re.search(r"device parse: lines=\d+ entries=(\d+)", out).group(1) == str(len(po.read_snap(path, isTrans)[2]))


# ---- the device entry, reuse -------------------------------------------------------------------------------------------
def parse_on_device(handle, text, declared, flags=0):
    d = hs.h2d(np.frombuffer(bytes(text), np.uint8))             # a pool block: aligned far beyond 16 bytes
    try:
        r, c, v, n, st = hs.parse_edge_lines_raw(handle, d, len(text), declared, flags)
    finally:
        hs.dev_free(d)
    try:
        return hs.d2h(r, n, np.int32), hs.d2h(c, n, np.int32), hs.d2h(v, n, np.uint32), n, st
    finally:
        for p in (r, c, v):
            hs.dev_free(p)


def slow_text():
    """every fourth line holds a value the device hands to the host: a float midpoint, 17 digits, inf, a huge exponent"""
    g = Gen(8)
    slow = ["16777217.0", "0.10000000000000001", "inf", "1e30"]
    for k in range(600):
        g.line(v=slow[(k // 4) % 4] if k % 4 == 1 else "rand")
    return g


def test_device_text_entry_equals_the_host_text_entry(handle):
    g = Gen(9).fill_to(3 * T + 333)
    a, b = parse(handle, g.text, len(g.rows)), parse_on_device(handle, g.text, len(g.rows))
    assert_triplets(b, g.expected(), "device text")
    assert [x.tobytes() for x in a[:3]] == [x.tobytes() for x in b[:3]] and a[3] == b[3]
    s = slow_text()
    a, b = parse(handle, s.text, 600, transpose=True), parse_on_device(handle, s.text, 600, hs.EDGES_TRANSPOSE)
    assert a[4]["slow_lines"] == b[4]["slow_lines"] == 150 and a[3] == b[3] == 600       # only those lines were copied back
    want = s.expected()
    assert_triplets(a, (want[1], want[0], want[2]), "slow lines, host text")
    assert_triplets(b, (want[1], want[0], want[2]), "slow lines, device text")
    inf = int(np.float32(np.inf).view(np.uint32))
    assert np.count_nonzero(a[2] == inf) == 150 // 4 + (1 if 150 % 4 > 2 else 0)


def test_handle_is_usable_after_an_error_and_calls_repeat(handle):
    g = Gen(10).fill_to(3 * T + 77)
    outs, n = [C.c_void_p(1) for _ in range(3)], C.c_int(5)
    d = hs.h2d(np.frombuffer(bytes(g.text), np.uint8))
    try:
        rc = hs.lib().hip_parse_edge_lines(handle.ptr, C.c_void_p(d + 4), len(g.text) - 4, 10, 0, *[C.byref(x) for x in outs],
                                           C.byref(n), None)
    finally:
        hs.dev_free(d)
    assert rc == ERR_ARG and [x.value for x in outs] == [None] * 3 and n.value == 0
    with pytest.raises(hs.SpgemmError, match="square"):         # fails behind the parse: the triplets are released
        hs.read_edge_file(os.path.join(DATA, "own_pattern.mtx"), True, hs.COO_SELF_LOOPS, handle)
    first = parse(handle, g.text, len(g.rows))
    again = parse(handle, g.text, len(g.rows))
    assert_triplets(first, g.expected(), "after an error return")
    assert [x.tobytes() for x in first[:3]] == [x.tobytes() for x in again[:3]]
