"""CPU: the device text parser's host side.  hip_edge_text_header reads the banner / comments / size line as the reference
loader does (through the oracle's restatement po.read_snap); the number scanner shared by host and device
(csrc/edge_scan.hpp) equals strtol / strtol / strtof on generated lines and on the crafted table
(tests/cpp/edge_scan_check.cc, built with g++ alone, once more under the address / undefined-behaviour sanitizers and
run stand-alone); the three device entries check their arguments without a GPU; the Python mirror refuses non-bytes input
and bad flags before any device work."""
import ctypes as C
import os
import re
import subprocess

import pytest

from devcsr import built  # noqa: F401
from devcsr import _outs
from helpers import DATA, ROOT, po
from sparse_matrix_with_flops_amd import hipspgemm as hs

ERR_ARG, ERR_OVERFLOW, ERR_INPUT = 2, 3, 5
CPP = os.path.join(ROOT, "tests", "cpp")
ONE = C.c_void_p(16)          # a "device pointer" that is never dereferenced


def make(target):
    subprocess.check_call(["make", "-s", "-f", "edges.mk", "-C", CPP, target])
    return os.path.join(CPP, target)


# ---- the header ------------------------------------------------------------------------------------------------------
def own_size_line(data):
    """the numbers of the first line that is no comment, read by hand"""
    for ln in data.split(b"\n"):
        if not ln.startswith((b"#", b"%")):
            return [int(x) for x in ln.split()[:3]]
    return None


@pytest.mark.parametrize("name", sorted(os.listdir(DATA)))
def test_header_of_every_fixture_file(name):
    path = os.path.join(DATA, name)
    data = open(path, "rb").read()
    h = hs.edge_text_header(data)
    rows, cols, ri, _, _ = po.read_snap(path, False)
    assert (h["rows"], h["cols"]) == (rows, cols)
    nums = own_size_line(data)
    assert h["declared"] == nums[-1] and h["rows"] == nums[0]
    assert h["one_based"] == name.endswith(".mtx") and h["symmetric"] == (b"symmetric" in data.split(b"\n")[0])
    cap = h["declared"] * (2 if h["symmetric"] else 1)
    lines = [ln for ln in data[h["data_offset"]:].split(b"\n") if ln.strip()]
    if len(lines) >= h["declared"] and not h["symmetric"]:
        assert len(ri) == h["declared"]                    # the entry cap the loader reports
    else:
        assert len(ri) <= cap                              # a short file: declared is the file's own size line (above)
    assert data[:h["data_offset"]].endswith(b"\n") and data[:h["data_offset"]].split(b"\n")[-2].split() == [str(x).encode() for x in nums]


HEADS = [
    # text, rows, cols, declared, one_based, symmetric, what lies at data_offset
    (b"7 9\n1 2\n", 7, 7, 9, False, False, b"1 2\n"),
    (b"7 8 9\n1 2\n", 7, 8, 9, False, False, b"1 2\n"),
    (b"# a\r\n# b\r\n7 8 9\r\n1 2\r\n", 7, 8, 9, False, False, b"1 2\r\n"),
    (b"# a\n% b\n#\n5 3\n", 5, 5, 3, False, False, b""),
    (b"%%MatrixMarket matrix coordinate real general\n% c\n4 5 6\n1 1 2.0\n", 4, 5, 6, True, False, b"1 1 2.0\n"),
    (b"%%MatrixMarket matrix coordinate real SYMMETRIC\n4 4 6\n1 1\n", 4, 4, 6, True, True, b"1 1\n"),
    (b"%%MatrixMarket matrix coordinate real\n4 4 6\n", 4, 4, 6, False, False, b""),          # 4 tokens: no banner
]


@pytest.mark.parametrize("case", HEADS, ids=[repr(c[0][:24]) for c in HEADS])
def test_header_of_generated_heads(case, tmp_path):
    text, rows, cols, declared, one, sym, rest = case
    h = hs.edge_text_header(text)
    assert (h["rows"], h["cols"], h["declared"], h["one_based"], h["symmetric"]) == (rows, cols, declared, one, sym)
    assert text[h["data_offset"]:] == rest
    p = tmp_path / "head.txt"                                 # the same numbers through the reference loader's restatement
    p.write_bytes(text)
    r, c, _, _, _ = po.read_snap(str(p), False)
    assert (r, c) == (rows, cols)


def test_header_without_a_size_line_and_empty():
    for text in (b"# only\nnot numbers\n1 2\n", b"# c\n5\n", b"\n1 2\n"):
        with pytest.raises(hs.SpgemmError, match="size line"):
            hs.edge_text_header(text)
    L = hs.lib()
    z = [C.c_int(7) for _ in range(5)] + [C.c_size_t(7)]
    assert L.hip_edge_text_header(b"x y\n", 4, *[C.byref(x) for x in z]) == ERR_INPUT
    assert [x.value for x in z] == [0] * 6
    for text in (b"", b"# a\n% b\n", b"# no newline"):
        h = hs.edge_text_header(text)
        assert (h["rows"], h["cols"], h["declared"], h["data_offset"]) == (0, 0, 0, 0) and not h["symmetric"]
    h = hs.edge_text_header(b"%%MatrixMarket matrix coordinate real symmetric\n")    # the banner alone says which loader
    assert h["symmetric"] and h["one_based"] and h["declared"] == 0
    assert hs.edge_text_header(b"3 -2\n")["declared"] == -2                          # as written; the parse reads it as 0
    # a size line that ends the file without '\n' is read as COO::readSNAPFile of the mirror reads it (the reference stops
    # at the end of file and reports an empty matrix; no entry follows either way)
    h = hs.edge_text_header(b"3 4")
    assert (h["rows"], h["cols"], h["declared"], h["data_offset"]) == (3, 3, 4, 3)
    assert L.hip_edge_text_header(None, 5, *[C.byref(x) for x in z]) == ERR_ARG
    for k in range(6):
        refs = [C.byref(x) for x in z]
        refs[k] = None
        assert L.hip_edge_text_header(b"1 2\n", 4, *refs) == ERR_ARG


# ---- the scanner against the C library -------------------------------------------------------------------------------
def _scanner_report(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=600)
    rep = {m.group(1): {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(2))}
           for m in re.finditer(r"^\((\w)\) (.*)$", r.stdout, re.M)}
    return r, rep


def _assert_scanner(r, rep):
    assert set(rep) == {"a", "b", "c"}, r.stdout + r.stderr
    assert rep["a"]["lines"] == 1000000 and rep["a"]["mismatches"] == 0 and rep["a"]["slow"] == 0, r.stdout
    assert rep["b"]["lines"] == 1000000 and rep["b"]["mismatches"] == 0, r.stdout
    assert rep["c"]["mismatches"] == 0 and rep["c"]["wrong_slow_flags"] == 0 and rep["c"]["slow"] == 11, r.stdout
    assert r.returncode == 0 and r.stdout.rstrip().endswith("PASS"), r.stdout + r.stderr


def test_scanner_equals_strtol_and_strtof():
    _assert_scanner(*_scanner_report(make("edge_scan_check.x"), 20240607))


def test_scanner_under_the_sanitizers():
    """the same program built with -fsanitize=address,undefined: every line is handed over in an exact-size heap copy, so
    a read behind the line's end aborts the run"""
    r, rep = _scanner_report(make("edge_scan_check_san.x"), 7)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    _assert_scanner(r, rep)


# ---- argument errors: no device is touched ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["hip_parse_edge_lines", "hip_parse_edge_text"])
def test_parse_argument_errors_do_not_need_a_gpu(entry):
    fn = getattr(hs.lib(), entry)
    n = C.c_int(7)
    text = ONE if entry == "hip_parse_edge_lines" else b"1 2\n3 4\n"

    def call(text=text, nbytes=8, declared=2, flags=0, outs=None, count=C.byref(n), st=None):
        o = outs if outs is not None else [C.byref(x) for x in _outs(3)]
        return fn(None, text, nbytes, declared, flags, *o, count, st)

    for k in range(3):
        o = [C.byref(x) for x in _outs(3)]
        o[k] = None
        assert call(outs=o) == ERR_ARG
    assert call(count=None) == ERR_ARG
    assert call(text=None) == ERR_ARG                          # null text with nbytes > 0
    assert call(flags=4) == ERR_ARG and call(flags=-1) == ERR_ARG and call(flags=1 << 16) == ERR_ARG
    assert call(nbytes=2 ** 31) == ERR_OVERFLOW and call(nbytes=2 ** 33 + 5) == ERR_OVERFLOW
    assert hs.lib().spgemm_hip_last_error()
    if entry == "hip_parse_edge_lines":
        for bad in (1, 8, 17, 4096 + 4):
            assert call(text=C.c_void_p(bad)) == ERR_ARG        # the device text must be 16-byte aligned
    outs, st = _outs(3), hs.EdgeStats()
    st.lines = st.entries = 9
    assert call(flags=8, outs=[C.byref(x) for x in outs], st=C.byref(st)) == ERR_ARG
    assert [x.value for x in outs] == [None] * 3 and n.value == 0
    assert (st.lines, st.entries, st.slow_lines, st.first_bad_line) == (0, 0, 0, -1)


def test_read_file_argument_errors_do_not_need_a_gpu(tmp_path):
    fn = hs.lib().hip_read_edge_file
    rows, cols, nnz = C.c_int(7), C.c_int(7), C.c_int(7)
    good = os.path.join(DATA, "own_graph.snap").encode()

    def call(path=good, outs=None, r=C.byref(rows), c=C.byref(cols), count=C.byref(nnz)):
        o = outs if outs is not None else [C.byref(x) for x in _outs(3)]
        return fn(None, path, 1, 1, r, c, *o, count, None)

    for k in range(3):
        o = [C.byref(x) for x in _outs(3)]
        o[k] = None
        assert call(outs=o) == ERR_ARG
    assert call(r=None) == ERR_ARG and call(c=None) == ERR_ARG and call(count=None) == ERR_ARG
    assert call(path=None) == ERR_ARG
    assert call(path=str(tmp_path / "absent.snap").encode()) == ERR_ARG
    assert call(path=str(tmp_path).encode()) == ERR_ARG                        # a directory is not readable as a file
    outs = _outs(3)
    assert call(path=os.path.join(DATA, "own_sym.mtx").encode(), outs=[C.byref(x) for x in outs]) == ERR_INPUT
    assert b"host loader" in hs.lib().spgemm_hip_last_error()
    assert [x.value for x in outs] == [None] * 3 and (rows.value, cols.value, nnz.value) == (0, 0, 0)
    bad = tmp_path / "nosize.snap"
    bad.write_bytes(b"# c\nno size line\n")
    assert call(path=str(bad).encode()) == ERR_INPUT


def test_python_mirror_refuses_before_device_work():
    for data in ("1 2\n", 12, None, [b"1 2\n"]):
        with pytest.raises(hs.SpgemmError, match="bytes"):
            hs.parse_edge_text(data, 1)
        with pytest.raises(hs.SpgemmError, match="bytes"):
            hs.edge_text_header(data)
    for flags in (4, -1, 1 << 20):
        with pytest.raises(hs.SpgemmError, match="flags"):
            hs.parse_edge_lines_raw(None, 16, 8, 2, flags)
    with pytest.raises(hs.SpgemmError, match="flags"):
        hs.read_edge_file(os.path.join(DATA, "own_graph.snap"), flags=16)
    with pytest.raises(hs.SpgemmError, match="path"):
        hs.read_edge_file(12)
    with pytest.raises(hs.SpgemmError, match="host loader"):
        hs.read_edge_file(os.path.join(DATA, "own_sym.mtx"))
