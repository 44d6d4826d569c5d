"""CPU: the device text writer's host side.  The line formatter (csrc/edge_print.hpp) equals snprintf on the crafted
table and on 2 M generated doubles and 2 M floats in both formats, converts every value of the required classes without
the host, and stays inside its line bound (tests/cpp/edge_print_check.cc, built with g++ alone, once more under the
address / undefined-behaviour sanitizers and run stand-alone); every new entry checks its arguments without a GPU;
hip_edge_text_write_header writes what hip_edge_text_header reads; the Python mirror refuses a bad dtype."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from devcsr import built  # noqa: F401
from devcsr import _outs
from helpers import ROOT
from sparse_matrix_with_flops_amd import hipspgemm as hs

ERR_ARG = 2
CPP = os.path.join(ROOT, "tests", "cpp")
ONE = C.c_void_p(16)          # a "device pointer" that is never dereferenced


def make(target):
    subprocess.check_call(["make", "-s", "-f", "edges_write.mk", "-C", CPP, target])
    return os.path.join(CPP, target)


# ---- the formatter against the C library -----------------------------------------------------------------------------
def _formatter_report(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=600)
    rep = {m.group(1): {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(2))}
           for m in re.finditer(r"^\((\w)\) (.*)$", r.stdout, re.M)}
    return r, rep


def _assert_formatter(r, rep):
    assert set(rep) == {"a", "b", "c"}, r.stdout + r.stderr
    for part in rep.values():
        assert part["mismatches"] == 0 and part["fast_missed"] == 0, r.stdout
    a, b, c = rep["a"], rep["b"], rep["c"]
    assert a["must_fast"] >= 1000 and a["slow"] >= 16, r.stdout       # inf, nan, the largest values: 4 signs/types x 2 formats
    # 2 M doubles and 2 M floats, each in both formats; the half drawn inside the classes (4 M lines) must be fast, and of
    # the random bit patterns those that happen to fall inside
    assert b["lines"] == 8000000 and b["must_fast"] > 4000000 and b["lines"] - b["slow"] >= b["must_fast"], r.stdout
    assert c["must_fast"] > 0 and max(p["longest"] for p in rep.values()) <= 11 + 1 + 11 + 1 + 24 + 1, r.stdout
    assert r.returncode == 0 and r.stdout.rstrip().endswith("PASS"), r.stdout + r.stderr


def test_formatter_equals_snprintf():
    _assert_formatter(*_formatter_report(make("edge_print_check.x"), 20240607))


def test_formatter_under_the_sanitizers():
    """the same program built with -fsanitize=address,undefined: every line is written into a heap block of exactly its
    length, so a byte written behind the line aborts the run, and so does a shift or an overflow the integer conversion
    must not make"""
    r, rep = _formatter_report(make("edge_print_check_san.x"), 7)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    _assert_formatter(r, rep)


def test_the_line_bound_is_the_one_the_kernels_size_their_stage_by():
    with open(os.path.join(ROOT, "sparse_matrix_with_flops_amd", "csrc", "edge_print.hpp")) as f:
        src = f.read()
    assert re.search(r"PRINT_LINE_MAX = INDEX_MAX \+ 1 \+ INDEX_MAX \+ 1 \+ VALUE_MAX \+ 1;", src)
    assert int(re.search(r"INDEX_MAX = (\d+);", src).group(1)) == 11 and int(re.search(r"VALUE_MAX = (\d+);", src).group(1)) == 24
    with open(os.path.join(ROOT, "sparse_matrix_with_flops_amd", "csrc", "edges_write_device.hpp")) as f:
        assert "EW_STAGE = EW_THREADS * edgeprint::PRINT_LINE_MAX + 16" in f.read()


# ---- the header: written here, read by the parser's header reader -----------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_written_header_reads_back(kind):
    head = hs.edge_text_write_header(kind, 12, 34, 5)
    want = {0: b"", 1: b"12 34 5\n", 2: b"%%MatrixMarket matrix coordinate real general\n12 34 5\n"}[kind]
    assert head == want
    if kind == 0:
        return
    got = hs.edge_text_header(head + b"1 2 0.5\n")
    assert (got["rows"], got["cols"], got["declared"]) == (12, 34, 5)
    assert got["one_based"] == (kind == 2) and not got["symmetric"] and got["data_offset"] == len(head)


def test_header_sizes_up_to_the_largest():
    head = hs.edge_text_write_header(2, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 62)
    got = hs.edge_text_header(head)
    assert (got["rows"], got["cols"]) == (2 ** 31 - 1, 2 ** 31 - 1) and got["data_offset"] == len(head)


def test_header_argument_errors():
    fn = hs.lib().hip_edge_text_write_header
    buf, n = C.create_string_buffer(128), C.c_size_t(7)
    assert fn(buf, 128, 1, 3, 3, 3, None) == ERR_ARG
    for kind in (-1, 3, 1 << 20):
        assert fn(buf, 128, kind, 3, 3, 3, C.byref(n)) == ERR_ARG and n.value == 0
    assert fn(buf, 128, 1, -1, 3, 3, C.byref(n)) == ERR_ARG and fn(buf, 128, 1, 3, -1, 3, C.byref(n)) == ERR_ARG
    assert fn(buf, 128, 1, 3, 3, -1, C.byref(n)) == ERR_ARG
    assert fn(buf, 5, 1, 3, 3, 3, C.byref(n)) == ERR_ARG and n.value == 0          # "3 3 3\n" needs 6 bytes
    assert fn(None, 128, 1, 3, 3, 3, C.byref(n)) == ERR_ARG
    assert fn(None, 0, 0, 3, 3, 3, C.byref(n)) == 0 and n.value == 0                # nothing to write: no buffer needed
    assert fn(buf, 6, 1, 3, 3, 3, C.byref(n)) == 0 and n.value == 6 and buf.raw[:6] == b"3 3 3\n"
    assert hs.lib().spgemm_hip_last_error()


# ---- argument errors: no device is touched ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["hip_format_csr_edges", "hip_format_csr_edges_f64", "hip_csr_to_edge_text",
                                   "hip_csr_to_edge_text_f64"])
def test_range_entries_argument_errors_do_not_need_a_gpu(entry):
    fn = getattr(hs.lib(), entry)
    to_host = "to_edge_text" in entry

    def call(m=4, n=4, arrays=(ONE, ONE, ONE), row0=0, row1=4, fmt=0, flags=0, text="out", nbytes="out", st=None):
        t, nb = C.c_void_p(1), C.c_size_t(7)
        out = ([None, 0] if to_host else [C.byref(t)]) if text == "out" else ([text, 0] if to_host else [text])
        rc = fn(None, m, n, *arrays, row0, row1, fmt, flags, *out, C.byref(nb) if nbytes == "out" else nbytes, st)
        return rc, t.value, nb.value

    assert call(nbytes=None)[0] == ERR_ARG
    if not to_host:
        assert call(text=None)[0] == ERR_ARG
    for kw in ({"fmt": 2}, {"fmt": -1}, {"flags": 4}, {"flags": -1}, {"flags": 1 << 16}, {"row0": 3, "row1": 2},
               {"row0": -1}, {"row1": 5}, {"m": -1}, {"n": -1}):
        rc, t, nb = call(**kw)
        assert rc == ERR_ARG and nb == 0 and (to_host or t is None), kw
    for k in range(3):
        arrays = [ONE, ONE, ONE]
        arrays[k] = None
        assert call(arrays=arrays)[0] == ERR_ARG                                    # a null CSR array with m > 0
    st = hs.EdgeWriteStats()
    st.entries = st.bytes = st.slabs = 9
    assert call(fmt=7, st=C.byref(st))[0] == ERR_ARG
    assert (st.entries, st.bytes, st.slow_entries, st.slabs, st.ms_total) == (0, 0, 0, 0, 0.0)
    assert hs.lib().spgemm_hip_last_error()


@pytest.mark.parametrize("entry", ["hip_write_edge_file", "hip_write_edge_file_f64"])
def test_write_file_argument_errors_do_not_need_a_gpu(entry, tmp_path):
    fn = getattr(hs.lib(), entry)
    good = str(tmp_path / "out.txt").encode()

    def call(path=good, m=4, n=4, arrays=(ONE, ONE, ONE), fmt=0, flags=0, header=1, st=None):
        return fn(None, path, m, n, *arrays, fmt, flags, header, st)

    assert call(path=None) == ERR_ARG
    assert call(fmt=2) == ERR_ARG and call(flags=4) == ERR_ARG and call(flags=-1) == ERR_ARG
    assert call(header=3) == ERR_ARG and call(header=-1) == ERR_ARG and call(m=-1) == ERR_ARG
    for k in range(3):
        arrays = [ONE, ONE, ONE]
        arrays[k] = None
        assert call(arrays=arrays) == ERR_ARG
    assert not os.path.exists(good)                                                 # refused before the file is opened
    st = hs.EdgeWriteStats()
    st.entries = st.slabs = 9
    assert call(path=str(tmp_path / "no" / "such" / "dir" / "out.txt").encode(), st=C.byref(st)) == ERR_ARG   # unwritable
    assert call(path=str(tmp_path).encode()) == ERR_ARG                             # a directory
    assert (st.entries, st.slabs) == (0, 0)
    assert b"cannot open" in hs.lib().spgemm_hip_last_error()


def test_python_mirror_refuses_a_bad_dtype_before_device_work(tmp_path):
    dM = hs.CSR(16, 16, 16, 4, 4, 3, True, dtype=np.float32)                        # device "pointers" never dereferenced
    calls = (lambda **kw: hs.format_csr_edges(dM, **kw), lambda **kw: hs.csr_to_edge_text(dM, **kw),
             lambda **kw: hs.write_edge_file(dM, str(tmp_path / "x.txt"), **kw))
    for f in calls:
        for bad in (np.float16, np.int32, "int64", np.complex128):
            with pytest.raises(hs.SpgemmError, match="dtype"):
                f(dtype=bad)
        with pytest.raises(hs.SpgemmError, match="dtype"):
            f(dtype=np.float64)                                                     # not the matrix's
        with pytest.raises(hs.SpgemmError, match="fmt"):
            f(fmt=2)
        for flags in (4, -1, 1 << 20):
            with pytest.raises(hs.SpgemmError, match="flags"):
                f(flags=flags)
    for f in calls[:2]:
        with pytest.raises(hs.SpgemmError, match="rows"):
            f(row0=3, row1=2)
        with pytest.raises(hs.SpgemmError, match="rows"):
            f(row1=5)
    with pytest.raises(hs.SpgemmError, match="header"):
        hs.write_edge_file(dM, str(tmp_path / "x.txt"), header=3)
    with pytest.raises(hs.SpgemmError, match="path"):
        hs.write_edge_file(dM, 7)
    host = hs.CSR.from_arrays([0, 1], [0], [1.0], 1, 1)
    with pytest.raises(hs.SpgemmError, match="device CSR"):
        hs.csr_to_edge_text(host)
    assert not os.path.exists(tmp_path / "x.txt")
    for name in ("hip_edge_text_write_header", "hip_format_csr_edges", "hip_format_csr_edges_f64", "hip_csr_to_edge_text",
                 "hip_csr_to_edge_text_f64", "hip_write_edge_file", "hip_write_edge_file_f64"):
        assert name in hs.EXPORTS
