"""CPU: the double edge-list loader's host side.  The double scanner (csrc/edge_scan.hpp: scan_double /
edge_scan_line_f64) equals strtol / strtol / strtod on the crafted table and on 2 M generated tokens, and every token of
the required fast class (at most 19 significant digits, |e10| <= 27) is converted without the host
(tests/cpp/edge_scan_f64_check.cc, built with g++ alone, once more under the address / undefined-behaviour sanitizers and
run stand-alone); the four _f64 entries check their arguments without a GPU; the Python mirror refuses a bad dtype."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from devcsr import built  # noqa: F401
from devcsr import _outs
from helpers import DATA, ROOT
from sparse_matrix_with_flops_amd import hipspgemm as hs

ERR_ARG, ERR_OVERFLOW, ERR_INPUT = 2, 3, 5
CPP = os.path.join(ROOT, "tests", "cpp")
ONE = C.c_void_p(16)          # a "device pointer" that is never dereferenced


def make(target):
    subprocess.check_call(["make", "-s", "-f", "edges_f64.mk", "-C", CPP, target])
    return os.path.join(CPP, target)


# ---- the scanner against the C library -------------------------------------------------------------------------------
def _scanner_report(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=600)
    rep = {m.group(1): {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", m.group(2))}
           for m in re.finditer(r"^\((\w)\) (.*)$", r.stdout, re.M)}
    return r, rep


def _assert_scanner(r, rep):
    assert set(rep) == {"a", "b"}, r.stdout + r.stderr
    a, b = rep["a"], rep["b"]
    assert a["mismatches"] == 0 and a["fast_missed"] == 0 and a["wrong_slow"] == 0, r.stdout
    assert a["must_fast"] >= 40 and a["slow"] >= 7, r.stdout          # the table's fast rows; inf / nan / hex / a clamped index
    assert b["lines"] == 2000000 and b["mismatches"] == 0 and b["fast_missed"] == 0, r.stdout
    # 19 of 21 digit counts and 55 of 61 exponents are required fast: about 1.63 M of the 2 M tokens; the scanner may
    # convert more than that, never fewer
    assert b["must_fast"] > 1500000 and b["lines"] - b["slow"] >= b["must_fast"], r.stdout
    assert r.returncode == 0 and r.stdout.rstrip().endswith("PASS"), r.stdout + r.stderr


def test_double_scanner_equals_strtol_and_strtod():
    _assert_scanner(*_scanner_report(make("edge_scan_f64_check.x"), 20240607))


def test_double_scanner_under_the_sanitizers():
    """the same program built with -fsanitize=address,undefined: every line is handed over in an exact-size heap copy, so
    a read behind the line's end aborts the run, and so does a shift or an overflow the integer conversion must not make"""
    r, rep = _scanner_report(make("edge_scan_f64_check_san.x"), 7)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    _assert_scanner(r, rep)


# ---- argument errors: no device is touched ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["hip_parse_edge_lines_f64", "hip_parse_edge_text_f64"])
def test_parse_argument_errors_do_not_need_a_gpu(entry):
    fn = getattr(hs.lib(), entry)
    n = C.c_int(7)
    text = ONE if entry == "hip_parse_edge_lines_f64" else b"1 2\n3 4\n"

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
    if entry == "hip_parse_edge_lines_f64":
        for bad in (1, 8, 17, 4096 + 4):
            assert call(text=C.c_void_p(bad)) == ERR_ARG        # the device text must be 16-byte aligned
    outs, st = _outs(3), hs.EdgeStats()
    st.lines = st.entries = 9
    assert call(flags=8, outs=[C.byref(x) for x in outs], st=C.byref(st)) == ERR_ARG
    assert [x.value for x in outs] == [None] * 3 and n.value == 0
    assert (st.lines, st.entries, st.slow_lines, st.first_bad_line) == (0, 0, 0, -1)


def test_read_file_argument_errors_do_not_need_a_gpu(tmp_path):
    fn = hs.lib().hip_read_edge_file_f64
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


def test_coo_argument_errors_do_not_need_a_gpu():
    fn = hs.lib().hip_coo_to_csr_f64
    n = C.c_int(7)

    def call(rows=3, cols=3, nnz=2, arrays=(ONE, ONE, ONE), flags=1, outs=None, count=C.byref(n)):
        o = outs if outs is not None else [C.byref(x) for x in _outs(3)]
        return fn(None, rows, cols, nnz, *arrays, flags, *o, count)

    for k in range(3):
        o = [C.byref(x) for x in _outs(3)]
        o[k] = None
        assert call(outs=o) == ERR_ARG
    assert call(count=None) == ERR_ARG
    assert call(rows=-1) == ERR_ARG and call(cols=-1) == ERR_ARG and call(nnz=-1) == ERR_ARG
    for k in range(3):
        arrays = [ONE, ONE, ONE]
        arrays[k] = None
        assert call(arrays=arrays) == ERR_ARG                                  # a null COO array with nnz > 0
    outs = _outs(3)
    assert call(rows=3, cols=4, flags=2, outs=[C.byref(x) for x in outs]) == ERR_ARG    # self loops on a non-square matrix
    assert b"square" in hs.lib().spgemm_hip_last_error()
    assert [x.value for x in outs] == [None] * 3 and n.value == 0


def test_python_mirror_refuses_a_bad_dtype_before_device_work():
    path = os.path.join(DATA, "own_graph.snap")
    for bad in (np.float16, np.int32, "int64", np.complex128):
        with pytest.raises(hs.SpgemmError, match="dtype"):
            hs.parse_edge_text(b"1 2\n", 1, dtype=bad)
        with pytest.raises(hs.SpgemmError, match="dtype"):
            hs.read_edge_file(path, dtype=bad)
        with pytest.raises(hs.SpgemmError, match="dtype"):
            hs.coo_to_csr(2, 2, [0], [1], [1.0], hs.COO_DEDUPE, dtype=bad)
    for flags in (4, -1, 1 << 20):
        with pytest.raises(hs.SpgemmError, match="flags"):
            hs.parse_edge_lines_raw_f64(None, 16, 8, 2, flags)
    with pytest.raises(hs.SpgemmError, match="flags"):
        hs.read_edge_file(path, flags=16, dtype=np.float64)
    with pytest.raises(hs.SpgemmError, match="host loader"):
        hs.read_edge_file(os.path.join(DATA, "own_sym.mtx"), dtype=np.float64)
    with pytest.raises(hs.SpgemmError, match="bytes"):
        hs.parse_edge_text("1 2\n", 1, dtype=np.float64)
    # the keyword is the last parameter of each: positional calls keep their meaning
    import inspect
    for fn in (hs.coo_to_csr, hs.parse_edge_text, hs.read_edge_file):
        assert list(inspect.signature(fn).parameters)[-1] == "dtype"
