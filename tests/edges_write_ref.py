"""The reference of the device text writer: the bytes hip_format_csr_edges / hip_csr_to_edge_text / hip_write_edge_file
must produce, from Python's %-formatting of the host arrays (correctly rounded, like the C library's printf) and, for nan
and inf (where Python's spelling differs: it never writes "-nan"), from the C library's snprintf itself."""
import ctypes as C
import ctypes.util
import math

import numpy as np

FIXED6, ROUNDTRIP = 0, 1
ONE_BASED, TRANSPOSE = 1, 2

_libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")
_libc.snprintf.restype = C.c_int


def _c_value(fmt, x):
    buf = C.create_string_buffer(512)
    n = _libc.snprintf(buf, C.c_size_t(512), fmt, C.c_double(x))
    assert 0 < n < 512, n
    return buf.raw[:n]


def _wrap(i):
    """i + 1 as the int it is printed as"""
    return (int(i) + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31


def value_text(x, fmt, dtype):
    """'%.6lf' / '%.9g' (float32) / '%.17g' (float64) of one value"""
    spec = "%.6f" if fmt == FIXED6 else ("%.9g" if np.dtype(dtype) == np.float32 else "%.17g")
    x = float(x)                                  # a float32 promotes exactly, as printf promotes it
    if math.isfinite(x):
        return (spec % x).encode()
    return _c_value(spec.encode(), x)


def outside_class(values, fmt):
    """how many values the device need not format itself: FIXED6 |x| >= 1e15, ROUNDTRIP outside [1e-15, 1e17), zero
    excepted; inf and nan in both"""
    a = np.abs(np.asarray(values, np.float64))
    with np.errstate(invalid="ignore"):
        inside = (a < 1e15) if fmt == FIXED6 else ((a == 0) | ((a >= 1e-15) & (a < 1e17)))
    return int(np.count_nonzero(~inside))


def lines(rowPtr, colInd, values, fmt, flags=0):
    """-> the list of line bytes, one per entry in CSR order"""
    rowPtr = np.asarray(rowPtr, np.int64)
    rows = np.repeat(np.arange(len(rowPtr) - 1, dtype=np.int64), np.diff(rowPtr))
    sep = b"\t" if fmt == FIXED6 else b" "
    out = []
    for r, c, v in zip(rows.tolist(), np.asarray(colInd).tolist(), np.asarray(values)):
        if flags & ONE_BASED:
            r, c = _wrap(r), _wrap(c)
        a, b = (c, r) if flags & TRANSPOSE else (r, c)
        out.append(b"%d" % a + sep + b"%d" % b + sep + value_text(v, fmt, values.dtype) + b"\n")
    return out


class Text:
    """the whole text of a host CSR with the byte offset of every entry (offsets[nnz] = its size)"""

    def __init__(self, M, fmt, flags=0):
        ls = lines(M.rowPtr, M.colInd, M.values, fmt, flags)
        self.offsets = np.zeros(len(ls) + 1, np.int64)
        np.cumsum([len(x) for x in ls], out=self.offsets[1:])
        self.data = b"".join(ls)
        self.rowPtr = np.asarray(M.rowPtr, np.int64)

    def rows(self, row0, row1):
        """the slice of rows [row0, row1)"""
        return self.data[self.offsets[self.rowPtr[row0]]:self.offsets[self.rowPtr[row1]]]


def header(kind, rows, cols, entries):
    size = b"%d %d %d\n" % (rows, cols, entries)
    return {0: b"", 1: size, 2: b"%%MatrixMarket matrix coordinate real general\n" + size}[kind]
