"""Python reference of the double edge-list loader, for tests/test_gpu_edges_parse_f64.py and tests/test_gpu_coo_f64.py.

  Gen64        writes lines "from to [value]" and keeps the triplets they stand for; the value of a token is Python's
               float(token), which is correctly rounded like strtod
  coo_to_csr   COO::makeOrdered / orderedAndDuplicatesRemoving / toCSR / addSelfLoopIfNeeded / averAndNormRowQValue / toAbs
               for float64 values: numpy's stable argsort on (row, col), every run of equal pairs summed sequentially, left
               to right in input order, in float64
  load         the header by hs.edge_text_header, the tokens by int() / float() under the reference's counting rule, then
               coo_to_csr

pytest does not rewrite the asserts of a helper module: every assert here carries its message."""
import numpy as np

from f64ref import Host64
from sparse_matrix_with_flops_amd import hipspgemm as hs


def bits64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


class Gen64:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.text = bytearray()
        self.rows, self.cols, self.vals = [], [], []

    def line(self, v=None, lead=0, width=0, a=None, b=None, eol=b"\n"):
        """v: the value's text, or None for a line without one (1.0); `lead` blanks in front; padded behind with blanks to
        at least `width` bytes (without the eol)"""
        a = int(self.rng.integers(0, 100000)) if a is None else a
        b = int(self.rng.integers(0, 100000)) if b is None else b
        body = b" " * lead + f"{a} {b}".encode() + (b" " + v.encode() if v is not None else b"")
        body += b" " * max(0, width - len(body))
        self.text += body + eol
        self.rows.append(a); self.cols.append(b)
        self.vals.append(1.0 if v is None else float(v))
        return self

    def mixed(self, eol=b"\n"):
        """one line of the all-fast mix: no value, k / 8, 0.1, the repr() of a double in (1e-10, 1), a float midpoint"""
        k = int(self.rng.integers(0, 5))
        if k == 0:
            return self.line(eol=eol)
        if k == 1:
            return self.line(f"{int(self.rng.integers(0, 4000)) / 8:g}", eol=eol)
        if k == 2:
            return self.line("0.1", eol=eol)
        if k == 3:
            return self.line(repr(float(10.0 ** self.rng.uniform(-9, 0) * self.rng.uniform(0.1, 1.0))), eol=eol)
        return self.line("16777217.0", eol=eol)

    def fill_to(self, nbytes):
        """mixed lines until the text is nbytes long: the last one is padded so that its '\\n' is byte nbytes - 1"""
        while len(self.text) + 80 < nbytes:
            self.mixed()
        return self.line(width=nbytes - len(self.text) - 1)

    def expected(self, n=None):
        n = len(self.rows) if n is None else n
        return np.array(self.rows[:n], np.int32), np.array(self.cols[:n], np.int32), bits64(self.vals[:n])


def coo_to_csr(rows, cols, ri, ci, v, dedupe=True, self_loops=False, row_normalise=False, use_abs=False):
    """-> Host64.  Appended self loops are (i, i, 1.0) behind the input in row order, for every row without a diagonal."""
    ri, ci = np.asarray(ri, np.int64), np.asarray(ci, np.int64)
    v = np.asarray(v, np.float64)
    if self_loops:
        assert rows == cols, "self loops need a square matrix"
        has = np.zeros(rows, bool)
        has[ri[ri == ci]] = True
        miss = np.flatnonzero(~has)
        ri, ci, v = np.r_[ri, miss], np.r_[ci, miss], np.r_[v, np.ones(len(miss))]
    key = ri * max(cols, 1) + ci
    order = np.argsort(key, kind="stable")
    key, v = key[order], v[order]
    n = len(key)
    if dedupe and n:
        starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
        lens = np.diff(np.r_[starts, n])
        acc = v[starts].copy()
        for k in range(1, int(lens.max())):                      # the k-th term of every run that has one: left to right
            m = lens > k
            acc[m] = acc[m] + v[starts[m] + k]
        key, v = key[starts], acc
    if use_abs:
        v = np.abs(v)
    row = key // max(cols, 1)
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=rows), out=rp[1:])
    if row_normalise:
        v = 1.0 / np.repeat(np.diff(rp), np.diff(rp)).astype(np.float64)
    return Host64(rp, key % max(cols, 1), v, rows, cols)


def read_triplets(data, isTrans):
    """(rows, cols, ri, ci, v) of a SNAP / MatrixMarket text under the reference's counting rule: at most `declared` lines,
    reading stops at the first line with fewer than two fields, a missing value is 1.0"""
    h = hs.edge_text_header(data)
    assert not h["symmetric"], "a symmetric file is not line-oriented"
    ri, ci, v = [], [], []
    body = data[h["data_offset"]:]
    lines = body.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for ln in lines[:max(h["declared"], 0)]:
        f = ln.split()
        if len(f) < 2:
            break
        a, b = int(f[0]) - h["one_based"], int(f[1]) - h["one_based"]
        ri.append(b if isTrans else a); ci.append(a if isTrans else b)
        v.append(float(f[2]) if len(f) > 2 else 1.0)
    return h["rows"], h["cols"], np.array(ri, np.int64), np.array(ci, np.int64), np.array(v, np.float64)


def load(path, isTrans, flags):
    with open(path, "rb") as f:
        rows, cols, ri, ci, v = read_triplets(f.read(), isTrans)
    return coo_to_csr(rows, cols, ri, ci, v, dedupe=bool(flags & hs.COO_DEDUPE), self_loops=bool(flags & hs.COO_SELF_LOOPS),
                      row_normalise=bool(flags & hs.COO_ROW_NORMALISE), use_abs=bool(flags & hs.COO_ABS)), len(ri)


def assert_bits64(got, want, what):
    """got: a host hs.CSR with float64 values; want: Host64"""
    assert (got.rows, got.cols, got.nnz) == (want.rows, want.cols, want.nnz), f"{what}: shape / nnz {got.rows, got.cols, got.nnz}"
    assert np.array_equal(got.rowPtr, want.rowPtr), f"{what}: rowPtr"
    assert np.array_equal(got.colInd, want.colInd), f"{what}: colInd"
    assert got.values.dtype == np.float64, f"{what}: values are {got.values.dtype}"
    g, w = bits64(got.values), bits64(want.values)
    assert np.array_equal(g, w), f"{what}: value bits differ first at {int(np.flatnonzero(g != w)[0]) if len(g) == len(w) else -1}"
