"""GPU (-m gpu): comparing two device CSRs on the device -- hip_csr_diff (the report, CSR::differs, the isEqual /
isRelativeEqual / parity predicates) and hip_csr_differsStats -- in float32 and float64 against the numpy restatement
tests/compare_ref.py (pinned in tests/test_compare_abi.py).  Integer fields, first rows and maxima are exact (each maximum
is one double operation on exactly converted inputs); sum_sq is held to the worst-case bound of a double summation of N
non-negative terms.  float64 values carry bits beyond float32 (x + 2^-40), so a pass through float would show.  The last
tests go through the product path and the C++ mirror."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import compare_ref as cr
from reorder_ref import Host
from devcsr import built_gpu, handle  # noqa: F401
from helpers import DATA, ROOT, synth_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
ERR_INPUT = 5
CMP_TILE = 1024         # work items (entries of A, then of B) per block of the walk (compare_device.hpp)
INT_FIELDS = ("rows_len_differ", "first_len_row", "only_a", "only_b", "first_only_row", "beyond", "first_beyond_row")
MAX_FIELDS = ("max_abs_err", "max_rel_err", "max_abs_only_a", "max_abs_only_b")
REF_PERCENTS = [-30, -20, -5, 0, 5, 20, 30, 100]


# ---- inputs (made once per name, never modified) ---------------------------------------------------------------------
def from_flat(pos, values, rows, cols):
    """sorted distinct flat positions row * cols + col -> CSR with strictly ascending rows"""
    pos = np.asarray(pos, np.int64)
    rp = np.zeros(rows + 1, np.int32)
    if rows:
        np.cumsum(np.bincount(pos // max(cols, 1), minlength=rows), out=rp[1:])
    return Host(rp, pos % max(cols, 1), values, rows, cols)


def typed_pair(rows, cols, nnzA, seed, drop, insert, dtype):
    """-> (A, B) with strictly ascending rows.  B is A after a seeded edit: `drop` entries dropped, `insert` inserted, a
    fifth of the values scaled by 1 +- 1e-3, a fifth by 1 +- 1e-8 (no change at all in float32), the rest bit-identical."""
    rng = np.random.default_rng(seed)
    f64 = np.dtype(dtype) == np.float64
    picked = rng.choice(rows * cols, size=nnzA + insert, replace=False) if rows * cols else np.zeros(0, np.int64)
    posA, posI = np.sort(picked[:nnzA]), picked[nnzA:]

    def values(n):                                          # float32 numbers of either sign; float64 gets bits beyond float32
        v = ((rng.random(n) + 0.25) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32).astype(np.float64)
        return v + 2.0 ** -40 if f64 else v
    va, vi = values(nnzA), values(insert)
    kind, sign = rng.integers(0, 5, size=nnzA), rng.choice([-1.0, 1.0], size=nnzA)
    scale = np.where(kind == 0, 1.0 + sign * 1e-3, np.where(kind == 1, 1.0 + sign * 1e-8, 1.0))
    keep = np.ones(nnzA, bool)
    keep[rng.choice(nnzA, size=drop, replace=False)] = False
    posB, vb = np.concatenate([posA[keep], posI]), np.concatenate([(va * scale)[keep], vi])
    order = np.argsort(posB)
    return from_flat(posA, va.astype(dtype), rows, cols), from_flat(posB[order], vb[order].astype(dtype), rows, cols)


def long_row_pair(dtype):
    """300 x 40 000: row 17 holds 20 000 strictly ascending columns in A and, in B, half of those plus 10 000 others;
    every other row is empty"""
    rng = np.random.default_rng(17)
    cols = rng.permutation(40000)
    ca, extra = np.sort(cols[:20000]), cols[20000:30000]
    va = (rng.random(20000) + 0.25).astype(np.float32).astype(np.float64)
    if np.dtype(dtype) == np.float64:
        va = va + 2.0 ** -40
    half = np.sort(rng.choice(20000, size=10000, replace=False))
    scale = np.where(rng.integers(0, 4, size=10000) == 0, 1.0 + 1e-3, 1.0)
    cb = np.concatenate([ca[half], extra])
    vb = np.concatenate([va[half] * scale, (rng.random(10000) + 0.25).astype(np.float32).astype(np.float64)])
    order = np.argsort(cb)
    rp = np.zeros(301, np.int32)
    rp[18:] = 20000
    return Host(rp, ca, va.astype(dtype), 300, 40000), Host(rp, cb[order], vb[order].astype(dtype), 300, 40000)


T = CMP_TILE
SHAPES = {
    "0x0": lambda dt: typed_pair(0, 0, 0, 1, 0, 0, dt),
    "5x7 both empty": lambda dt: typed_pair(5, 7, 0, 2, 0, 0, dt),
    "A empty": lambda dt: typed_pair(61, 97, 0, 3, 0, 300, dt),
    "B empty": lambda dt: typed_pair(61, 97, 300, 4, 300, 0, dt),
    # nnzA + nnzB = T - 1, T, T + 1 (nnzB = 520 - 60 + insert)
    "total T-1": lambda dt: typed_pair(61, 97, 520, 5, 60, T - 1 - 980, dt),
    "total T": lambda dt: typed_pair(61, 97, 520, 6, 60, T - 980, dt),
    "total T+1": lambda dt: typed_pair(61, 97, 520, 7, 60, T + 1 - 980, dt),
    # nnzA = T - 1, T, T + 1: the A / B seam on a block edge
    "nnzA T-1": lambda dt: typed_pair(61, 97, T - 1, 8, 50, 70, dt),
    "nnzA T": lambda dt: typed_pair(61, 97, T, 9, 50, 70, dt),
    "nnzA T+1": lambda dt: typed_pair(61, 97, T + 1, 10, 50, 70, dt),
    "1000x257": lambda dt: typed_pair(1000, 257, 5000, 11, 400, 450, dt),
    "257x1000": lambda dt: typed_pair(257, 1000, 5000, 12, 400, 450, dt),
    "long row": long_row_pair,
}


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """-> (A, B, restated report, fsum of the double terms, the float32 sequential CSR::differs or None)"""
    A, B = SHAPES[name](dtype)
    rep, terms = cr.report(A, B, rel=1e-6, abs_tol=0.0)
    seq = cr.differs_f32(A, B) if np.dtype(dtype) == np.float32 else None
    return A, B, rep, cr.sum_sq(terms), seq


# unlike devcsr.to_hs: the values' own dtype, not float32
def to_hs(M):
    return hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols, dtype=M.values.dtype)


def assert_report(got, want, what):
    for f in INT_FIELDS:
        assert getattr(got, f) == want[f], f"{what}: {f} = {getattr(got, f)}, expected {want[f]}"
    for f in MAX_FIELDS:
        assert getattr(got, f) == want[f], f"{what}: {f} = {getattr(got, f)!r}, expected {want[f]!r}"


def test_the_shapes_are_what_they_claim():
    for name, dt in (("total T-1", np.float32), ("total T", np.float64), ("total T+1", np.float32)):
        A, B = case(name, dt)[:2]
        assert A.nnz + B.nnz == {"total T-1": T - 1, "total T": T, "total T+1": T + 1}[name]
    assert [case(n, np.float32)[0].nnz for n in ("nnzA T-1", "nnzA T", "nnzA T+1")] == [T - 1, T, T + 1]
    A, B, rep = case("long row", np.float64)[:3]
    assert (A.nnz, B.nnz, rep["only_a"], rep["only_b"]) == (20000, 20000, 10000, 10000) and rep["rows_len_differ"] == 0
    A, B, rep = case("1000x257", np.float64)[:3]
    assert rep["only_a"] == 400 and rep["only_b"] == 450 and 0 < rep["beyond"] < A.nnz - 400
    assert 0.0 < rep["max_rel_err"] and rep["max_abs_only_a"] > 0 and rep["first_beyond_row"] >= 0
    for M in (A, B):                                        # strictly ascending rows
        rp = M.rowPtr.astype(np.int64)
        inner = np.ones(M.nnz, bool)
        inner[rp[:-1][np.diff(rp) > 0]] = False
        assert np.all(np.diff(M.colInd.astype(np.int64))[inner[1:]] > 0)


# ---- the report ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_report_matches_the_restatement(handle, name, dtype):
    A, B, want, exact, seq = case(name, dtype)
    dA, dB = to_hs(A).toGpuCSR(), to_hs(B).toGpuCSR()
    try:
        got = dA.diff(dB, rel=1e-6, abs=0.0, handle=handle)
        assert_report(got, want, name)
        N = A.nnz + B.nnz
        print(f"{name} {np.dtype(dtype).name}: sum_sq {got.sum_sq!r} fsum {exact!r} float32 loop {seq!r}")
        assert abs(got.sum_sq - exact) <= N * 2.0 ** -52 * exact, f"{name}: sum_sq {got.sum_sq!r} vs fsum {exact!r}"
        if seq is not None:
            assert abs(got.sum_sq - seq) <= N * 2.0 ** -23 * seq, f"{name}: sum_sq {got.sum_sq!r} vs the float32 loop {seq!r}"
        again = dA.diff(dB, rel=1e-6, abs=0.0, handle=handle)
        assert np.float64(again.sum_sq).tobytes() == np.float64(got.sum_sq).tobytes(), "two calls, two sums"
        assert dA.differs(dB, handle) == got.sum_sq
        # the other side as the reference, and the host-resident form (uploaded for the call)
        back, _ = cr.report(B, A, rel=1e-6, abs_tol=0.0)
        assert_report(to_hs(B).diff(to_hs(A), handle=handle), back, name + " swapped, host resident")
        # predicates against the reference's own rules
        assert dA.isEqual(dB, handle) == cr.is_equal(A, B), name
        assert dA.isRelativeEqual(dB, 1e-6, handle) == cr.is_relative_equal(A, B, 1e-6), name
        assert dA.isParityEqual(dB, 1e-6, handle) == (want["rows_len_differ"] + want["only_a"] + want["only_b"] + want["beyond"] == 0)
        # the row lengths
        for pc in ([], REF_PERCENTS, [-0.5, -0.25, 0.0, 0.25, 0.5, 1.0, 2.0, 4.0]):
            counts = dA.differsStats(dB, pc, handle)
            assert counts == cr.differs_stats(A.rowPtr, B.rowPtr, pc, dtype) and sum(counts) == A.rows, (name, pc)
    finally:
        dA.deviceDispose()
        dB.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["5x7 both empty", "total T+1", "1000x257", "long row"])
def test_a_matrix_equals_itself(handle, name, dtype):
    A = to_hs(case(name, dtype)[0])
    dA = A.toGpuCSR()
    try:
        for d in (dA.diff(dA, handle=handle), A.diff(A, handle=handle)):
            assert [getattr(d, f) for f in INT_FIELDS] == [0, -1, 0, 0, -1, 0, -1]
            assert [getattr(d, f) for f in MAX_FIELDS] == [0.0] * 4 and d.sum_sq == 0.0
        assert dA.isEqual(dA, handle) and dA.isParityEqual(dA, handle=handle) and dA.isRelativeEqual(dA, 0.0, handle)
        assert dA.differs(dA, handle) == 0.0
    finally:
        dA.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_nan_in_a_common_column(handle, dtype):
    A, B, want = case("1000x257", dtype)[:3]
    # an entry of A, in a row of the second half, whose column B holds with the same bits: not beyond, no maximum is its
    p = row = -1
    for r in range(A.rows // 2, A.rows):
        b_row = dict(zip(B.colInd[B.rowPtr[r]:B.rowPtr[r + 1]].tolist(), B.values[B.rowPtr[r]:B.rowPtr[r + 1]].tolist()))
        hits = [q for q in range(A.rowPtr[r], A.rowPtr[r + 1]) if b_row.get(int(A.colInd[q])) == A.values[q]]
        if hits:
            p, row = hits[0], r
            break
    assert p >= 0
    v = A.values.copy()
    v[p] = np.nan
    An = Host(A.rowPtr, A.colInd, v, A.rows, A.cols)
    dAn, dB = to_hs(An).toGpuCSR(), to_hs(B).toGpuCSR()
    try:
        d = dAn.diff(dB, rel=1e-6, abs=0.0, handle=handle)
        assert_report(d, cr.report(An, B)[0], "NaN in A")
        assert d.beyond == want["beyond"] + 1
        assert [getattr(d, f) for f in MAX_FIELDS] == [want[f] for f in MAX_FIELDS], "the maxima skip the NaN"
        assert math.isnan(d.sum_sq)
        loose = dAn.diff(dB, rel=1e9, abs=0.0, handle=handle)                 # every finite pair is within rel = 1e9
        assert (loose.beyond, loose.first_beyond_row) == (1, row)
        other = dB.diff(dAn, rel=1e9, abs=0.0, handle=handle)                 # the NaN on the reference side
        assert (other.beyond, other.first_beyond_row) == (1, row) and math.isnan(other.sum_sq)
        assert not dAn.isParityEqual(dAn, handle=handle)                      # a NaN equals nothing, itself included
    finally:
        dAn.deviceDispose()
        dB.deviceDispose()


# ---- predicates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_predicates_flip_where_the_reference_says(handle, dtype):
    A = case("1000x257", dtype)[0]
    p = A.nnz // 3
    base = A.values.copy()
    base[p] = 0.375

    def other(x):
        v = base.copy()
        v[p] = x
        return to_hs(Host(A.rowPtr, A.colInd, v.astype(dtype), A.rows, A.cols)).toGpuCSR()

    dA = other(0.375)
    made = [dA]
    try:
        for x, equal, parity in ((0.375 + 5e-8, True, None), (0.375 + 2e-7, False, None), (0.375 - 2e-7, False, None),
                                 (0.375 * (1 + 1e-8), True, True), (0.375 * (1 + 1e-5), None, False),
                                 (0.375 * (1 - 1e-5), None, False)):
            dB = other(x)
            made.append(dB)
            if equal is not None:
                assert dB.isEqual(dA, handle) == equal and dA.isEqual(dB, handle) == equal, x
            if parity is not None:
                assert dB.isParityEqual(dA, 1e-6, handle) == parity, x
                assert dB.isRelativeEqual(dA, 1e-6, handle) == parity, x
    finally:
        for d in made:
            d.deviceDispose()


# ---- differsStats ----------------------------------------------------------------------------------------------------
def every_slot_lengths(percents, m, seed):
    """row-length pairs (a, b) that hit every one of the n + 4 slots, thresholds being multiples of 1/16 above -1: slot 0
    by a row that empties (ratio -1), slot k by a ratio EQUAL to percents[k - 1] (the compare is strict: the row goes to
    the next slot), slot n by a ratio equal to the last threshold; then the three special slots; then random pairs"""
    pairs = [(16, 0)]
    for p in percents:
        b = 16 + int(round(16 * p))
        pairs.append((16, b) if b != 16 else (32, 33))      # ratio 0 would be "equal lengths": 1/32 sits in the same slot
    pairs += [(0, 3), (0, 0), (5, 5)]
    rng = np.random.default_rng(seed)
    rest = m - len(pairs)
    pairs += list(zip(rng.integers(0, 9, size=rest).tolist(), rng.integers(0, 9, size=rest).tolist()))
    order = rng.permutation(m)
    a, b = np.array(pairs, np.int64)[order].T
    return a, b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [255, 256, 257])
@pytest.mark.parametrize("npercents", [0, 8, 64])
def test_differs_stats_hits_every_slot(handle, npercents, m, dtype):
    step = {0: 1, 8: 4, 64: 16}[npercents]
    percents = [-1.0 + (k + 1) / step for k in range(npercents)]             # 8: -0.75 .. 1.0, 64: -0.9375 .. 3.0
    if npercents == 8:
        percents[3] = 0.03125                               # a threshold no ratio equals exactly next to one that does
    a, b = every_slot_lengths(percents, m, 100 * npercents + m)
    rpa, rpb = np.zeros(m + 1, np.int32), np.zeros(m + 1, np.int32)
    np.cumsum(a, out=rpa[1:])
    np.cumsum(b, out=rpb[1:])
    want = cr.differs_stats(rpa, rpb, percents, dtype)
    assert min(want) >= 1 and sum(want) == m, want
    da, db = hs.h2d(rpa), hs.h2d(rpb)
    try:
        assert hs.csr_differs_stats_raw(handle, m, da, db, percents, dtype=dtype) == want
        assert hs.csr_differs_stats_raw(handle, 0, da, db, percents, dtype=dtype) == [0] * (npercents + 4)
    finally:
        hs.dev_free(da)
        hs.dev_free(db)


# ---- bad input -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_input_is_an_error_not_a_fault(handle, dtype):
    L = hs.lib()
    fn = L.hip_csr_diff_f64 if np.dtype(dtype) == np.float64 else L.hip_csr_diff
    A, B, want = case("1000x257", dtype)[:3]
    dB = to_hs(B).toGpuCSR()
    dA = to_hs(A).toGpuCSR()
    rp = A.rowPtr.astype(np.int64)
    r = int(np.nonzero(np.diff(rp) >= 3)[0][5])             # a row with at least three entries
    s = int(rp[r])

    def changed(arr, idx, vals):
        arr = arr.copy()
        arr[idx] = vals
        return arr

    swapped = changed(A.colInd, [s, s + 1], [A.colInd[s + 1], A.colInd[s]])
    repeated = changed(A.colInd, [s + 1], [A.colInd[s]])
    dips = changed(A.rowPtr, [r + 1], [A.rowPtr[r] - 1 if s > 0 else A.rowPtr[r + 2] + 1])
    short = changed(A.rowPtr, [A.rows], [A.nnz - 1])

    def call(I, J, as_b=False):
        out = hs.CsrDiff()
        out.beyond = 77
        mine = [C.c_void_p(I), C.c_void_p(J), C.c_void_p(dA.values), A.nnz]
        theirs = [C.c_void_p(dB.rowPtr), C.c_void_p(dB.colInd), C.c_void_p(dB.values), B.nnz]
        args = theirs + mine if as_b else mine + theirs
        rc = fn(handle.ptr, A.rows, A.cols, *args, 1e-6, 0.0, C.byref(out))
        return rc, out, L.spgemm_hip_last_error()

    try:
        for I, J, word in ((A.rowPtr, swapped, b"ascending"), (A.rowPtr, repeated, b"ascending"),
                           (dips, A.colInd, b"rowPtr"), (short, A.colInd, b"rowPtr")):
            for as_b in (False, True):
                dI, dJ = hs.h2d(I), hs.h2d(J)
                try:
                    rc, out, msg = call(dI, dJ, as_b)
                finally:
                    hs.dev_free(dI)
                    hs.dev_free(dJ)
                assert rc == ERR_INPUT and word in msg, (rc, msg)
                assert all(getattr(out, f) == 0 for f, _ in hs.CsrDiff._fields_), "the report is left zeroed"
                # the handle is still good
                assert_report(dA.diff(dB, rel=1e-6, abs=0.0, handle=handle), want, "valid pair after the error")
        with pytest.raises(hs.SpgemmError):
            to_hs(Host(A.rowPtr, swapped, A.values, A.rows, A.cols)).diff(to_hs(B), handle=handle)
    finally:
        dA.deviceDispose()
        dB.deviceDispose()


def test_pool_does_not_grow(handle):
    A, B = case("1000x257", np.float64)[:2]
    dA, dB = to_hs(A).toGpuCSR(), to_hs(B).toGpuCSR()

    def rounds(k):
        for _ in range(k):
            dA.diff(dB, handle=handle)
            dA.differsStats(dB, REF_PERCENTS, handle)
    try:
        rounds(20)
        before = hs.pool_cached_bytes(handle.device)
        rounds(5)
        assert hs.pool_cached_bytes(handle.device) == before
    finally:
        dA.deviceDispose()
        dB.deviceDispose()


# ---- through the product path ----------------------------------------------------------------------------------------
def test_two_routes_to_a_product_agree_on_the_device(handle):
    """hip_gpuSpMM on one handle, symbolic + numeric on another, both row-sorted on the device, compared without a
    download; CSR::differs between them stays under what 1e-6 relative per entry allows"""
    A = synth_csr(8192, 5, 2)
    hA = hs.CSR.from_arrays(A.rowPtr, A.colInd, A.values, A.rows, A.cols)
    dA = hA.toGpuCSR()
    second = hs.Handle(0)
    IC = JC = VC = 0
    one = None
    try:
        one = hs.gpuSpMMWrapper(dA, dA, handle)
        IC = hs.dev_alloc(4 * (A.rows + 1))
        nnz = hs.spgemm_symbolic_raw(second, dA.rowPtr, dA.colInd, A.nnz, dA.rowPtr, dA.colInd, A.nnz, A.rows, A.cols, A.cols, IC)
        assert nnz == one.nnz
        JC, VC = hs.dev_alloc(4 * nnz), hs.dev_alloc(4 * nnz)
        hs.spgemm_numeric_raw(second, dA.rowPtr, dA.colInd, dA.values, A.nnz, dA.rowPtr, dA.colInd, dA.values, A.nnz,
                              A.rows, A.cols, A.cols, IC, JC, VC)
        two = hs.CSR(VC, JC, IC, A.rows, A.cols, nnz, True, dtype=np.float32)
        hs.sort_rows_device(one, handle)
        hs.sort_rows_device(two, second)
        assert one.isParityEqual(two, 1e-6, handle)
        d = one.diff(two, rel=1e-6, abs=0.0, handle=handle)
        assert (d.rows_len_differ, d.only_a, d.only_b, d.beyond) == (0, 0, 0, 0) and d.max_rel_err <= 1e-6
        values = hs.d2h(VC, nnz, np.float32).astype(np.float64)
        bound = math.fsum((1e-6 * values) ** 2)             # every |a - b| <= 1e-6 |b|
        moved = one.differs(two, handle)
        print(f"differs between the two routes: {moved!r} (bound {bound!r}), max_rel_err {d.max_rel_err!r}")
        assert 0.0 <= moved <= bound
        assert one.differsStats(two, REF_PERCENTS, handle)[len(REF_PERCENTS) + 1] == 0
    finally:
        if one is not None:
            one.deviceDispose()
        for p in (IC, JC, VC):
            hs.dev_free(p)
        dA.deviceDispose()
        second.close()


def test_cpp_mirror_runs_the_end_of_run_check_on_the_device():
    """tests/cpp/compare_check.cc: RMCL(..., GPU), the result and its deepCopy sorted and compared on the device (Same),
    then one value changed by 1e-3 (Diffs, naming the row)"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-B", "-C", cpp, "compare_check.x"])
    for name in ("own_graph.snap", "t2.snap"):
        out = subprocess.run([os.path.join(cpp, "compare_check.x"), os.path.join(DATA, name), "3"], capture_output=True,
                             text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.splitlines()
        assert lines.index("Same") < lines.index("Diffs") and lines.count("Same") == 1 and lines.count("Diffs") == 1
        row = [ln for ln in lines if ln.startswith("changed row ")][0].split()[-1]
        assert any(ln.startswith(f"row {row}: values differ") for ln in lines), out.stdout
