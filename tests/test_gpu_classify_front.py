"""GPU (-m gpu): the front end of every product -- per-row products and records (K1), the slot scan (K2), the row scatter
(K3) -- and the scan between the passes, compared EXACTLY with the numpy restatement in tests/classify_ref.py, at the
edges of their waves, blocks, chunks and tiles.

The classification reads A and B.rowPtr only, so most cases fabricate a B.rowPtr (row lengths chosen at will, no columns);
the records (one per entry of A, read by every later kernel) and the scan of C's row lengths are checked through plain
products against the CPU oracle, or against a product known in closed form (I * A = A)."""
import ctypes as C

import numpy as np
import pytest

import classify_ref as cr
from devcsr import built_gpu, handle  # noqa: F401
from devcsr import to_hs
from helpers import assert_parity, po
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu


# ---- inputs --------------------------------------------------------------------------------------------------------------
def row_ptr(lens):
    rp = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    assert rp[-1] < 2**31
    return rp.astype(np.int32)


def random_a(m, k, seed, empty=(), max_len=12):
    """m x k, 0..max_len entries per row (sorted distinct columns), the rows in `empty` (those that exist) without any"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, min(max_len, k) + 1, size=m)
    for r in empty:
        if -m <= r < m:
            lens[r] = 0
    IA = row_ptr(lens)
    JA = np.concatenate([np.sort(rng.choice(k, size=n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return IA, JA


def real_b(IB, n, seed):
    """a B with the given row pointer: sorted distinct columns below n, small integer values (exact float sums)"""
    rng = np.random.default_rng(seed)
    lens = np.diff(IB)
    JB = np.concatenate([np.sort(rng.choice(n, size=x, replace=False)) for x in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return JB, rng.integers(1, 4, size=len(JB)).astype(np.float32)


# ---- device calls --------------------------------------------------------------------------------------------------------
def classify(h, dIA, dJA, dIB, m, k):
    """hip_gpuFlopsClassify on raw device pointers -> (hv, hv_len, rowIds, dflops, total)"""
    ids, fl, hv = C.c_void_p(), C.c_void_p(), (C.c_int * hs.HV_LEN)()
    hvl, tot = C.c_int(0), C.c_longlong(0)
    rc = hs.lib().hip_gpuFlopsClassify(h.ptr, C.c_void_p(dIA), C.c_void_p(dJA), C.c_void_p(dIB), m, k, C.byref(ids),
                                       C.byref(fl), hv, C.byref(hvl), C.byref(tot))
    assert rc == 0, hs.lib().spgemm_hip_last_error()
    out = ([int(x) for x in hv], hvl.value, hs.d2h(ids.value, m, np.int32), hs.d2h(fl.value, m + 1, np.int32), tot.value)
    hs.dev_free(ids.value)
    hs.dev_free(fl.value)
    return out


def check_front(h, IA, JA, IB, what, dIB=None):
    """classification API and hip_csr_row_flops of (A, B.rowPtr) against the restatement, exactly; returns the products"""
    m, k = len(IA) - 1, len(IB) - 1
    flops = cr.row_products(IA, JA, IB)
    order = cr.row_order(flops)
    dIA, dJA = hs.h2d(IA), hs.h2d(JA)
    own = dIB is None
    if own:
        dIB = hs.h2d(IB)
    try:
        hv, hv_len, rowIds, dflops, tot = classify(h, dIA, dJA, dIB, m, k)
        want_hv, want_len = cr.hv_of(flops)
        assert tot == int(flops.sum()), what
        assert hv[:9] == want_hv and hv_len == want_len, (what, hv, want_hv)
        assert np.array_equal(rowIds, order), (what, "row ids: slot order, ascending inside a slot")
        assert np.array_equal(dflops, cr.dflops_of(flops, order)), (what, "dflops")
        out = hs.dev_alloc(4 * max(m, 1))
        assert hs.row_flops_raw(h, dIA, dJA, dIB, m, out) == int(flops.sum()), what
        assert np.array_equal(hs.d2h(out, m, np.int32), flops.astype(np.int32)), (what, "row flops")
        hs.dev_free(out)
    finally:
        for p in (dIA, dJA) + ((dIB,) if own else ()):
            hs.dev_free(p)
    return flops


def check_product(h, IA, JA, IB, n, what, binned=False):
    """A * B with a real B of that row pointer (the records, every symbolic and numeric kernel behind them, the scan) against
    the CPU oracle; binned: through the classification API and hip_sgpuSpMM, whose records come from k_entry_lens"""
    m, k = len(IA) - 1, len(IB) - 1
    rng = np.random.default_rng(len(JA))
    JB, VB = real_b(IB, n, 5)
    A = po.CSRHost(IA, JA, rng.integers(1, 4, size=len(JA)).astype(np.float32), m, k)
    B = po.CSRHost(IB, JB, VB, k, n)
    dA, dB = to_hs(A).toGpuCSR(), to_hs(B).toGpuCSR()
    if binned:
        hv, _, ids, fl, _ = hs.gpuFlopsClassify(dA, dB, h)
        dC = hs.sgpuSpMMWrapper(dA, dB, ids, hv, fl, h)
        hs.dev_free(ids)
        hs.dev_free(fl)
    else:
        dC = hs.gpuSpMMWrapper(dA, dB, h)
    got = dC.toCpuCSR()
    for d in (dC, dA, dB):
        d.deviceDispose()
    assert_parity(got, po.omp_spmm(A, B), what=what)


# ---- K1: rows at the edges of a wave (64 rows) and of a block (256 rows) --------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_rows_at_wave_and_block_edges(handle, m):
    """the first and last row of a wave's 64-row range empty (rows 0, 63, 64, 127, ..., and the last row), and not"""
    k = 97
    IB = row_ptr(np.random.default_rng(1).integers(0, 9, size=k))
    edges = [r for w in range(0, m, 64) for r in (w, w + 63)] + [-1]
    for empty, tag in ((edges, "empty"), ((), "full")):
        IA, JA = random_a(m, k, 10 + m, empty=empty)
        check_front(handle, IA, JA, IB, f"m={m} edges {tag}")
        check_product(handle, IA, JA, IB, 211, f"m={m} edges {tag}: product")


# ---- K1: ranges of entries longer than the chunks a wave keeps in flight (4 x 64) ------------------------------------------
@pytest.mark.parametrize("long_len", [257, 1025])
def test_one_long_row_between_empty_neighbours(handle, long_len):
    """one wave's range of entries ends inside a chunk; its other rows are empty"""
    k = 2000
    IB = row_ptr(np.random.default_rng(2).integers(0, 5, size=k))
    for m, row in ((1, 0), (70, 0), (70, 63), (70, 64), (300, 131)):
        lens = np.zeros(m, np.int64)
        lens[row] = long_len
        JA = np.sort(np.random.default_rng(row).choice(k, size=long_len, replace=False)).astype(np.int32)
        flops = check_front(handle, row_ptr(lens), JA, IB, f"row {row} of {m} holds {long_len} entries")
        assert np.count_nonzero(flops) == 1
        check_product(handle, row_ptr(lens), JA, IB, 300, f"row {row} of {m} holds {long_len} entries: product")


@pytest.mark.parametrize("nnz", [64, 256, 512, 320])
def test_last_entry_is_the_last_lane_of_a_chunk(handle, nnz):
    """nnz(A) a multiple of 64: the last entry sits in lane 63; of 256: it closes a full set of chunks"""
    k, m = 50, 64
    IB = row_ptr(np.random.default_rng(3).integers(0, 7, size=k))
    lens = np.full(m, nnz // m, np.int64)
    JA = np.concatenate([np.sort(np.random.default_rng(r).choice(k, size=nnz // m, replace=False)) for r in range(m)]).astype(np.int32)
    assert len(JA) == nnz
    check_front(handle, row_ptr(lens), JA, IB, f"nnz={nnz}")
    check_product(handle, row_ptr(lens), JA, IB, 64, f"nnz={nnz}: product")


# ---- K1: {IB[j], IB[j + 1]} as one load -----------------------------------------------------------------------------------
def _pair_case(k):
    rng = np.random.default_rng(k)
    blen = rng.integers(0, 6, size=k)
    blen[[1, 2, k - 2]] = 0                                   # empty B rows, next to the first and the last
    blen[[0, k - 1]] = 3
    IB = row_ptr(blen)
    rows = [[0], [k - 1], [0, k - 1], [1], [2], [k - 2], list(range(0, k, 2)), list(range(1, k, 2)), list(range(k))]
    rows += [sorted(rng.choice(k, size=5, replace=False).tolist()) for _ in range(70)]
    IA = row_ptr([len(r) for r in rows])
    JA = np.concatenate(rows).astype(np.int32)
    return IA, JA, IB


@pytest.mark.parametrize("k", [64, 65])
def test_pair_gather_first_last_odd_even_columns_and_empty_b_rows(handle, k):
    IA, JA, IB = _pair_case(k)
    check_front(handle, IA, JA, IB, f"pair gather k={k}")
    check_product(handle, IA, JA, IB, 40, f"pair gather k={k}: product")
    check_product(handle, IA, JA, IB, 40, f"pair gather k={k}: binned product (k_entry_lens)", binned=True)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_b_row_pointer_that_is_only_4_byte_aligned(handle, shift):
    """B.rowPtr as a view at an offset of 1, 2, 3 ints into a larger device buffer: {IB[j], IB[j+1]} is gathered with one
    8-byte load (the compiler merges the two reads), from an address that is a multiple of 4 and not of 8 for odd or for
    even j"""
    k = 65
    IA, JA, IB = _pair_case(k)
    buf = hs.h2d(np.concatenate([np.full(shift, -12345, np.int32), IB, np.full(4, -12345, np.int32)]))
    assert buf % 8 == 0
    try:
        check_front(handle, IA, JA, IB, f"rowPtr view at +{shift}", dIB=buf + 4 * shift)
        # the product too, on raw pointers: records from K1, then the classification API's from k_entry_lens
        JB, VB = real_b(IB, 40, 5)
        VA = np.ones(len(JA), np.float32)
        m = len(IA) - 1
        d = [hs.h2d(x) for x in (IA, JA, VA, JB, VB)]
        ic, jc, cv, nnz = hs.gpu_spmm_raw(handle, d[0], d[1], d[2], len(JA), buf + 4 * shift, d[3], d[4], len(JB), m, k, 40)
        got = hs.CSR(hs.d2h(cv, nnz, np.float32), hs.d2h(jc, nnz, np.int32), hs.d2h(ic, m + 1, np.int32), m, 40, nnz)
        for p in d + [ic, jc, cv]:
            hs.dev_free(p)
        assert_parity(got, po.omp_spmm(po.CSRHost(IA, JA, VA, m, k), po.CSRHost(IB, JB, VB, k, 40)), what=f"view at +{shift}")
    finally:
        hs.dev_free(buf)


# ---- K2 / K3: every layout slot, order inside the slots -------------------------------------------------------------------
SLOT_LENS = [0, 1, 2, 4, 5, 16, 17, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096,
             4097, 8192, 16384, 40000, 65536, 131072, 131073, 300000]


def test_all_layout_slots_at_once(handle):
    """rows of 0, 1, 2-4, ..., 2049-4096 products and of each of the six size classes above: one A entry that points at a B
    row of that length.  Several rows per slot, scattered over three blocks."""
    IB = row_ptr(SLOT_LENS)
    k = len(SLOT_LENS)
    rng = np.random.default_rng(4)
    JA = np.concatenate([rng.permutation(k) for _ in range(25)]).astype(np.int32)     # 650 rows
    IA = np.arange(len(JA) + 1, dtype=np.int32)
    flops = check_front(handle, IA, JA, IB, "all slots")
    assert np.all(cr.slot_counts(flops) > 0)
    # ... and once with a single row in each of the classes above 4096 products
    one = np.concatenate([rng.permutation(k), rng.integers(0, 18, size=300)]).astype(np.int32)
    flops = check_front(handle, np.arange(len(one) + 1, dtype=np.int32), one, IB, "all slots, one big row per class")
    assert np.all(cr.slot_counts(flops)[10:] >= 1) and cr.slot_counts(flops)[11] == 1


def test_all_layout_slots_product(handle):
    """the same row lengths through a real product (n >= 131 073 for the longest rows), one row per length"""
    lens = [x for x in SLOT_LENS if x <= 131073]
    IB = row_ptr(lens)
    JA = np.arange(len(lens), dtype=np.int32)
    check_product(handle, np.arange(len(lens) + 1, dtype=np.int32), JA, IB, 131100, "one row per slot: product")


# ---- K2: blocks of K1 (256 rows each) at the edges of the scan's rounds ----------------------------------------------------
@pytest.mark.parametrize("nblk", [1, 1023, 1024, 1025, 4096, 4097])
def test_slot_scan_at_its_loop_edges(handle, nblk):
    """one entry per row; the last block holds 3 rows.  Once with rows of every slot up to 4096 products and a few above,
    once with every row in ONE slot (all other slots empty)."""
    m = (nblk - 1) * 256 + 3
    rng = np.random.default_rng(nblk)
    IB = row_ptr(SLOT_LENS)
    IA = np.arange(m + 1, dtype=np.int32)
    JA = rng.integers(0, 18, size=m).astype(np.int32)
    JA[rng.integers(0, m, size=min(m, 8))] = rng.integers(18, len(SLOT_LENS), size=min(m, 8))
    check_front(handle, IA, JA, IB, f"nblk={nblk} mixed")
    flops = check_front(handle, IA, np.full(m, 2, np.int32), IB, f"nblk={nblk} one slot")
    assert np.count_nonzero(cr.slot_counts(flops)) == 1


# ---- the scan between the passes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 1, 4095, 4096, 4097, 3 * 4096 + 5, 1025 * 4096 + 1, 4097 * 4096 + 1])
def test_scan_of_row_lengths_closed_form(handle, m):
    """C = I * A has A's rows: rowPtr(C) == rowPtr(A), to the last entry.  Tiles of 4096 rows: one, two, several, more
    than the 1024 a block adds up in one round, and more than the blocks add up themselves (a third launch scans them)."""
    rng = np.random.default_rng(m % 1000)
    lens = rng.integers(0, 3, size=m) if m > 2 else np.ones(m, np.int64)
    if m > 2:
        lens[[0, -1]] = 2                                    # the first and the last row count
    IA = row_ptr(lens)
    nnz = int(IA[-1])
    # any columns, distinct inside a row (7919 is prime and no m here is a multiple): rows of I * A are A's
    JA = (np.arange(nnz, dtype=np.int64) * 7919 % max(m, 1)).astype(np.int32)
    eye = hs.CSR.from_arrays(np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32), np.ones(m, np.float32), m, m)
    A = hs.CSR.from_arrays(IA, JA, np.ones(nnz, np.float32), m, m)
    dI, dA = eye.toGpuCSR(), A.toGpuCSR()
    dC = hs.gpuSpMMWrapper(dI, dA, handle)
    assert dC.nnz == nnz and handle.stats()["nnzC"] == nnz
    got = dC.toCpuCSR()
    for d in (dC, dI, dA):
        d.deviceDispose()
    assert np.array_equal(got.rowPtr, IA)
    assert np.array_equal(got.values, A.values)
    assert int(got.colInd.sum(dtype=np.int64)) == int(JA.sum(dtype=np.int64))
    if m <= 3 * 4096 + 5:
        assert np.array_equal(_canon(got.rowPtr, got.colInd, got.values)[0], _canon(IA, JA, A.values)[0])
        # the classification API's scan (wrapping form) over the same rows: products == A's row lengths
        check_front(handle, np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32), IA, f"scan m={m}")


# ---- K1 on extents: B left unpacked by the previous R-MCL iteration ---------------------------------------------------------
def _canon(rp, ci, v):
    key = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp)) * (1 << 32) + ci
    o = np.argsort(key, kind="stable")
    return ci[o], v[o]


def test_two_device_iterations_equal_two_packed_steps(handle):
    """hip_gpuRmclIter_device classifies its second iteration from {start, end} pairs per row of the unpacked Mt
    (k_row_flops<true>); two hip_rmcl_expand_prune steps classify both from packed row pointers.  Same kernels behind,
    same matrices: row pointers, columns and value bits.  (A graph of degree <= 4: every row stays with the one-wave
    kernels, whose sums do not depend on timing.)"""
    m = 2000
    rng = np.random.default_rng(12)
    src = np.repeat(np.arange(m, dtype=np.int32), 3)
    dst = ((src + rng.integers(1, 40, size=len(src))) % m).astype(np.int32)
    M0 = po.rmcl_init(m, m, dst, src, np.ones(len(src), np.float32))
    dM = to_hs(M0).toGpuCSR()
    d2 = hs.gpuRmclIter_device(2, dM, dM, handle)
    loop = d2.toCpuCSR()
    d2.deviceDispose()
    cur = dM
    for _ in range(2):
        i_, j_, c_, n_ = hs.rmcl_expand_prune_raw(handle, dM.rowPtr, dM.colInd, dM.values, dM.nnz, cur.rowPtr, cur.colInd,
                                                  cur.values, cur.nnz, m, m, m)
        if cur is not dM:
            cur.deviceDispose()
        cur = hs.CSR(c_, j_, i_, m, m, n_, on_device=True)
    steps = cur.toCpuCSR()
    cur.deviceDispose()
    dM.deviceDispose()
    assert loop.nnz == steps.nnz > m
    assert np.array_equal(loop.rowPtr, steps.rowPtr)
    (lc, lv), (sc, sv) = _canon(loop.rowPtr, loop.colInd, loop.values), _canon(steps.rowPtr, steps.colInd, steps.values)
    assert np.array_equal(lc, sc)
    assert lv.tobytes() == sv.tobytes()
