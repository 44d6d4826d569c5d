"""GPU (-m gpu): the column-partitioned CSR -- hip_csr_split_columns, hip_pcsr_join, hip_pcsr_spmm and their _f64 twins --
against the numpy restatement tests/pcsr_ref.py (pinned by hand in tests/test_pcsr_abi.py).  Split and join move entries
and do no arithmetic, so they are compared on bits, in-row order included; float64 values carry bits beyond float32
(x + 2^-40), so a pass through float would show.  The product tests use values from {1, 2, 3}: every product and every
row sum is then exact in float and in double whatever the order of summation, so the blockwise product must equal the
whole product at tolerance 0.  The last tests run the reference's experiment (correctTests/pcsrTest.cc) through the C++
mirror and through the Python PCSR class."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcsr_ref as pr
import reorder_ref as rr
from devcsr import built_gpu, handle  # noqa: F401
from devcsr import assert_bits, one_long_row, take, typed, typed_plain, with_nnz
from helpers import DATA, ROOT, po, random_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
ERR_INPUT = 5
CP_TILE = 1024          # entries per block of the split key / join copy kernels (csr_common_device.hpp, pcsr_device.hpp)
RS_TILE = 2048          # keys per block of the radix kernels (csr_common_device.hpp)
BLOCK_COUNTS = [1, 2, 3, 7, 64]


# ---- inputs (made once, never modified) ------------------------------------------------------------------------------
# this format's own edge: the block boundaries b * stride_of(n, c) (bcsr: b * c; mcsr: the corner's last column)
def boundary_columns(rows, n, c):
    """every row holds exactly the columns b * stride - 1 and b * stride for each b: the last column of a block and the
    first of the next, in descending order"""
    stride = pr.stride_of(n, c)
    cols = np.array([x for b in range(1, c) for x in (b * stride - 1, b * stride) if x < n][::-1], np.int32)
    rp = np.arange(rows + 1, dtype=np.int32) * len(cols)
    v = (np.arange(rows * len(cols)) % 97 + 1).astype(np.float32)
    return rr.Host(rp, np.tile(cols, rows), v, rows, n)


# per format: the second member is this format's parameter list (block counts; bcsr: tile shapes)
def _cases():
    """name -> (matrix, block counts)"""
    out = {"0x0": (rr.Host(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 0, 0), BLOCK_COUNTS),
           "5x7 empty": (rr.Host(np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 5, 7), BLOCK_COUNTS),
           "1000x257": (random_csr(1000, 257, 0.02, 1, sorted_rows=False), BLOCK_COUNTS),
           "257x1000": (random_csr(257, 1000, 0.02, 2, sorted_rows=False), BLOCK_COUNTS),
           "long row": (one_long_row(), BLOCK_COUNTS)}
    for nnz in (CP_TILE - 1, CP_TILE, CP_TILE + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1):
        out[f"nnz {nnz}"] = (with_nnz(61, 97, nnz, nnz), BLOCK_COUNTS)
    out["n=5 c=7: stride 1, two empty blocks"] = (random_csr(40, 5, 0.5, 3, sorted_rows=False), [7])
    out["n=256 c=4: n == c * stride"] = (random_csr(100, 256, 0.05, 4, sorted_rows=False), [4])
    out["boundary columns"] = (boundary_columns(50, 100, 7), [7])
    return out


CASES = _cases()


# per format: what is downloaded and the restatement's type differ (here pcsr_ref.Split)
def downloaded(p):
    """the packed arrays of a split hs.PCSR as a pcsr_ref.Split"""
    ip, jp, vp = p._base
    n = p.nnz()
    return pr.Split(hs.d2h(ip, p.c * (p.rows + 1), np.int32), hs.d2h(jp, n, np.int32), hs.d2h(vp, n, p.dtype), p.blockPtr,
                    p.rows, p.cols, p.c)


def assert_split_bits(got, want, what):
    assert (got.rows, got.cols, got.c, got.stride) == (want.rows, want.cols, want.c, want.stride), what
    assert np.array_equal(got.blockPtr, want.blockPtr), f"{what}: blockPtr"
    assert np.array_equal(got.rowPtrs, want.rowPtrs), f"{what}: rowPtrs"
    assert np.array_equal(got.colInd, want.colInd), f"{what}: local columns"
    assert got.values.dtype == want.values.dtype and got.values.tobytes() == want.values.tobytes(), f"{what}: value bits"


# ---- split and join --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_split_and_join_match_the_restatement(handle, name, dtype):
    M0, counts = CASES[name]
    M = typed(M0, dtype)
    S = typed(rr.sort_rows(M0), dtype)
    dM, dS = M.toGpuCSR(), S.toGpuCSR()
    try:
        for c in counts:
            p = hs.PCSR(dM, c, handle)
            try:
                assert (p.rows, p.cols, p.c, p.stride) == (M.rows, M.cols, c, pr.stride_of(M.cols, c))
                assert_split_bits(downloaded(p), pr.split(M, c), f"{name} c={c}: split")
                assert_bits(take(p.join(handle)), pr.stable_partition(M, c), f"{name} c={c}: join(split)")
            finally:
                p.deviceDispose()
            p = hs.PCSR.from_csr(dS, c, handle)
            try:
                assert_bits(take(p.join(handle)), S, f"{name} c={c}: join(split) of a row-sorted matrix is the matrix")
            finally:
                p.deviceDispose()
    finally:
        dM.deviceDispose()
        dS.deviceDispose()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,c", [("1000x257", 3), ("long row", 7), (f"nnz {CP_TILE + 1}", 64), ("5x7 empty", 2)])
def test_join_of_separate_allocations_equals_join_of_the_packed_views(handle, name, c, dtype):
    M = typed(CASES[name][0], dtype)
    dM = M.toGpuCSR()
    p = hs.PCSR(dM, c, handle)
    apart = [typed_plain(B, dtype).toGpuCSR() for B in pr.split(M, c).blocks()]     # every block its own three arrays
    try:
        packed = take(p.join(handle))
        q = hs.PCSR._of_blocks(apart, M.rows, M.cols, dtype)
        assert_bits(take(q.join(handle)), packed, f"{name} c={c}")
        assert_bits(packed, pr.stable_partition(M, c), f"{name} c={c}")
    finally:
        for d in apart + [dM]:
            d.deviceDispose()
        p.deviceDispose()


# ---- bad input -------------------------------------------------------------------------------------------------------
def test_bad_input_is_an_error_not_a_fault(handle):
    L = hs.lib()
    M = typed(CASES["1000x257"][0], np.float32)
    dM = M.toGpuCSR()
    m, n, c = M.rows, M.cols, 3
    stride = pr.stride_of(n, c)

    def split_rc(JA, nnz):
        o = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        bp = (C.c_int * (c + 1))()
        rc = L.hip_csr_split_columns(handle.ptr, m, n, nnz, C.c_void_p(dM.rowPtr), C.c_void_p(JA), C.c_void_p(dM.values), c,
                                     *[C.byref(x) for x in o], bp)
        return rc, [x.value for x in o], L.spgemm_hip_last_error()

    def join_rc(blocks, cols):
        o = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        nnz = C.c_int(9)
        rc = L.hip_pcsr_join(handle.ptr, m, cols, len(blocks), *hs._block_table(blocks), *[C.byref(x) for x in o], C.byref(nnz))
        return rc, [x.value for x in o], L.spgemm_hip_last_error()

    def valid_call(what):
        p = hs.PCSR(dM, c, handle)
        try:
            assert_split_bits(downloaded(p), pr.split(M, c), what)
            assert_bits(take(p.join(handle)), pr.stable_partition(M, c), what)
        finally:
            p.deviceDispose()

    good = pr.split(M, c)
    ups = []
    try:
        # split: a column equal to n
        bad_cols = M.colInd.copy()
        bad_cols[7] = n
        ups.append(hs.h2d(bad_cols))
        rc, outs, msg = split_rc(ups[-1], M.nnz)
        assert rc == ERR_INPUT and outs == [None, None, None] and b"column" in msg, (rc, outs, msg)
        valid_call("valid call after a column equal to n")
        # split: rowPtr[m] != nnz
        rc, outs, msg = split_rc(dM.colInd, M.nnz - 1)
        assert rc == ERR_INPUT and outs == [None, None, None] and b"rowPtr" in msg, (rc, outs, msg)
        valid_call("valid call after rowPtr[m] != nnz")

        def uploaded(blocks):
            table = []
            for B in blocks:
                ptrs = [hs.h2d(np.asarray(B.rowPtr, np.int32)), hs.h2d(np.asarray(B.colInd, np.int32)),
                        hs.h2d(np.asarray(B.values, np.float32))]
                ups.extend(ptrs)
                table.append((*ptrs, B.nnz))
            return table
        # join: a local column equal to stride (block 0)
        blocks = good.blocks()
        wrong = blocks[0].colInd.copy()
        wrong[5] = stride
        blocks[0] = rr.Host(blocks[0].rowPtr, wrong, blocks[0].values, m, stride)
        rc, outs, msg = join_rc(uploaded(blocks), n)
        assert rc == ERR_INPUT and outs == [None, None, None] and b"column" in msg, (rc, outs, msg)
        valid_call("valid call after a local column equal to stride")
        # join: a column of the last block inside [0, stride) whose global column is n or more
        assert (c - 1) * stride + stride - 1 >= n
        blocks = good.blocks()
        wrong = blocks[-1].colInd.copy()
        wrong[0] = stride - 1
        blocks[-1] = rr.Host(blocks[-1].rowPtr, wrong, blocks[-1].values, m, stride)
        rc, outs, msg = join_rc(uploaded(blocks), n)
        assert rc == ERR_INPUT and outs == [None, None, None] and b"column" in msg, (rc, outs, msg)
        # the same blocks are a valid partition of a matrix one column wider ... that keeps the stride
        assert pr.stride_of(n + 1, c) == stride
        rc, outs, msg = join_rc(uploaded(blocks), n + 1)
        assert rc == 0 and all(outs), (rc, outs, msg)
        for ptr in outs:
            hs.dev_free(ptr)
        # join: a block's rowPtr that does not end at its count
        table = uploaded(good.blocks())
        table[1] = (*table[1][:3], table[1][3] - 1)
        rc, outs, msg = join_rc(table, n)
        assert rc == ERR_INPUT and outs == [None, None, None] and b"rowPtr" in msg, (rc, outs, msg)
        valid_call("valid call after the join errors")
    finally:
        for ptr in ups:
            hs.dev_free(ptr)
        dM.deviceDispose()


def test_pool_does_not_grow(handle):
    M = typed(CASES["1000x257"][0], np.float64)
    dM = M.toGpuCSR()

    def rounds(k):
        for _ in range(k):
            p = hs.PCSR(dM, 7, handle)
            p.join(handle).deviceDispose()
            p.deviceDispose()
    try:
        rounds(20)
        before = hs.pool_cached_bytes(handle.device)
        rounds(5)
        assert hs.pool_cached_bytes(handle.device) == before
    finally:
        dM.deviceDispose()


# ---- the blockwise product -------------------------------------------------------------------------------------------
def small_ints(M, seed):
    """M with values drawn from {1, 2, 3}"""
    v = np.random.default_rng(seed).integers(1, 4, size=M.nnz).astype(np.float32)
    return po.CSRHost(M.rowPtr, M.colInd, v, M.rows, M.cols)


def _empty_middle_block(B, c):
    """B without the entries of block 1"""
    stride = pr.stride_of(B.cols, c)
    keep = (B.colInd // stride) != 1
    row_of = np.repeat(np.arange(B.rows), np.diff(B.rowPtr))
    rp = np.zeros(B.rows + 1, np.int32)
    np.cumsum(np.bincount(row_of[keep], minlength=B.rows), out=rp[1:])
    return po.CSRHost(rp, B.colInd[keep], B.values[keep], B.rows, B.cols)


@pytest.fixture(scope="module")
def products():
    """name -> (A, B, the oracle's A * B with rows sorted); computed once"""
    sq = small_ints(random_csr(600, 600, 0.03, 11, sorted_rows=False), 1)
    a = small_ints(random_csr(400, 300, 0.03, 12, sorted_rows=False), 2)
    b = small_ints(random_csr(300, 500, 0.03, 13, sorted_rows=False), 3)
    hollow = _empty_middle_block(b, 3)
    return {"600x600 squared": (sq, sq, po.omp_spmm(sq, sq).canonical()),
            "400x300 . 300x500": (a, b, po.omp_spmm(a, b).canonical()),
            "block 1 of B empty": (a, hollow, po.omp_spmm(a, hollow).canonical())}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,c", [("600x600 squared", 2), ("600x600 squared", 3), ("400x300 . 300x500", 2),
                                    ("400x300 . 300x500", 3), ("block 1 of B empty", 3)])
def test_blockwise_product_is_the_whole_product(handle, products, name, c, dtype):
    A, B, want = products[name]
    dA, dB = typed_plain(A, dtype).toGpuCSR(), typed_plain(B, dtype).toGpuCSR()
    whole = hs.gpuSpMMWrapper(dA, dB, handle)
    pB = hs.PCSR(dB, c, handle)
    pC = pB.spmm_left(dA, handle)
    try:
        assert handle.stats()["nnzC"] == pC.block(c - 1).nnz            # the statistics describe the last block
        assert (pC.rows, pC.cols, pC.c, pC.stride) == (A.rows, B.cols, c, pB.stride)
        assert all((blk.rows, blk.cols) == (A.rows, pB.stride) for blk in pC.blocks)
        if name == "block 1 of B empty":
            assert pB.block(1).nnz == 0 and pC.block(1).nnz == 0
            assert not hs.d2h(pC.block(1).rowPtr, A.rows + 1, np.int32).any()
        joined = pC.join(handle)
        try:
            hs.sort_rows_device(joined, handle)
            hs.sort_rows_device(whole, handle)
            d = joined.diff(whole, rel=0.0, abs=0.0, handle=handle)
            assert (d.rows_len_differ, d.only_a, d.only_b, d.beyond) == (0, 0, 0, 0), d.as_dict()
            assert joined.nnz == whole.nnz == want.nnz
            got = joined.toCpuCSR()
            assert np.array_equal(got.rowPtr, want.rowPtr) and np.array_equal(got.colInd, want.colInd)
            assert np.array_equal(got.values, want.values.astype(dtype))   # small integers: exact on every side
        finally:
            joined.deviceDispose()
    finally:
        pC.deviceDispose()
        pB.deviceDispose()
        for d in (whole, dA, dB):
            d.deviceDispose()


def test_a_failing_block_clears_every_output(handle, products):
    """the double product runs a symbolic phase, which the test hook makes fail: block 0 fails, every output slot is NULL,
    the failing block's status and message come back, and the same call then succeeds on the same handle"""
    L = hs.lib()
    A, B, _ = products["400x300 . 300x500"]
    dA, dB = typed_plain(A, np.float64).toGpuCSR(), typed_plain(B, np.float64).toGpuCSR()
    pB = hs.PCSR(dB, 3, handle)
    try:
        outs = [(C.c_void_p * 3)(1, 1, 1) for _ in range(3)] + [(C.c_int * 3)(7, 7, 7)]
        handle.fail_next(1)
        rc = L.hip_pcsr_spmm_f64(handle.ptr, C.c_void_p(dA.rowPtr), C.c_void_p(dA.colInd), C.c_void_p(dA.values), dA.nnz, dA.rows,
                                 dA.cols, dB.cols, 3, *hs._block_table(pB._table()), *outs)
        assert rc == 6 and b"forced failure" in L.spgemm_hip_last_error()               # SPGEMM_ERR_INTERNAL
        assert [list(a) for a in outs[:3]] == [[None] * 3] * 3 and list(outs[3]) == [0, 0, 0]
        pC = pB.spmm_left(dA, handle)
        assert sum(blk.nnz for blk in pC.blocks) > 0
        pC.deviceDispose()
    finally:
        pB.deviceDispose()
        dA.deviceDispose()
        dB.deviceDispose()


# ---- the reference's experiment --------------------------------------------------------------------------------------
def test_cpp_mirror_runs_the_column_partition_experiment():
    """tests/cpp/pcsr_check.cc: the flow of the reference's correctTests/pcsrTest.cc on the C++ mirror, c = 2 and c = 3"""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-B", "-C", cpp, "pcsr_check.x"])
    for c in ("2", "3"):
        out = subprocess.run([os.path.join(cpp, "pcsr_check.x"), os.path.join(DATA, "own_graph.snap"), c], capture_output=True,
                             text=True, timeout=120)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "Same" in out.stdout and "Diffs" not in out.stdout


@pytest.mark.parametrize("c", [2, 3])
def test_python_pcsr_round_trip(handle, c):
    """the same input through the Python class: from_csr -> spmm_left -> join -> isEqual"""
    A = po.load(os.path.join(DATA, "own_graph.snap"), isTrans=True, mode=1)
    dA = hs.CSR.from_arrays(A.rowPtr, A.colInd, A.values, A.rows, A.cols).toGpuCSR()
    whole = hs.gpuSpMMWrapper(dA, dA, handle)
    pB = hs.PCSR.from_csr(dA, c, handle)
    pC = pB.spmm_left(dA, handle)
    joined = pC.join(handle)
    try:
        assert (pC.nnz(), joined.nnz) == (whole.nnz, whole.nnz)
        before = whole.toCpuCSR()
        same = pC.isEqual(whole, handle)
        assert_bits(whole.toCpuCSR(), before, "isEqual leaves its argument alone")
        hs.sort_rows_device(joined, handle)
        hs.sort_rows_device(whole, handle)
        d = joined.diff(whole, rel=1e-6, abs=1e-7, handle=handle)
        print(f"c={c}: max_abs_err={d.max_abs_err!r} max_rel_err={d.max_rel_err!r} isEqual={same}")
        assert (d.rows_len_differ, d.only_a, d.only_b, d.beyond) == (0, 0, 0, 0), d.as_dict()
        assert same
        assert whole.nnz != dA.nnz and not pC.isEqual(dA, handle)           # another nnz: refused
    finally:
        for d in (joined, whole, dA):
            d.deviceDispose()
        pC.deviceDispose()
        pB.deviceDispose()
