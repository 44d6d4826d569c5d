"""The test kit of the device-CSR formats (reorder, compare, pcsr, bcsr, mcsr, coo) and of the modules around them: the
fixtures and helpers that two or more test modules used to spell out themselves.  A plain module, imported by name:

    from devcsr import built_gpu, handle  # noqa: F401      (pytest registers a fixture in the importing module, so
                                                             module scope and autouse mean "per test module", as before)
    from devcsr import typed, take, assert_bits

pytest does not rewrite the asserts of a helper module: every assert here carries its message."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

import reorder_ref as rr
from helpers import canonical_arrays, po, synth_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs


# ---- fixtures --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def built():
    """the native pieces are compiled (the *_abi.py modules: no GPU needed)"""
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(scope="module", autouse=True)
def built_gpu():
    """the native pieces are compiled and there is a HIP device (the test_gpu_*.py modules)"""
    import __graft_entry__ as ge
    ge.build()
    assert hs.device_count() >= 1, "no HIP device"


@pytest.fixture(scope="module")
def handle():
    h = hs.Handle(0)
    yield h
    h.close()


@pytest.fixture(scope="module", autouse=True)
def _seasoned_pool(built_gpu):
    """For the modules that compare the pool's cached bytes (test_gpu_rmcl_pool.py, test_gpu_spgemm_pool.py).  The figure
    compared is the pool's cached bytes, so no call may fetch a block from the driver: such a block is
    cached when it is released, and the figure grows although nothing leaked -- in whichever call first finds no fitting
    block, which depends on what earlier tests left in the pool (the best fit of a call's requests moves once its own
    blocks are in the cache).  A ladder of blocks from 1 KiB to 8 MiB, 12 per octave, is cached up front: every request
    of these calls (the largest is the 2.7 MB scratch product of iteration 2) finds a block, whatever ran before, and a
    block that is not released always shows, because its replacement comes out of the cache."""
    for p in [hs.dev_alloc(int(n)) for n in np.geomspace(1 << 10, 1 << 23, 160)]:
        hs.dev_free(p)


def twice(call, device=0):
    """warm, record, run again: the cached bytes must not have moved; -> what the second run returned"""
    call()
    before = hs.pool_cached_bytes(device)
    out = call()
    after = hs.pool_cached_bytes(device)
    assert after == before, f"cached bytes moved by {after - before}"
    return out


# ---- inputs (made once by their callers, never modified) -------------------------------------------------------------
def with_nnz(rows, cols, nnz, seed):
    """exactly nnz entries over `rows` rows, random columns (repeats allowed), some rows empty"""
    rng = np.random.default_rng(seed)
    owner = np.sort(rng.integers(0, rows, size=nnz))
    rp = np.zeros(rows + 1, np.int32)
    np.cumsum(np.bincount(owner, minlength=rows), out=rp[1:])
    return rr.Host(rp, rng.integers(0, cols, size=nnz), (rng.random(nnz) + 0.25).astype(np.float32), rows, cols)


def one_long_row(rows=300, cols=300, row=17):
    """row `row` holds 20 000 entries (columns repeat), every other row is empty"""
    rng = np.random.default_rng(17)
    rp = np.zeros(rows + 1, np.int32)
    rp[row + 1:] = 20000
    return rr.Host(rp, rng.integers(0, cols, size=20000), (rng.random(20000) + 0.25).astype(np.float32), rows, cols)


def _plain(M):
    return rr.Host(M.rowPtr, M.colInd, M.values, M.rows, M.cols)


def _special(dtype):
    """name -> value: NaN with a payload, -0.0, a denormal, 1e-9 and the next number above it, in `dtype`"""
    dt = np.dtype(dtype)
    nan = np.array([0x7fc12345] if dt == np.float32 else [0x7ff8000012345678], np.uint32 if dt == np.float32 else np.uint64).view(dt)[0]
    tiny = np.array([1], np.uint32 if dt == np.float32 else np.uint64).view(dt)[0]
    at = dt.type(1e-9)
    return {"nan": nan, "-0": dt.type(-0.0), "denormal": tiny, "1e-9": at, "above": np.nextafter(at, dt.type(1))}


def _strided_tiles(ntiles, side, tile):
    """side x side, one entry in the top left cell of each of the first `ntiles` tile x tile tiles"""
    per_row = (side + tile - 1) // tile
    t = np.arange(ntiles, dtype=np.int64)
    rows_of, cols_of = (t // per_row) * tile, (t % per_row) * tile
    rp = np.zeros(side + 1, np.int64)
    np.cumsum(np.bincount(rows_of, minlength=side), out=rp[1:])
    return rr.Host(rp, cols_of, np.ones(ntiles, np.float32), side, side)


def _graph(m, seed):
    """the R-MCL start matrix of a synthetic graph: transpose + self loops + row-normalise"""
    A = synth_csr(m, seed, 2)
    ri = np.repeat(np.arange(A.rows, dtype=np.int32), np.diff(A.rowPtr))
    return po.rmcl_init(A.rows, A.cols, A.colInd, ri, np.ones_like(A.values))


def start_graph(base):
    """a 2000-node power-law graph as R-MCL starts from it (transpose + self loops + row-normalise); host and device"""
    A = synth_csr(2000, 7, base)
    ri = np.repeat(np.arange(A.rows, dtype=np.int32), np.diff(A.rowPtr))
    M0 = po.rmcl_init(A.rows, A.cols, A.colInd, ri, np.ones_like(A.values))
    return M0, hs.CSR.from_arrays(M0.rowPtr, M0.colInd, M0.values, M0.rows, M0.cols).toGpuCSR()


def unpack(z, prefix):
    r, c = z[prefix + "_shape"]
    return po.CSRHost(z[prefix + "_rowPtr"], z[prefix + "_colInd"], z[prefix + "_values"], int(r), int(c))


# ---- host <-> device -------------------------------------------------------------------------------------------------
def to_hs(M):
    return hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols)


def typed(M, dtype):
    """host hs.CSR of M; float64 values get bits a float cannot hold"""
    v = np.asarray(M.values, np.float64)
    if np.dtype(dtype) == np.float64:
        v = v + 2.0 ** -40
    return hs.CSR.from_arrays(M.rowPtr, M.colInd, v, M.rows, M.cols, dtype=dtype)


def typed_plain(M, dtype):
    return hs.CSR.from_arrays(M.rowPtr, M.colInd, np.asarray(M.values, dtype), M.rows, M.cols, dtype=dtype)


def take(dev):
    host = dev.toCpuCSR()
    dev.deviceDispose()
    return host


def taken(i, j, v, n, rows, dtype=np.float32):
    """host copy of a raw device result, which is freed"""
    out = (hs.d2h(i, rows + 1, np.int32), hs.d2h(j, n, np.int32), hs.d2h(v, n, dtype))
    for p in (i, j, v):
        hs.dev_free(p)
    return out


def assert_bits(got, want, what=""):
    assert got.rows == want.rows and got.cols == want.cols, what
    assert np.array_equal(np.asarray(got.rowPtr), np.asarray(want.rowPtr)), f"{what}: rowPtr"
    assert np.array_equal(np.asarray(got.colInd), np.asarray(want.colInd)), f"{what}: colInd"
    g, w = np.ascontiguousarray(got.values), np.ascontiguousarray(want.values)
    assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: value bits"


# ---- products on a fresh handle, compared bit for bit (the big-row, mid-row and wide-column modules) ------------------
def env_handle(**env):
    """a fresh handle; the SPGEMM_* knobs are read when it is created"""
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return hs.Handle(0)
    finally:
        for k in env:
            del os.environ[k]


def int_csr(rows, ncols, seed, lo=1, hi=4):
    """rows: column arrays; values: small integers (any summation order is exact)"""
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    v = rng.integers(lo, hi + 1, size=len(ci)).astype(np.float32)
    return po.CSRHost(rp, ci, v, len(rows), ncols)


def row_flops(A, B):
    """products of every row of A * B"""
    blen = np.diff(np.asarray(B.rowPtr, np.int64))
    per = blen[np.asarray(A.colInd)]
    rp = np.asarray(A.rowPtr, np.int64)
    return np.array([per[rp[i]:rp[i + 1]].sum() for i in range(A.rows)])


def float_bits(M):
    c, v = canonical_arrays(M.rowPtr, M.colInd, M.values)
    return np.asarray(M.rowPtr, np.int32).tobytes(), c.tobytes(), v.view(np.uint32).tobytes()


def same_bits(got, want, what, zero_signs=True):
    """rowPtr, per-row sorted columns and float value bits.  zero_signs=False: +0.0 and -0.0 count as equal (the oracle's
    accumulators start from +0.0)"""
    g, w = float_bits(got), float_bits(want)
    assert g[0] == w[0], f"{what}: rowPtr differs"
    assert g[1] == w[1], f"{what}: columns differ"
    if zero_signs:
        assert g[2] == w[2], f"{what}: value bits differ"
    else:
        assert np.array_equal(canonical_arrays(got.rowPtr, got.colInd, got.values)[1],
                              canonical_arrays(want.rowPtr, want.colInd, want.values)[1]), f"{what}: values differ"


def bigrow_handle(**env):
    """env_handle with SPGEMM_BD_MINROWS=1 unless the caller says otherwise: a product with fewer big rows than the device has
    CUs keeps the hash kernel by default, and the cases of these modules are a handful of rows"""
    env.setdefault("SPGEMM_BD_MINROWS", 1)
    return env_handle(**env)


def bigrow_mul(h, A, B):
    """-> (A * B on handle h as a host CSR, the big-row routes it took)"""
    dA, dB = to_hs(A).toGpuCSR(), to_hs(B).toGpuCSR()
    dC = hs.gpuSpMMWrapper(dA, dB, h)
    got = dC.toCpuCSR()
    for d in (dC, dA, dB):
        d.deviceDispose()
    return got, h.bigrow_paths()


def bigrow_twice(A, B, what, direct, zero_signs=True, want=None, **env):
    """A fresh handle whose first call has big rows (no log yet: every row takes the hash kernel), then the same call again
    (`direct` rows take the direct kernel); both equal the reference bit for bit (want; None: the oracle's product).  Returns
    the second result and its routes."""
    if want is None:
        want = po.sequential_spmm(A, B)
    nbig = int((row_flops(A, B) > 4096).sum())
    h = bigrow_handle(**env)
    try:
        got1, p1 = bigrow_mul(h, A, B)
        same_bits(got1, want, what + " (first call)", zero_signs)
        assert (p1["direct"], p1["fallback"]) == (0, nbig), f"{what}: first call {p1}"
        got2, p2 = bigrow_mul(h, A, B)
        same_bits(got2, want, what + " (second call)", zero_signs)
        if direct is not None:
            assert (p2["direct"], p2["fallback"]) == (direct, nbig - direct), f"{what}: second call {p2}"
    finally:
        h.close()
    return got2, p2


# ---- the rest --------------------------------------------------------------------------------------------------------
def _outs(n=3):
    """n non-null output slots for an entry point that must fail before it writes them"""
    return [C.c_void_p(1) for _ in range(n)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p
