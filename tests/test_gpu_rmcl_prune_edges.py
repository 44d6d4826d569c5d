"""GPU: the R-MCL row rule on rows in device memory (csrc/rmcl_rows_device.hpp: k_rmcl_stats / k_rmcl_compact / k_rmcl_move
/ k_rmcl_fix_rows, one body for float and double) at the row lengths where its lane strides can go wrong, against the
float64 reference of rmcl_f64_ref.py on the inputs promoted to float64.

Prune (hip_rmcl_prune[_n][_f64]): L lanes share a row, L = 16 when nnz < 96 * m, else a wave of 64.  Pass 1 loads 4 * L
entries per trip and pass 2 compacts 2 * L; the row lengths straddle both steps of both forms, m = 13 is no multiple of
the 16 (4) rows a block takes, so the padded dead rows of the last block take part in the ballots.
Fused float step (hip_rmcl_expand_prune): four rows of more than 4096 products are written out in full and fixed in
place by k_rmcl_fix_rows<float>, 256 entries per trip; their product rows have 255, 256, 257 and 513 entries.

Values alternate exactly between a high band [0.63, 0.77] and a low band [0.15, 0.25] (prune: by position in the row,
fused: by column of B), so that every threshold falls between the bands: each case first asserts, on the reference
alone, that every row's gap (min |v^2 - th| / th) is at least 1000 times the value bound.  Under that precondition the
device must keep exactly the reference's entries (no tie allowance), every value within bound * reference.
Bound: rmcl_f64_ref.step_bound(N, n, u) = (8 N + 2 n + 16) u with u = 2^-24 (float) or 2^-53 (double), n the longest
row, N the terms per product entry (0 for the prune: the same C on both sides).

Fused epilogues (csrc/spgemm_device.hpp: prune_emit_group / prune_emit_block, one body for both value types, inside
k_num_g16<V>, k_num_hash and k_num64_rows): three small products whose rows sit on the edges of those bodies, see EPILOGUE_ROWS,
each run as the float step with and without its symbolic pass and as the double step.  Float results go against the oracle's
rule (helpers.assert_rmcl_step) with no row allowed to differ, double ones against rmcl_f64_ref.step64."""
import functools

import numpy as np
import pytest

from f64ref import Host64, sorted_rows
from helpers import assert_rmcl_step, po
from rmcl_f64_ref import row_rule64, step64, step_bound
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu

UNIT = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
# lanes per row -> the row lengths of the case
LENGTHS = {16: [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129],
           64: [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513]}
NCOLS = 600


@pytest.fixture(scope="module")
def handle():
    if hs.device_count() < 1:
        pytest.fail("GPU test without a HIP device")
    return hs.Handle(0)


def banded(rng, position, dtype, low=(0.15, 0.25)):
    """high band at even positions, low band at odd ones, rounded to dtype"""
    hi = rng.uniform(0.63, 0.77, len(position))
    lo = rng.uniform(low[0], low[1], len(position))
    return np.where(position % 2 == 0, hi, lo).astype(dtype)


def length_classes(L):
    """row lengths up to one compaction half-step, one compaction step (2 L), one load step (4 L), and beyond"""
    return [(1, L), (L + 1, 2 * L), (2 * L + 1, 4 * L), (4 * L + 1, 1 << 30)]


@functools.lru_cache(maxsize=None)
def prune_case(dtype, L):
    """-> (C as Host64 of dtype-rounded values, reference result, bound): built once, shared, never modified"""
    lens = LENGTHS[L]
    m = len(lens)
    rng = np.random.default_rng(100 + L)
    rp = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = np.concatenate([rng.permutation(NCOLS)[:l] for l in lens]).astype(np.int32)
    pos = np.concatenate([np.arange(l) for l in lens])
    Cm = Host64(rp, ci, banded(rng, pos, dtype), m, NCOLS)
    assert m % (256 // L) != 0 and (Cm.nnz >= 96 * m) == (L == 64)         # the form the library picks, dead rows in its last block
    want, _, gap = row_rule64(Cm.rowPtr, Cm.colInd, Cm.values)
    bound = step_bound(0, max(lens), UNIT[dtype])
    assert float(gap.min()) >= 1000.0 * bound, f"bad input, smallest gap {gap.min():.3e} < 1000 * bound {bound:.3e}"
    kept = np.diff(want.rowPtr)
    for lo, hi in length_classes(L):
        assert any(lo <= l <= hi and 0 < k < l for l, k in zip(lens, kept)), f"no row of {lo}..{hi} entries loses any"
    return Cm, want, bound


def take(out, rows, cols, dtype):
    """(I, J, V, nnz) of pool arrays -> host CSR; the device arrays are released"""
    i_, j_, v_, n_ = out
    d = hs.CSR(v_, j_, i_, rows, cols, n_, True, dtype=dtype)
    try:
        return d.toCpuCSR()
    finally:
        d.deviceDispose()


@pytest.mark.parametrize("L", [16, 64])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_prune_at_the_lane_strides(handle, dtype, L):
    Cm, want, bound = prune_case(dtype, L)
    prune = hs.rmcl_prune_raw if dtype is np.float32 else hs.rmcl_prune_raw_f64
    dC = hs.CSR.from_arrays(Cm.rowPtr, Cm.colInd, Cm.values, Cm.rows, Cm.cols, dtype=dtype).toGpuCSR()
    try:
        a = take(prune(handle, Cm.rows, dC.rowPtr, dC.colInd, dC.values), Cm.rows, Cm.cols, dtype)
        b = take(prune(handle, Cm.rows, dC.rowPtr, dC.colInd, dC.values, nnz=Cm.nnz), Cm.rows, Cm.cols, dtype)
        back = dC.toCpuCSR()
    finally:
        dC.deviceDispose()
    assert back.values.dtype == dtype and a.values.dtype == dtype
    assert np.array_equal(back.rowPtr, Cm.rowPtr) and np.array_equal(back.colInd, Cm.colInd)       # the input is left alone
    assert np.array_equal(back.values.astype(np.float64), Cm.values)
    assert np.array_equal(a.rowPtr, want.rowPtr)
    assert np.array_equal(a.colInd, want.colInd), "kept entries are not the reference's, in input order"   # stable compaction
    err = np.abs(a.values.astype(np.float64) - want.values)
    print(f"{np.dtype(dtype).name} L={L}: kept {want.nnz} of {Cm.nnz}, worst relative error "
          f"{float((err / want.values).max()):.3e}, bound {bound:.3e}")
    assert np.all(err <= bound * want.values)
    for x, y in ((a.rowPtr, b.rowPtr), (a.colInd, b.colInd), (a.values, b.values)):
        assert np.array_equal(x, y), "hip_rmcl_prune and hip_rmcl_prune_n differ"


# ---- k_rmcl_fix_rows<float> at its 256-entry stride ----------------------------------------------------------------
FIX_L = [255, 256, 257, 513]
FIX_TERMS = 17


@functools.lru_cache(maxsize=None)
def fix_rows_case():
    """-> (A, B, Step64 of A * B) with float32-rounded values; row r of A * B has FIX_L[r] entries of FIX_TERMS terms"""
    rng = np.random.default_rng(7)
    n = max(FIX_L)
    A = Host64(np.arange(len(FIX_L) + 1) * FIX_TERMS, np.arange(len(FIX_L) * FIX_TERMS),
               (rng.uniform(0.9, 1.1, len(FIX_L) * FIX_TERMS) / FIX_TERMS).astype(np.float32), len(FIX_L), len(FIX_L) * FIX_TERMS)
    blen = np.repeat(FIX_L, FIX_TERMS)
    brp = np.zeros(len(blen) + 1, np.int32)
    np.cumsum(blen, out=brp[1:])
    bci = np.concatenate([np.arange(l) for l in blen])
    B = Host64(brp, bci, banded(rng, bci, np.float32), len(blen), n)
    return A, B, step64(A, B)


def test_fused_float_step_fixes_full_rows_in_place(handle):
    A, B, step = fix_rows_case()
    bound = step_bound(FIX_TERMS, max(FIX_L), UNIT[np.float32])
    assert step.N == FIX_TERMS and step.n == max(FIX_L)
    assert list(np.diff(step.product.rowPtr)) == FIX_L and list(np.diff(step.kept.rowPtr)) == [128, 128, 129, 257]
    assert float(step.gap.min()) >= 1000.0 * bound, f"bad input, smallest gap {step.gap.min():.3e} < 1000 * bound {bound:.3e}"
    dA = hs.CSR.from_arrays(A.rowPtr, A.colInd, A.values, A.rows, A.cols, dtype=np.float32).toGpuCSR()
    dB = hs.CSR.from_arrays(B.rowPtr, B.colInd, B.values, B.rows, B.cols, dtype=np.float32).toGpuCSR()
    try:
        got = take(hs.rmcl_expand_prune_raw(handle, dA.rowPtr, dA.colInd, dA.values, dA.nnz, dB.rowPtr, dB.colInd, dB.values,
                                            dB.nnz, A.rows, A.cols, B.cols), A.rows, B.cols, np.float32)
        bins = handle.stats()["bin_rows"]
    finally:
        dA.deviceDispose()
        dB.deviceDispose()
    # every row has more than 4096 products: the last bin, written out in full and fixed in place
    assert bins[-1] == len(FIX_L) and sum(bins) == len(FIX_L), bins
    assert got.values.dtype == np.float32
    assert np.array_equal(got.rowPtr, step.kept.rowPtr)
    gc, gv = sorted_rows(got.rowPtr, got.colInd, got.values)
    wc, wv = sorted_rows(step.kept.rowPtr, step.kept.colInd, step.kept.values)
    assert np.array_equal(gc, wc), "kept columns"
    err = np.abs(gv.astype(np.float64) - wv)
    print(f"fix_rows<float>: kept {len(wv)}, worst relative error {float((err / wv).max()):.3e}, bound {bound:.3e}")
    assert np.all(err <= bound * wv)


# ---- the fused epilogues at their edges ----------------------------------------------------------------------------
# (terms, columns) per row: the row of A has `terms` entries, each on a B row of its own with the columns 0..columns-1, so
# the product row has terms * columns products on `columns` distinct columns.  The rows of a 16-lane wave take one path
# together, so rows with repeated columns (hashed) are kept out of the products whose rows are plain lists.
EPILOGUE_ROWS = {
    # 16 lanes per row, the products as a plain list (float: with the symbolic pass; hashed without it): lengths that are
    # no multiple of 16, both table sizes (up to 16 and 17..64 products); 3 and 2 rows per launch, so the block's other
    # 16-lane groups are dead beside live ones
    "list16": [(1, 1), (1, 15), (1, 16), (1, 17), (1, 64)],
    # a wave per row at 65 and 512 products (float: list with the symbolic pass, else hashed); float blocks of 4 and 8
    # waves at 513, 2048, 2049 and 4096 products; double: one block per row, tables of 256 to 8192 slots
    "long": [(1, 65), (1, 512), (1, 513), (1, 2048), (1, 2049), (1, 4096)],
    # fewer distinct columns than products, hashed in every mode: 16 lanes at both table sizes (14 and 40 products), a
    # wave per row at 65 and 512 products, 513 products on 19 columns (double: a 64-slot table under 256 threads and 16
    # steps, of which one is live and three quarters of its threads hold no slot)
    "hashed": [(2, 7), (2, 20), (5, 13), (2, 256), (27, 19)],
}


@functools.lru_cache(maxsize=None)
def epilogue_case(name):
    """-> (A, B as Host64 of float32-rounded values, Step64 of A * B): built once, shared, never modified"""
    spec = EPILOGUE_ROWS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    terms = np.array([t for t, _ in spec])
    arp = np.zeros(len(spec) + 1, np.int32)
    np.cumsum(terms, out=arp[1:])
    aval = (rng.uniform(0.98, 1.02, arp[-1]) / np.repeat(terms, terms)).astype(np.float32)
    A = Host64(arp, np.arange(arp[-1]), aval, len(spec), arp[-1])
    blen = np.repeat([l for _, l in spec], terms)
    brp = np.zeros(len(blen) + 1, np.int32)
    np.cumsum(blen, out=brp[1:])
    bci = np.concatenate([np.arange(l) for l in blen])
    B = Host64(brp, bci, banded(rng, bci, np.float32, low=(0.05, 0.10)), len(blen), int(blen.max()))
    return A, B, step64(A, B)


@pytest.mark.parametrize("name", list(EPILOGUE_ROWS))
@pytest.mark.parametrize("mode", ["float", "float-symbolic", "double"])
def test_fused_epilogues_at_their_edges(handle, mode, name, monkeypatch):
    dtype = np.float64 if mode == "double" else np.float32
    if mode == "float-symbolic":
        monkeypatch.setenv("SPGEMM_RMCL_SYMBOLIC", "1")
    else:
        monkeypatch.delenv("SPGEMM_RMCL_SYMBOLIC", raising=False)
    A, B, step = epilogue_case(name)
    spec = EPILOGUE_ROWS[name]
    bound = step_bound(step.N, step.n, UNIT[dtype])
    assert step.N == max(t for t, _ in spec) and list(np.diff(step.product.rowPtr)) == [l for _, l in spec]
    assert float(step.gap.min()) >= 1000.0 * bound, f"bad input, smallest gap {step.gap.min():.3e} < 1000 * bound {bound:.3e}"
    kept = np.diff(step.kept.rowPtr)
    assert all(0 < k < l or l == 1 for k, (_, l) in zip(kept, spec)), "a row keeps all or nothing"
    dA = hs.CSR.from_arrays(A.rowPtr, A.colInd, A.values, A.rows, A.cols, dtype=dtype).toGpuCSR()
    dB = hs.CSR.from_arrays(B.rowPtr, B.colInd, B.values, B.rows, B.cols, dtype=dtype).toGpuCSR()
    call = hs.rmcl_expand_prune_raw_f64 if mode == "double" else hs.rmcl_expand_prune_raw
    try:
        got = take(call(handle, dA.rowPtr, dA.colInd, dA.values, dA.nnz, dB.rowPtr, dB.colInd, dB.values, dB.nnz,
                        A.rows, A.cols, B.cols), A.rows, B.cols, dtype)
        bins = handle.stats()["bin_rows"]
    finally:
        dA.deviceDispose()
        dB.deviceDispose()
    products = [t * l for t, l in spec]
    edges = [16, 64, 512, 2048, 4096, 1 << 30]                          # the last five bins, one numeric launch each
    assert bins[-5:] == [sum(lo < p <= hi for p in products) for lo, hi in zip(edges[:-1], edges[1:])], bins
    assert sum(bins) == len(spec)
    assert got.values.dtype == dtype
    assert np.array_equal(got.rowPtr, step.kept.rowPtr)
    gc, gv = sorted_rows(got.rowPtr, got.colInd, got.values)
    wc, wv = sorted_rows(step.kept.rowPtr, step.kept.colInd, step.kept.values)
    assert np.array_equal(gc, wc), "kept columns"
    if mode == "double":
        err = np.abs(gv - wv)
        print(f"{name} {mode}: kept {len(wv)}, worst relative error {float((err / wv).max()):.3e}, bound {bound:.3e}")
        assert np.all(err <= bound * wv)
    else:
        ndiff, _, _ = assert_rmcl_step(got, po.CSRHost(A.rowPtr, A.colInd, A.values, A.rows, A.cols),
                                       po.CSRHost(B.rowPtr, B.colInd, B.values, B.rows, B.cols), what=f"{name} {mode}")
        assert ndiff == 0, f"{ndiff} rows differ from the oracle's"
