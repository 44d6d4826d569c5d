"""GPU: every branch of the R-MCL row rule in every device body that applies it -- k_rmcl_stats + k_rmcl_compact (16 lanes
and a wave per row), prune_emit_group<16> (plain list and hashed), prune_emit_group<64>, prune_emit_block over WaveSegments
and over BlockStrided, k_rmcl_fix_rows -- in float and in double, on the rows of rmcl_rule_cases.py: the threshold raised
to the floor 1e-7 (formula negative; formula positive but small), lowered to the row maximum (entries survive by equality
alone), an entry equal to its threshold, signs and explicit zeros, one-entry and empty rows.

Every case asserts its preconditions on the reference alone when it is built (branch, kept set, gap >= 1000 * bound for
every entry whose fate does not follow from identical input bits; tests/test_rmcl_rule_cases_ref.py runs the same
builders without a GPU).  On the device: the route the case names was taken (bin_rows; lanes by nnz < 96 * m), rowPtr and
kept columns exact (in input order for the prune), every value within step_bound(N, n, u) of the float64 rule on the
dtype-rounded inputs, and the rows whose result follows from exact arithmetic (cap, uniform, one entry) bit for bit.  The
float fused cases also pass helpers.assert_rmcl_step with no differing row, and every fused case equals hip_gpuSpMM followed
by hip_rmcl_prune.  Each test prints its worst relative error beside its bound."""
import functools

import numpy as np
import pytest

import rmcl_rule_cases as rc
from f64ref import Host64, sorted_rows
from helpers import assert_rmcl_step, po
from rmcl_f64_ref import row_rule64
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def handle():
    if hs.device_count() < 1:
        pytest.fail("GPU test without a HIP device")
    return hs.Handle(0)


@functools.lru_cache(maxsize=None)
def prune_case(lanes, dtype):
    return rc.PruneCase(rc.PRUNE_LENGTHS[lanes], dtype)


@functools.lru_cache(maxsize=None)
def fused_case(name, dtype):
    lengths, terms, _ = rc.FUSED_LAUNCHES[name]
    return rc.FusedCase(lengths, dtype, terms)


# ---- device calls ----------------------------------------------------------------------------------------------------
def dev(M, dtype):
    return hs.CSR.from_arrays(M.rowPtr, M.colInd, M.values, M.rows, M.cols, dtype=dtype).toGpuCSR()


def take(out, rows, cols, dtype):
    """(I, J, V, nnz) of pool arrays -> host CSR; the device arrays are released"""
    i_, j_, v_, n_ = out
    d = hs.CSR(v_, j_, i_, rows, cols, n_, True, dtype=dtype)
    try:
        return d.toCpuCSR()
    finally:
        d.deviceDispose()


def run_prune(handle, Cm, dtype):
    """-> (hip_rmcl_prune's result, hip_rmcl_prune_n's, the input read back)"""
    prune = hs.rmcl_prune_raw if dtype is F32 else hs.rmcl_prune_raw_f64
    dC = dev(Cm, dtype)
    try:
        a = take(prune(handle, Cm.rows, dC.rowPtr, dC.colInd, dC.values), Cm.rows, Cm.cols, dtype)
        b = take(prune(handle, Cm.rows, dC.rowPtr, dC.colInd, dC.values, nnz=Cm.nnz), Cm.rows, Cm.cols, dtype)
        back = dC.toCpuCSR()
    finally:
        dC.deviceDispose()
    assert np.array_equal(back.rowPtr, Cm.rowPtr) and np.array_equal(back.colInd, Cm.colInd)       # the input is left alone
    assert np.array_equal(back.values.astype(F64), Cm.values), "the input does not survive the round trip in this dtype"
    for x, y in ((a.rowPtr, b.rowPtr), (a.colInd, b.colInd), (a.values, b.values)):
        assert np.array_equal(x, y), "hip_rmcl_prune and hip_rmcl_prune_n differ"
    return a


def run_fused(handle, A, B, dtype):
    """-> (the fused step, bin_rows of its classification, hip_gpuSpMM followed by hip_rmcl_prune on the same operands)"""
    f64 = dtype is F64
    step = hs.rmcl_expand_prune_raw_f64 if f64 else hs.rmcl_expand_prune_raw
    spmm = hs.gpu_spmm_raw_f64 if f64 else hs.gpu_spmm_raw
    prune = hs.rmcl_prune_raw_f64 if f64 else hs.rmcl_prune_raw
    dA, dB = dev(A, dtype), dev(B, dtype)
    try:
        ops = (dA.rowPtr, dA.colInd, dA.values, dA.nnz, dB.rowPtr, dB.colInd, dB.values, dB.nnz, A.rows, A.cols, B.cols)
        one = take(step(handle, *ops), A.rows, B.cols, dtype)
        bins = list(handle.stats()["bin_rows"])
        ic, jc, vc, nnz = spmm(handle, *ops)
        try:
            two = take(prune(handle, A.rows, ic, jc, vc, nnz=nnz), A.rows, B.cols, dtype)
        finally:
            for p in (ic, jc, vc):
                hs.dev_free(p)
    finally:
        dA.deviceDispose()
        dB.deviceDispose()
    return one, bins, two


# ---- assertions ------------------------------------------------------------------------------------------------------
def assert_result(got, want, bound, kinds, dtype, what, in_order=False):
    """rowPtr and kept columns exact (rows sorted by column unless in_order), values within bound * reference, the rows of
    a kind in rc.EXACT bit for bit"""
    assert got.values.dtype == dtype, what
    assert np.array_equal(np.asarray(got.rowPtr), want.rowPtr), f"{what}: row pointer {list(got.rowPtr)} vs {list(want.rowPtr)}"
    if in_order:
        gc, gv, wc, wv = np.asarray(got.colInd), np.asarray(got.values), want.colInd, want.values
    else:
        gc, gv = sorted_rows(got.rowPtr, got.colInd, got.values)
        wc, wv = sorted_rows(want.rowPtr, want.colInd, want.values)
    assert np.array_equal(gc, wc), f"{what}: kept columns"
    err = np.abs(gv.astype(F64) - wv)
    worst = float((err / wv).max()) if len(wv) else 0.0
    print(f"{what}: kept {want.nnz}, worst relative error {worst:.3e}, bound {bound:.3e}")
    bad = np.flatnonzero(~(err <= bound * wv))
    assert len(bad) == 0, f"{what}: {len(bad)} values beyond the bound, first {gv[bad[0]]!r} vs {wv[bad[0]]!r}"
    for r, ev in rc.exact_values(kinds, want.rowPtr, dtype).items():
        a, b = want.rowPtr[r], want.rowPtr[r + 1]
        assert np.array_equal(gv[a:b], ev), f"{what}: row {r} ({kinds[r][0]}) is {gv[a:b][:4]!r}..., not {ev[0]!r} bit for bit"


def assert_same_steps(one, two, want, bound, what):
    """the fused step equals SpGEMM + prune: identical structure, values within the bound of one another"""
    assert np.array_equal(one.rowPtr, two.rowPtr), f"{what}: fused and two-step row pointers differ"
    c1, v1 = sorted_rows(one.rowPtr, one.colInd, one.values)
    c2, v2 = sorted_rows(two.rowPtr, two.colInd, two.values)
    assert np.array_equal(c1, c2), f"{what}: fused and two-step kept columns differ"
    _, wv = sorted_rows(want.rowPtr, want.colInd, want.values)
    d = np.abs(v1.astype(F64) - v2.astype(F64))
    print(f"{what}: fused against two steps, worst relative difference {float((d / wv).max()) if len(wv) else 0.0:.3e}, bound {bound:.3e}")
    assert np.all(d <= bound * wv), f"{what}: fused and two-step values differ by more than the bound"


def set_mode(monkeypatch, mode):
    if mode == "float-symbolic":
        monkeypatch.setenv("SPGEMM_RMCL_SYMBOLIC", "1")
    else:
        monkeypatch.delenv("SPGEMM_RMCL_SYMBOLIC", raising=False)
    return rc.MODE_DTYPE[mode]


def as_oracle(M):
    return po.CSRHost(M.rowPtr, M.colInd, M.values, M.rows, M.cols)


# ---- 1. rows in device memory: k_rmcl_stats + k_rmcl_compact -------------------------------------------------------------
@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_prune_every_branch(handle, dtype, lanes):
    case = prune_case(lanes, dtype)
    assert case.lanes == lanes and case.C.rows % (256 // lanes) != 0           # the form the library picks; dead rows in its last block
    got = run_prune(handle, case.C, dtype)
    assert_result(got, case.want, case.bound, case.rows, dtype, f"prune {np.dtype(dtype).name} L={lanes}", in_order=True)


# ---- 2. the fused epilogues and the rows fixed in place --------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [(n, m) for n, (_, _, modes) in rc.FUSED_LAUNCHES.items() for m in modes])
def test_fused_every_branch(handle, name, mode, monkeypatch):
    dtype = set_mode(monkeypatch, mode)
    case = fused_case(name, dtype)
    what = f"{name} {mode}"
    one, bins, two = run_fused(handle, case.A, case.B, dtype)
    assert bins == case.bin_rows, f"{what}: rows per bin {bins}, not {case.bin_rows}"        # every row took the route it names
    # rows written out in full and fixed in place: float beyond 4096 products, double beyond 6144 entries
    assert rc.launch_uses_fix_rows(name, mode) == (name.startswith("fix") or (name == "over-4096" and mode != "double"))
    assert_result(one, case.step.kept, case.bound, case.rows, dtype, what)
    assert_result(two, case.step.kept, case.bound, case.rows, dtype, what + " (SpGEMM + prune)")
    assert_same_steps(one, two, case.step.kept, case.bound, what)
    if dtype is F32:
        ndiff, _, _ = assert_rmcl_step(one, as_oracle(case.A), as_oracle(case.B), what=what)
        assert ndiff == 0, f"{what}: {ndiff} rows differ from the oracle's"


# ---- 3. the float threshold's promotions -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def promotion_rows():
    return [("promotion-kept", rc.promotion_row("kept")[0]), ("empty", np.zeros(0)), ("one", rc.row_values("one", 1)),
            ("promotion-dropped", rc.promotion_row("dropped")[0])]


def promotion_want(C, dtype):
    """the rule with the value type's own threshold: computeThreshold's promotions in float, plain double in double"""
    _, th, _ = row_rule64(C.rowPtr, C.colInd, C.values)
    if dtype is F32:
        for r in (0, 3):
            v = C.values[C.rowPtr[r]:C.rowPtr[r + 1]] ** 2
            th[r] = float(rc.threshold_f32(np.float32(np.cumsum(v)[-1] / len(v)), np.float32(v.max())))
    return rc.kept_with(C, th)


@pytest.mark.parametrize("mode", rc.ALL_MODES)
def test_threshold_promotions(handle, mode, monkeypatch):
    """Two rows whose probe entry lies between the threshold as computeThreshold rounds it in float (mx - avg in float,
    the product in double) and the threshold with mx - avg kept in double, thousands of float ulps from either: the float
    kernels keep the first row's probe and drop the second's, the double kernels the other way round."""
    dtype = set_mode(monkeypatch, mode)
    rows = promotion_rows()
    kept = {r: int(8 - ((which == "dropped") == (dtype is F32))) for r, which in ((0, "kept"), (3, "dropped"))}
    pc = rc.PruneCase((8,), dtype, rows=rows)
    want = promotion_want(pc.C, dtype)
    assert [int(x) for x in np.diff(want.rowPtr)] == [kept[0], 0, 1, kept[3]]
    got = run_prune(handle, pc.C, dtype)
    assert_result(got, want, pc.bound, rows, dtype, f"promotions, prune {mode}", in_order=True)
    fc = rc.FusedCase((8,), dtype, rows=rows)
    prod = fc.step.product
    want = promotion_want(Host64(prod.rowPtr, prod.colInd, prod.values, prod.rows, prod.cols), dtype)
    assert [int(x) for x in np.diff(want.rowPtr)] == [kept[0], 0, 1, kept[3]]
    one, bins, two = run_fused(handle, fc.A, fc.B, dtype)
    assert bins == fc.bin_rows and bins[3] == 2                               # both rows: the 16-lane kernel, up to 16 products
    assert_result(one, want, fc.bound, rows, dtype, f"promotions, fused {mode}")
    assert_result(two, want, fc.bound, rows, dtype, f"promotions, SpGEMM + prune {mode}")
    if dtype is F32:
        ndiff, _, _ = assert_rmcl_step(one, as_oracle(fc.A), as_oracle(fc.B), what=f"promotions {mode}")
        assert ndiff == 0


# ---- 4. the domain edge of the reciprocal ----------------------------------------------------------------------------------
DOMAIN_LAUNCHES = ["g16-list", "g16-hashed", "wave-65", "wave-512", "blocks", "over-4096", "fix-513x16", "fix-6145"]


@pytest.mark.parametrize("lanes", [16, 64])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_prune_at_the_smallest_normal_square(handle, dtype, lanes):
    rows = rc.domain_rows(rc.PRUNE_LENGTHS[lanes] + ((300,) if lanes == 64 else ()), dtype)
    case = rc.PruneCase((), dtype, rows=rows, exact32=False)
    assert case.lanes == lanes
    got = run_prune(handle, case.C, dtype)
    assert_result(got, case.want, case.bound, rows, dtype, f"smallest normal square, prune {np.dtype(dtype).name} L={lanes}", in_order=True)


@pytest.mark.parametrize("name,mode", [(n, m) for n in DOMAIN_LAUNCHES for m in rc.FUSED_LAUNCHES[n][2]])
def test_fused_at_the_smallest_normal_square(handle, name, mode, monkeypatch):
    """squares of 2^-126 (2^-1022): the last at which the reciprocal of a kept sum is a number of the type.  include/
    spgemm_hip.h states this domain at hip_rmcl_expand_prune; every body gives the reference's result on its edge."""
    dtype = set_mode(monkeypatch, mode)
    lengths, terms, _ = rc.FUSED_LAUNCHES[name]
    rows = rc.domain_rows(lengths, dtype)
    case = rc.FusedCase((), dtype, terms, rows=rows, exact32=False)
    what = f"smallest normal square, {name} {mode}"
    one, bins, two = run_fused(handle, case.A, case.B, dtype)
    assert bins == case.bin_rows, f"{what}: rows per bin {bins}, not {case.bin_rows}"
    assert_result(one, case.step.kept, case.bound, rows, dtype, what)
    assert_result(two, case.step.kept, case.bound, rows, dtype, what + " (SpGEMM + prune)")


# ---- 5. a loop that lives in these branches --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_loop_to_convergence(handle, dtype):
    """cliques joined by single edges, run until every row is a single 1.0: hip_gpuRmclIter_device[_f64] with
    maxIter = 1..k against loop64, iteration by iteration; rows pass through the floor branch on the way"""
    M, steps, bounds, floors = rc.loop_case(dtype)
    dM = dev(M, dtype)
    try:
        for k, (s, bound) in enumerate(zip(steps, bounds), 1):
            dOut = hs.gpuRmclIter_device(k, dM, dM, handle)
            try:
                assert dOut.dtype == dtype
                got = dOut.toCpuCSR()
            finally:
                dOut.deviceDispose()
            assert_result(got, s.kept, bound, [("loop", None)] * M.rows, dtype,
                          f"loop {np.dtype(dtype).name}, {k} iterations ({floors[k - 1]} rows in the floor branch)")
        back = dM.toCpuCSR()
    finally:
        dM.deviceDispose()
    assert np.array_equal(back.values.astype(F64), M.values) and np.array_equal(back.colInd, M.colInd)
    assert np.array_equal(got.rowPtr, np.arange(M.rows + 1)) and np.all(np.abs(got.values.astype(F64) - 1.0) <= bounds[-1])
