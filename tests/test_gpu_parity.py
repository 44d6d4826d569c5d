"""GPU (-m gpu): the HIP path, called through the C ABI, against the CPU oracle, the committed golden
vectors made from the real reference, and size-independent properties at the headline size.

Parity rule (BASELINE.json north_star): rowPtr bit-exact, per-row-sorted colInd bit-exact, values within
1e-6 relative (helpers.assert_parity).  The protocol is the reference's own GPU test
(tests/testGpuSpMM.cc:9-46): device SpGEMM -> toCpuCSR -> makeOrdered -> compare with A.spmm(B).
"""
import json
import os

import numpy as np
import pytest

from devcsr import to_hs, unpack
from helpers import DATA, GOLDEN, assert_parity, canonical_arrays, po, random_csr, summarize, synth_csr
from sparse_matrix_with_flops_amd import hipspgemm as hs

pytestmark = pytest.mark.gpu

FX = np.load(os.path.join(GOLDEN, "fixtures.npz"))
SM = np.load(os.path.join(GOLDEN, "synth_small.npz"))
META = json.load(open(os.path.join(GOLDEN, "golden.json")))


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as ge
    ge.build()
    assert hs.device_count() >= 1, "GPU tests need a HIP device (no CPU fallback exists)"
    h = hs.Handle(0)
    yield h
    h.close()


def hip_mul(A, B):
    """host in / host out through hip_CSR_SpMM"""
    hA = to_hs(A)
    return hA.hip_spmm(hA if B is A else to_hs(B))


def test_wave_primitives_selftest(handle):
    handle.selftest()


SQUARE = [n for n in sorted(os.listdir(DATA)) if "nnzC" in META["fixtures"].get(n, {})]


@pytest.mark.parametrize("name", SQUARE)
def test_reference_fixtures_AA(name):
    key = name.replace(".", "_")
    A = unpack(FX, key + "_load")
    assert_parity(hip_mul(A, A), unpack(FX, key + "_AA"), what=name, inputs=(A, A))


@pytest.mark.parametrize("key", ["synth_64_3_2", "synth_512_7_2", "synth_1024_9_4"])
def test_golden_synth_small(key):
    _, m, seed, base = key.split("_")
    A = synth_csr(int(m), int(seed), int(base))
    assert_parity(hip_mul(A, A), unpack(SM, key + "_AA"), what=key)


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_golden_rectangular_unsorted(idx):
    A, B, want = unpack(SM, f"rect{idx}_A"), unpack(SM, f"rect{idx}_B"), unpack(SM, f"rect{idx}_C")
    assert_parity(hip_mul(A, B), want, what=f"rect{idx}", inputs=(A, B))


@pytest.mark.parametrize("key", ["4096_11_2", "32768_13_2", "65536_17_4"])
def test_synth_vs_oracle_and_golden_summary(key):
    g = META["synth"][key]
    A = synth_csr(g["m"], g["seed"], g["base"])
    got = hip_mul(A, A)
    assert_parity(got, po.omp_spmm(A, A), what=key)
    s = summarize(got)
    assert s["nnz"] == g["nnz"] and s["hash"] == g["hash"]
    assert abs(s["sum"] - g["sum"]) <= 1e-6 * abs(g["sum"]) and abs(s["wsum"] - g["wsum"]) <= 1e-6 * abs(g["wsum"])


def test_headline_config_device_resident(handle):
    """BASELINE.json configs[1]: synthetic 262144^2, ~16 nnz/row, seed 42 — full parity vs the oracle, the
    golden summary from the real reference, device-resident API + device row sort."""
    g = META["synth"]["262144_42_2"]
    A = synth_csr(262144, 42, 2)
    dA = to_hs(A).toGpuCSR()
    dC0 = hs.gpuSpMMWrapper(dA, dA, handle)      # first call: big-row bitmaps are rebuilt in the numeric pass
    first = dC0.toCpuCSR()
    dC0.deviceDispose()
    dC = hs.gpuSpMMWrapper(dA, dA, handle)       # second call on the handle: bitmaps saved by the symbolic pass
    st = handle.stats()
    assert st["total_flops"] == g["P"] and st["nnzC"] == g["nnz"] and sum(st["bin_rows"]) == 262144
    raw = dC.toCpuCSR()
    assert np.array_equal(first.rowPtr, raw.rowPtr)
    hs.sort_rows_device(dC, handle)
    srt = dC.toCpuCSR()
    dC.deviceDispose()
    dA.deviceDispose()
    want = po.omp_spmm(A, A)
    assert_parity(raw, want, what="headline raw")
    assert_parity(first, want, what="headline first call")
    # device-side makeOrdered: columns ascending inside every row, same multiset
    cs, vs = canonical_arrays(raw.rowPtr, raw.colInd, raw.values)
    assert np.array_equal(srt.colInd, cs) and np.array_equal(srt.values, vs)
    s = summarize(raw)
    assert s["hash"] == g["hash"] and abs(s["sum"] - g["sum"]) <= 1e-6 * abs(g["sum"])


def test_device_makeOrdered_long_unsorted_rows(handle):
    """hip_csr_sort_rows on an output whose big rows come out of the LDS hash kernel UNSORTED and are longer than the
    4096-entry bitonic tile (n > 262 144 columns: no rank kernel): the per-row radix sort must give exactly
    CSR::makeOrdered's result (columns ascending, values carried along)."""
    A = synth_csr(300000, 5, 2)
    dA = to_hs(A).toGpuCSR()
    dC = hs.gpuSpMMWrapper(dA, dA, handle)
    raw = dC.toCpuCSR()
    lens = np.diff(raw.rowPtr)
    long_rows = np.nonzero(lens > 4096)[0]
    assert len(long_rows) > 100
    unsorted_long = sum(bool(np.any(np.diff(raw.colInd[raw.rowPtr[r]:raw.rowPtr[r + 1]]) < 0)) for r in long_rows[:200])
    assert unsorted_long > 0, "expected unsorted long rows from the hash kernel"
    hs.sort_rows_device(dC, handle)
    srt = dC.toCpuCSR()
    dC.deviceDispose()
    dA.deviceDispose()
    cs, vs = canonical_arrays(raw.rowPtr, raw.colInd, raw.values)
    assert np.array_equal(srt.rowPtr, raw.rowPtr)
    assert np.array_equal(srt.colInd, cs) and np.array_equal(srt.values.view(np.uint32), vs.view(np.uint32))


def test_bench_workload_1m_rows_vs_reference_summary(handle):
    """bench.py's default workload (1 048 576 rows, seed 43; columns exceed the 262 144-column rank kernel, so rows
    above 4096 products take the LDS hash kernel incl. multi-pass rows that park products in HBM) against the summary
    the real reference produced for it: nnz, structure hash (bit-exact), value checksums (1e-6)."""
    g = META["synth"]["1048576_43_2"]
    A = synth_csr(g["m"], g["seed"], g["base"])
    dA = to_hs(A).toGpuCSR()
    dC = hs.gpuSpMMWrapper(dA, dA, handle)
    st = handle.stats()
    assert st["total_flops"] == g["P"] and st["nnzC"] == g["nnz"]
    got = dC.toCpuCSR()
    dC.deviceDispose()
    dA.deviceDispose()
    s = summarize(got)
    assert s["nnz"] == g["nnz"] and s["hash"] == g["hash"]
    assert abs(s["sum"] - g["sum"]) <= 1e-6 * abs(g["sum"]) and abs(s["wsum"] - g["wsum"]) <= 1e-6 * abs(g["wsum"])


def test_config3_1m_rows_32_per_row_vs_reference_summary(handle):
    """BASELINE configs[3] on ONE GPU (the row-sharded form is tests/test_gpu_dist.py + bench.py --gpus N): synthetic
    1 048 576^2, ~32 nnz/row (seed 44, base 4), P = 0.89 G products, against the summary the real reference's
    omp_CSR_SpMM produced (tests/golden/golden_large.json, tests/golden/make_golden_large.py)."""
    import json
    g = json.load(open(os.path.join(GOLDEN, "golden_large.json")))["synth_1048576_44_4"]
    A = synth_csr(g["m"], g["seed"], g["base"])
    assert A.nnz == g["nnzA"]
    dA = to_hs(A).toGpuCSR()
    dC = hs.gpuSpMMWrapper(dA, dA, handle)
    st = handle.stats()
    assert st["total_flops"] == g["P"] and st["nnzC"] == g["nnz"]
    got = dC.toCpuCSR()
    dC.deviceDispose()
    dA.deviceDispose()
    s = summarize(got)
    assert s["nnz"] == g["nnz"] and s["hash"] == g["hash"]
    assert abs(s["sum"] - g["sum"]) <= 1e-6 * abs(g["sum"]) and abs(s["wsum"] - g["wsum"]) <= 1e-6 * abs(g["wsum"])
    # the 8-way flops partition the sharded run would use (arrayEqualPartition64 of the reference)
    flops = po.row_flops(A, A)
    prefix = np.concatenate([[0], np.cumsum(flops)]).astype(np.int64)
    from sparse_matrix_with_flops_amd.dist import equal_partition64
    assert [int(x) for x in equal_partition64(prefix, 8)] == g["partition8"]


def test_config2_web_google_surrogate_full_parity(handle):
    """BASELINE configs[2] by SHAPE (the real web-Google file is in neither container: "surrogate; reference totals
    unpinned"): synth.webgraph_csr -- 916 428 rows, ~5.5 entries per row, skewed in- and out-degree, nnz(C)/P = 0.49, the
    compressive regime of real web graphs that the power-law workloads (nnz(C)/P >= 0.91) never enter: about every second
    product meets a column that is already in its row's table.  Full size, full parity (rowPtr, sorted colInd bit-exact,
    values 1e-6) against the oracle's omp_CSR_SpMM restatement, and against the summary the REAL reference produced for
    the same input (tests/golden/golden_large.json, tests/golden/make_golden_web.py); also the classification (hv)."""
    import json
    g = json.load(open(os.path.join(GOLDEN, "golden_large.json")))["web_surrogate_916428_46"]
    from sparse_matrix_with_flops_amd import synth
    rp, ci, v = synth.webgraph_csr(g["m"], g["seed"])
    A = po.CSRHost(rp, ci, v, g["m"], g["m"])
    assert A.nnz == g["nnzA"]
    dA = to_hs(A).toGpuCSR()
    hv, hv_len, ids, fl, tot = hs.gpuFlopsClassify(dA, dA, handle)
    hs.dev_free(ids)
    hs.dev_free(fl)
    assert tot == g["P"] and [int(x) for x in hv[:hv_len]] == g["hv"][:g["hv_len"]]
    dC = hs.gpuSpMMWrapper(dA, dA, handle)
    st = handle.stats()
    assert st["total_flops"] == g["P"] and st["nnzC"] == g["nnz"]
    assert 0.45 <= st["nnzC"] / st["total_flops"] <= 0.55
    got = dC.toCpuCSR()
    dC.deviceDispose()
    dA.deviceDispose()
    s = summarize(got)
    assert s["nnz"] == g["nnz"] and s["hash"] == g["hash"]
    assert abs(s["sum"] - g["sum"]) <= 1e-6 * abs(g["sum"]) and abs(s["wsum"] - g["wsum"]) <= 1e-6 * abs(g["wsum"])
    want = po.omp_spmm(A, A)
    assert_parity(got, want, what="web-Google surrogate A*A")


@pytest.mark.skipif(not os.environ.get("SPGEMM_WEB_GOOGLE_MTX"), reason="set SPGEMM_WEB_GOOGLE_MTX=/path/to/web-Google.mtx")
def test_config2_web_google_known_totals(handle):
    """BASELINE configs[2]: SuiteSparse web-Google is on neither box; when a copy is supplied by environment variable,
    A*A must reproduce the totals the reference tree records for it (tools/res.txt:1910)."""
    k = META["survey_known_answers"]["res_txt_web_google"]
    A = po.load(os.environ["SPGEMM_WEB_GOOGLE_MTX"], isTrans=False, mode=0)
    assert A.rows == k["N"] and A.nnz == k["nnzA"]
    dA = to_hs(A).toGpuCSR()
    dC = hs.gpuSpMMWrapper(dA, dA, handle)
    st = handle.stats()
    dC.deviceDispose()
    dA.deviceDispose()
    assert st["nnzC"] == k["nnzC"] and 2 * st["total_flops"] == k["flops"]


def test_classify_matches_oracle(handle):
    A = synth_csr(20000, 23, 2)
    dA = to_hs(A).toGpuCSR()
    hv, hv_len, ids, fl, tot = hs.gpuFlopsClassify(dA, dA, handle)
    rowIds = hs.d2h(ids, A.rows, np.int32)
    dflops = hs.d2h(fl, A.rows + 1, np.int32)
    flops = po.row_flops(A, A)
    o_ids, o_scan, o_hv, o_len = po.gpu_classify(flops)
    assert tot == int(flops.sum())
    assert hv == [int(x) for x in o_hv] and hv_len == o_len
    assert sorted(rowIds.tolist()) == list(range(A.rows))
    # same rows in every reference bin (rows of bin b sit at drowIds + hv[b] - 1, gnnz.cuh:27); ascending inside
    for b in range(1, 8):
        lo, hi = max(hv[b] - 1, 0), hv[b + 1] - 1
        mine, theirs = rowIds[lo:hi], o_ids[lo:hi]
        assert np.array_equal(np.sort(mine), np.sort(theirs)), b
    # rows above 4096 products close the array, heaviest size class (power of two) first: the work queue of the
    # block-per-row kernels starts with them
    nbig = int((flops > 4096).sum())
    if nbig:
        cls = np.floor(np.log2(flops[rowIds[-nbig:]])).astype(int)
        assert np.all(flops[rowIds[-nbig:]] > 4096) and np.all(np.diff(cls) <= 0)
    # dflops = scan of the flops in drowIds order
    assert dflops[0] == 0 and np.array_equal(np.diff(dflops.astype(np.int64)), flops[rowIds])
    # binned SpGEMM on that classification == one-shot path == oracle
    dC = hs.sgpuSpMMWrapper(dA, dA, ids, hv, fl, handle)
    got = dC.toCpuCSR()
    dC.deviceDispose()
    hs.dev_free(ids)
    hs.dev_free(fl)
    dA.deviceDispose()
    assert_parity(got, po.omp_spmm(A, A), what="sgpuSpMMWrapper")


def test_scuda_spmm_host_roundtrip(handle):
    A = synth_csr(3000, 31, 4)
    hA = to_hs(A)
    assert_parity(hs.scudaSpMM(hA, hA, handle), po.sequential_spmm(A, A), what="scudaSpMM")


# ---- edge cases the reference's tests / loaders exercise ---------------------------------------
def test_empty_and_degenerate_inputs():
    Z = po.CSRHost(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 0, 0)
    got = hip_mul(Z, Z)
    assert got.rows == 0 and got.nnz == 0 and list(got.rowPtr) == [0]
    E = random_csr(50, 50, 0.0, 1)                       # no entries at all
    got = hip_mul(E, E)
    assert got.nnz == 0 and not got.rowPtr.any()
    S = random_csr(200, 200, 0.01, 2)                    # most rows empty; products hit empty B rows
    assert_parity(hip_mul(S, S), po.sequential_spmm(S, S), what="sparse-empty-rows", inputs=(S, S))
    one = po.CSRHost([0, 1], [0], [3.0], 1, 1)
    got = hip_mul(one, one)
    assert list(got.rowPtr) == [0, 1] and got.values[0] == 9.0


def test_rows_with_entries_but_zero_products():
    # A's columns point only at empty rows of B: flops 0 with nnz(A) > 0
    A = po.CSRHost([0, 2, 3], [1, 2, 1], [1.0, 2.0, 3.0], 2, 3)
    B = po.CSRHost([0, 1, 1, 1], [0], [5.0], 3, 4)
    got = hip_mul(A, B)
    assert got.nnz == 0 and list(got.rowPtr) == [0, 0, 0]


@pytest.mark.parametrize("seed", range(4))
def test_random_rectangular_unsorted(seed):
    rng = np.random.default_rng(100 + seed)
    r, k, c = (int(x) for x in rng.integers(1, 400, size=3))
    A = random_csr(r, k, float(rng.uniform(0.0, 0.2)), seed, sorted_rows=False)
    B = random_csr(k, c, float(rng.uniform(0.0, 0.2)), seed + 50, sorted_rows=False)
    assert_parity(hip_mul(A, B), po.sequential_spmm(A, B), what=f"rand{seed}", inputs=(A, B))


def _rows_csr(rows_cols, ncols, seed, signed=False):
    rng = np.random.default_rng(seed)
    rp = np.zeros(len(rows_cols) + 1, np.int32)
    np.cumsum([len(c) for c in rows_cols], out=rp[1:])
    ci = np.concatenate([np.asarray(c, np.int32) for c in rows_cols]) if len(rows_cols) else np.zeros(0, np.int32)
    v = (rng.random(len(ci)) + 0.5).astype(np.float32)
    if signed:
        v *= rng.choice(np.array([-1.0, 1.0], np.float32), size=len(ci))
    return po.CSRHost(rp, ci, v, len(rows_cols), ncols)


def test_big_rows_multi_window_and_rank_passes():
    """Rows > 4096 products; B wider than one 262144-column LDS window; > 18432 distinct columns in a row."""
    rng = np.random.default_rng(7)
    k, n = 3000, 700000
    B = _rows_csr([np.sort(rng.choice(n, size=int(rng.integers(40, 120)), replace=False)) for _ in range(k)], n, 1)
    A = _rows_csr([rng.choice(k, size=s, replace=False) for s in (400, 90, 1, 0, 700, 64, 65, 2500)], k, 2)
    want = po.sequential_spmm(A, B)
    assert np.diff(want.rowPtr).max() > 18432
    assert_parity(hip_mul(A, B), want, what="big-rows")


def test_big_rows_wider_than_one_symbolic_window():
    """B with 2.5 M columns: the symbolic bitmap kernel covers 1 M columns per window, so rows above 4096 products
    take three windows; the numeric side is the multi-pass LDS hash (one pass, parked passes, and the re-walk fallback).
    The hash kernel takes BH_CAP = 11 264 distinct columns per pass and parks the later classes of up to BH_MAXCLS = 32
    passes, BH_SPILL = 262 144 products in all: the 3900-entry row (some 230 000 products, 15 or more passes) reaches
    the re-walk because its parked products outgrow that buffer, not for its number of classes (that edge, more than
    32 * 11 264 columns, is pinned by tests/test_gpu_edges.py)."""
    rng = np.random.default_rng(17)
    k, n = 4000, 2500000
    B = _rows_csr([np.sort(rng.choice(n, size=int(rng.integers(30, 90)), replace=False)) for _ in range(k)], n, 5)
    A = _rows_csr([rng.choice(k, size=s, replace=False) for s in (120, 300, 0, 1100, 75, 3900)], k, 6)
    want = po.sequential_spmm(A, B)
    assert np.diff(want.rowPtr).max() > 16 * 10240        # 163 840 columns = 15 passes of BH_CAP or more: the parked
                                                          # products outgrow BH_SPILL (16 * 10 240: the former constants)
    assert_parity(hip_mul(A, B), want, what="wide-B big rows")


def test_parking_region_overflow_redoes_the_row():
    """Multi-pass rows park the products of later hash classes in per-class regions sized from the expected class
    size; SPGEMM_BHMARGIN=60 makes every region too small, so each such row must notice the overflow and redo itself
    with one walk per pass.  Same result either way."""
    rng = np.random.default_rng(29)
    k, n = 3000, 600000
    B = _rows_csr([np.sort(rng.choice(n, size=int(rng.integers(40, 100)), replace=False)) for _ in range(k)], n, 7)
    A = _rows_csr([rng.choice(k, size=s, replace=False) for s in (500, 260, 90, 1200)], k, 8)
    want = po.sequential_spmm(A, B)
    assert np.diff(want.rowPtr).max() > 3 * 10240
    os.environ["SPGEMM_BHMARGIN"] = "60"
    try:
        h = hs.Handle(0)                                   # the knob is read when a handle is created
    finally:
        del os.environ["SPGEMM_BHMARGIN"]
    dA, dB = to_hs(A).toGpuCSR(), to_hs(B).toGpuCSR()
    dC = hs.gpuSpMMWrapper(dA, dB, h)
    got = dC.toCpuCSR()
    for d in (dC, dA, dB):
        d.deviceDispose()
    h.close()
    assert_parity(got, want, what="parking overflow -> redo")


def test_long_A_rows_and_empty_B_rows_in_staging():
    """A rows longer than one staging chunk (1024 / 512 / 64 entries) whose B rows are short or empty."""
    rng = np.random.default_rng(11)
    k, n = 6000, 5000
    lens = rng.integers(0, 4, size=k)                     # many empty B rows
    lens[rng.integers(0, k, size=50)] = 300
    B = _rows_csr([np.sort(rng.choice(n, size=int(l), replace=False)) for l in lens], n, 3, signed=True)
    A = _rows_csr([rng.choice(k, size=s, replace=False) for s in (3000, 1500, 700, 130, 66, 20, 5800)], k, 4, signed=True)
    assert_parity(hip_mul(A, B), po.sequential_spmm(A, B), what="long-A-rows", inputs=(A, B))


def test_duplicate_columns_inside_A_and_B_rows():
    """Repeated column indices inside a row of A and inside a row of B (an unsorted, un-deduplicated input): the
    accumulators key on the column, so repeats just add up -- same structure and values as the CPU kernel."""
    rng = np.random.default_rng(5)
    k, n = 2000, 300000
    brows = []
    for _ in range(k):
        c = rng.integers(0, n, size=int(rng.integers(5, 80)))
        brows.append(np.concatenate([c, c[:len(c) // 3]]))                   # a third of the columns twice
    B = _rows_csr(brows, n, 1)
    arows = []
    for s_ in (3, 10, 40, 100, 300, 900, 1800):
        c = rng.choice(k, size=s_, replace=False)
        arows.append(np.concatenate([c, c[:s_ // 4]]))                        # repeated B rows
    arows += [rng.choice(k, size=int(rng.integers(1, 30)), replace=False) for _ in range(500)]
    A = _rows_csr(arows, k, 2)
    want = po.sequential_spmm(A, B)
    assert np.diff(want.rowPtr).max() > 4096
    assert_parity(hip_mul(A, B), want, what="duplicates in A and B rows")


def test_every_bin_boundary():
    """Rows engineered to sit exactly on the flop-bin edges 0,1,2,4,5,16,17,64,65,512,513,4096,4097."""
    edges = [0, 1, 2, 4, 5, 16, 17, 64, 65, 512, 513, 4096, 4097]
    n = 9000
    # B row j has exactly j entries (j = 0..4097 needs k > 4097): use a dictionary of needed lengths
    lens = sorted(set(edges))
    B = _rows_csr([np.arange(l, dtype=np.int32) * 2 % n if l else [] for l in lens], n, 5)
    A = _rows_csr([[lens.index(e)] for e in edges] + [[lens.index(2), lens.index(2)][:1]], len(lens), 6)
    got = hip_mul(A, B)
    want = po.sequential_spmm(A, B)
    assert list(np.diff(want.rowPtr))[:len(edges)] == edges
    assert_parity(got, want, what="bin-edges")


# ---- properties that hold at any size -----------------------------------------------------------
def test_identity_and_scaling_properties_full_size():
    A = synth_csr(262144, 42, 2)
    m = A.rows
    Id = po.CSRHost(np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32), np.ones(m, np.float32), m, m)
    got = hip_mul(A, Id)                                   # A*I == A exactly
    assert np.array_equal(got.rowPtr, A.rowPtr)
    gc, gv = canonical_arrays(got.rowPtr, got.colInd, got.values)
    assert np.array_equal(gc, A.colInd) and np.array_equal(gv, A.values)
    got = hip_mul(Id, A)                                   # I*A == A exactly
    gc, gv = canonical_arrays(got.rowPtr, got.colInd, got.values)
    assert np.array_equal(got.rowPtr, A.rowPtr) and np.array_equal(gc, A.colInd) and np.array_equal(gv, A.values)


def test_scaling_linearity_medium():
    A = synth_csr(16384, 77, 2)
    A2 = po.CSRHost(A.rowPtr, A.colInd, A.values * np.float32(2.0), A.rows, A.cols)
    c1, c2 = hip_mul(A, A), hip_mul(A2, A)
    assert np.array_equal(c1.rowPtr, c2.rowPtr)
    k1, v1 = canonical_arrays(c1.rowPtr, c1.colInd, c1.values)
    k2, v2 = canonical_arrays(c2.rowPtr, c2.colInd, c2.values)
    assert np.array_equal(k1, k2)
    assert np.allclose(v2, 2.0 * v1, rtol=2e-6, atol=0)


def test_error_behaviour():
    A = to_hs(random_csr(5, 7, 0.5, 1))
    with pytest.raises(hs.SpgemmError):
        A.hip_spmm(A)                                      # 5x7 times 5x7: the reference asserts (CSR.cc:60)
    bad = hs.CSR.from_arrays([0, 2, 4], [0, 9, 1, 0], [1, 1, 1, 1], 2, 2)   # column 9 out of range
    with pytest.raises(hs.SpgemmError):
        bad.hip_spmm(bad)
