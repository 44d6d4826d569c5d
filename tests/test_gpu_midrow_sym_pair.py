"""GPU (-m gpu): the symbolic kernel of bin 6 (rows of 513-2048 products) that takes two light rows at a time, k_sym_midpair:
all waves of a block (four, or two with SPGEMM_SP_WAVES=2) on a row of 1025-2048 products with the whole table of 4096 keys,
two rows of 513-1024 products side by side on half the waves and half the table each, one statically scheduled launch over
both layout slots.  It counts the rows' distinct columns and logs their re-hits for the
direct numeric kernels exactly as the four-wave kernel does, so every case is judged three ways: the product against the
CPU oracle (rowPtr, per-row sorted columns and the integer values, all exact); the rows each NUMERIC kernel took
(Handle.midrow_paths()), which follow from the logged counts alone (at most 448 re-hits: the wave kernel, at most 896: the
four-wave kernel, more: the hash kernel); and the rows the new kernel processed (Handle.midrow_sym_paths()).  The kernel
is opt-in (SPGEMM_SYM_PAIR=1); every case also runs with SPGEMM_SYM_PAIR=0 and must give the same bits and the same paths.

The inputs are built as in test_gpu_midrow_wave (B of disjoint rows: every re-hit is planted, and the planted count is
checked on the CPU as products minus the oracle's row length before anything is asserted about the GPU).  A fresh handle
per case, three products on it, the second and the third judged.  SPGEMM_MD_MINROWS=1 and SPGEMM_MW_MINROWS=1 as there, and
SPGEMM_SP_MINROWS=0: k_sym_midpair runs from the handle's first product (otherwise it waits for a previous product of the
same shape with 32 x CUs rows in the bin), so the first product sizes the log from this kernel's own reservations.
"""
import os

import numpy as np
import pytest

from helpers import assert_parity, po
from sparse_matrix_with_flops_amd import hipspgemm as hs
from test_gpu_midrow_wave import CAP, N, WCAP, Bld, _bits, _flops, _mixed, _mul, _split

pytestmark = pytest.mark.gpu

PATH_KEYS = ("rows", "direct", "fallback", "wave", "multiwave", "logged")


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()
    assert hs.device_count() >= 1, "GPU tests need a HIP device (no CPU fallback exists)"


@pytest.fixture(params=(4, 2), autouse=True)
def _waves(request):
    """every case with blocks of four waves (two per light row; the default) and of two (one per light row)"""
    os.environ["SPGEMM_SP_WAVES"] = str(request.param)
    yield request.param
    del os.environ["SPGEMM_SP_WAVES"]


def _handle(**env):
    """a fresh handle; the SPGEMM_* knobs are read when it is created"""
    env.setdefault("SPGEMM_MD_MINROWS", 1)
    env.setdefault("SPGEMM_MW_MINROWS", 1)
    env.setdefault("SPGEMM_SP_MINROWS", 0)
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return hs.Handle(0)
    finally:
        for k in env:
            del os.environ[k]


_ORACLE = {}


def _plan(case, A, B, planted):
    """the oracle's product, computed once per case and left alone, and the products of every row; the planted re-hits are
    checked against the two"""
    if case not in _ORACLE:
        want = po.omp_spmm(A, B)
        f = _flops(A, B)
        mid = (f > 512) & (f <= 4096)
        assert np.array_equal((f - np.diff(np.asarray(want.rowPtr, np.int64)))[mid], planted[mid]), f"{case}: planted re-hits"
        _ORACLE[case] = (want, f)
    return _ORACLE[case]


def _arm(case, A, B, planted, pair, split, env):
    """three products on a fresh handle with SPGEMM_SYM_PAIR=pair; returns (third result, its paths)"""
    want, f = _plan(case, A, B, planted)
    n6 = int(((f > 512) & (f <= 2048)).sum())
    nmid = int(((f > 512) & (f <= 4096)).sum())
    h = _handle(SPGEMM_SYM_PAIR=pair, **env)
    try:
        for call in ("first", "second", "third"):
            got, p = _mul(h, A, B)
            what = f"{case}, SPGEMM_SYM_PAIR={pair} ({call} call)"
            assert_parity(got, want, what=what)
            assert _bits(got) == _bits(want), what           # integer values: any order of summation is exact
            sp = h.midrow_sym_paths()
            assert sp == ({"pair": n6, "multiwave": 0} if pair else {"pair": 0, "multiwave": n6}), f"{what}: {sp}"
            assert p["rows"] == nmid, f"{what}: {p}"
            if call == "first":
                assert (p["direct"], p["wave"], p["multiwave"]) == (0, 0, 0), f"{what}: {p}"    # no log yet
                continue
            assert p["direct"] + p["fallback"] == nmid, f"{what}: {p}"
            if split:
                assert (p["wave"], p["multiwave"], p["fallback"]) == _split(f, planted), f"{what}: {p}"
                assert p["logged"] == int(planted[(f > 512) & (f <= 4096) & (planted <= CAP)].sum()), f"{what}: {p}"
        return got, p
    finally:
        h.close()


def run(case, A, B, planted, split=True, same_paths=True, **env):
    """both arms; k_sym_midpair's result and paths are returned after they are compared with the four-wave kernel's"""
    new, p = _arm(case, A, B, planted, 1, split, env)
    old, q = _arm(case, A, B, planted, 0, split, env)
    assert _bits(new) == _bits(old), case
    if same_paths:
        assert [p[k] for k in PATH_KEYS] == [q[k] for k in PATH_KEYS], f"{case}: {p} against {q}"
    return new, p


# ---- the kernel's hash, on the CPU ----------------------------------------------------------------------------------------
def _slot(c, size):
    """slot of column c in a table of `size` (a power of two) keys: the top bits of the multiplicative hash"""
    return ((int(c) * 2654435761) & 0xffffffff) >> (32 - int(size).bit_length() + 1)


# ---- the inputs -----------------------------------------------------------------------------------------------------------
def test_product_counts():
    """the ends of the bin and of its two modes: 513 and 1024 products (half a block each, 2048 keys), 1025 and 2048 (the whole
    block, 4096 keys); no re-hit (1024 and 2048 distinct columns: both tables at load 0.5), one, a few dozen; long entries (64
    products each) and flattened ones (8 each: up to 256 A entries, four groups of the walk)"""
    b = Bld(N, 1)
    for products in (513, 1024, 1025, 2048):
        for r in (0, 1, 40):
            b.add(64, products, r)
            b.add(8, products, r)
    A, B, planted = b.finish(2)
    f = _flops(A, B)
    assert sorted(set(f.tolist())) == [513, 1024, 1025, 2048]
    _, p = run("products", A, B, planted)
    assert (p["wave"], p["multiwave"], p["fallback"]) == (24, 0, 0), p


def test_colliding_columns():
    """light rows whose 600-640 columns all start their probes in 16 of the 2048 slots of the wave's half of the table, heavy
    rows whose 1050 columns start in 32 of 4096 (the low bits of the slot number are free, the high ones all zero): probe
    chains dozens to hundreds of steps long, which must neither leave the (half) table nor lose a column.  As one B row (one
    A entry, products gathered in trips of 8 rounds) and as B rows of 8 columns"""
    pool = [c for c in range(N) if _slot(c, 4096) < 32][:1050]
    assert len(pool) == 1050
    assert len({_slot(c, 2048) for c in pool[:640]}) <= 16 and len({_slot(c, 4096) for c in pool}) <= 32
    b = Bld(N, 3, reserve=pool)
    one = b._new(("coll", "one"), pool[:600])
    eights = [b._new(("coll", "eight", i), pool[8 * i:8 * i + 8]) for i in range(80)]
    more = b._new(("coll", "more"), pool[600:])                         # 450 columns
    b.row([one], rehits=0)                                              # 600 products in 16 slots of 2048
    b.row(eights, rehits=0)                                             # 640
    b.row([one], eights[:5], rehits=40)                                 # 640, 40 re-hits
    b.row([one], [more], rehits=0)                                      # 1050 products: the whole block, 4096 keys
    b.row(eights, [more], rehits=40)                                    # 1090 products, columns 600-639 twice
    b.row([one], eights, [more], rehits=640)                            # 1690 products
    A, B, planted = b.finish(4)
    f = _flops(A, B)
    assert f.tolist() == [600, 640, 640, 1050, 1090, 1690]
    _, p = run("collide", A, B, planted)
    assert (p["wave"], p["multiwave"], p["fallback"]) == (5, 1, 0), p


def test_a_entries_per_row():
    """1 A entry (a single B row of 600, 1500, 2048 columns), 64 and 65 (one and two staged groups), several hundred
    B rows of 8 columns, and heavy rows with long and short entries mixed"""
    b = Bld(N, 5)
    for L in (600, 1500, 2048):
        b.row([b.long[L]], rehits=0)
    b.row([b.long[600]], b.singles(b.brows[b.long[600]][:30]), rehits=30)
    b.row([b.long[70]], b.base[8][:63], rehits=0)                                      # 64 entries, 574 products
    b.row([b.long[70]], b.base[8][:62], [b.copy(b.base[8][0])], rehits=8)              # 64 entries, one a copy
    b.row([b.long[70]], b.base[8][:64], rehits=0)                                      # 65 entries
    b.row([b.long[70], b.copy(b.long[70])], b.base[8][:63], rehits=70)                 # 65 entries, the long one twice
    b.row([b.long[70]], b.base[8][:127], rehits=0)                                     # 128 entries, 1086 products: heavy
    b.row([b.long[70]], b.base[8][:128], rehits=0)                                     # 129 entries: a second chunk of one
    b.row([b.long[600]], b.base[8][:100], b.singles(b.brows[b.long[600]][100:200]), rehits=100)   # 201 entries, heavy
    b.row(b.base[8][:200], rehits=0)                                                   # 200 entries, 1600 products
    b.row(b.base[8][:256], rehits=0)                                                   # 256 entries, 2048 products
    b.row(b.base[8][:120], rehits=0)                                                   # 120 entries, 960 products: light
    b.row(b.base[8][:193], b.singles(b.brows[64 + 192][:7]), [b.long[70]], rehits=7)   # 201 entries
    b.row(b.base[64][:2], [b.long[1500]], b.base[8][:40], [b.copy(b.base[64][1])], rehits=64)     # 2012 products
    A, B, planted = b.finish(6)
    f = _flops(A, B)
    assert f.min() > 512 and f.max() <= 2048
    _, p = run("entries", A, B, planted)
    assert (p["wave"], p["fallback"]) == (A.rows, 0), p


REHITS = (0, 1, 448, 449, 896, 897)


def test_rehits_per_row():
    """0 and 1 re-hits; 448 and 449, 896 and 897: the caps the two direct numeric kernels read from the log's counts (897 is
    one above the cap a row may log, which sends it to the fallback list), in both modes; and one column hit 600 times"""
    b = Bld(N, 7)
    for r in REHITS:
        b.add(64, 2000, r)
        b.add(8, 2040, r, onecol=r % 2 == 1)
        b.add(64, 1000 + (r > 400) * 24, r)
    c1 = int(b.brows[0][0])
    b.row(b.base[64][:8], [b._new(("same", i), [c1]) for i in range(600)], rehits=600)     # 1112 products
    b.row(b.base[64][:1], [b._new(("same", i), [c1]) for i in range(600)], rehits=600)     # 664 products
    A, B, planted = b.finish(8)
    _, p = run("rehits", A, B, planted)
    assert (p["wave"], p["multiwave"], p["fallback"]) == (9, 6 + 2, 3), p


def test_only_heavy_only_light_few_rows():
    """a bin of heavy rows only, of light rows only, and of five rows (fewer than the 8 blocks of the smallest grid: XCD shares
    of none and of one row)"""
    for case, shapes in (("heavy", [(64, 1100 + 7 * i, i % 50) for i in range(40)]),
                         ("light", [(8, 520 + 7 * i, i % 50) for i in range(40)]),
                         ("five", [(64, 700, 3), (8, 1500, 0), (64, 2048, 20), (8, 513, 1), (64, 1025, 0)])):
        b = Bld(N, 9)
        for L, products, r in shapes:
            b.add(L, products, r)
        A, B, planted = b.finish(10)
        _, p = run(case, A, B, planted)
        assert (p["wave"], p["fallback"]) == (A.rows, 0), (case, p)


def test_more_rows_than_waves():
    """SPGEMM_SP_PERCU=1 caps the grid at one block per CU (32 per XCD on a 256-CU device): with 37-38 heavy and 75 light
    rows in every XCD's share the blocks stride -- a second trip in both modes, the last light trip partly filled and with
    an odd row (one wave of a block idle) -- and every wave passes its chunk of the log on from row to row"""
    b = Bld(N, 11)
    for i in range(900):
        if i % 3 == 0:
            b.add(64 if i % 2 else 8, 1030 + i, (0, 5, 300, 460, 897)[i % 5])
        else:
            b.add(8 if i % 4 else 64, 520 + i % 500, (0, 3, 120, 449)[i % 4] if 520 + i % 500 > 600 else i % 2)
    A, B, planted = b.finish(12)
    f = _flops(A, B)
    assert int((f > 1024).sum()) == 300 and int((f <= 1024).sum()) == 600 and f.min() > 512 and f.max() <= 2048
    w, m, fb = _split(f, planted)
    assert min(w, m, fb) >= 50, (w, m, fb)
    run("stride", A, B, planted, SPGEMM_SP_PERCU=1)


def test_mixed_all_bins():
    """bin 6 beside non-empty bins 5, 7 and 8 (the input of test_gpu_midrow_wave: wave, four-wave and fallback rows
    alternating in both layout slots, hub columns)"""
    A, B, planted = _mixed()
    f = _flops(A, B)
    for lo, hi in ((64, 512), (512, 1024), (1024, 2048), (2048, 4096), (4096, 1 << 30)):
        assert ((f > lo) & (f <= hi)).any(), (lo, hi)
    run("mixed", A, B, planted)


def test_log_space_runs_out_mid_launch():
    """SPGEMM_MRLOG leaves the log two chunks of 4096 ints and every block (heavy rows) or wave (light rows) with a row
    reserves one: two reservers find room, the others' rows fall back in the same launch, and the product does not change.
    Which rows find room depends on the order of the reservations, so the two kernels' paths are not compared here"""
    b = Bld(N, 16)
    for i in range(60):
        b.add(64 if i % 2 else 8, (1800 if i % 3 else 900) + i, 300)
    A, B, planted = b.finish(17)
    _, p = run("logfull", A, B, planted, split=False, same_paths=False, SPGEMM_MRLOG=8192)
    assert p["capacity"] == 8192 and p["multiwave"] == 0, p
    assert 1 <= p["wave"] <= 26 and p["wave"] + p["fallback"] == 60 and p["logged"] == 300 * p["wave"], p
