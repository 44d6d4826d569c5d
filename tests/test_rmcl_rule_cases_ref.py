"""CPU: the rows of rmcl_rule_cases.py do what they claim, on the reference alone.  Every launch the GPU tests of
test_gpu_rmcl_rule_branches.py run is built here (the builder asserts each row's branch, kept set and gap), and every row
is compared with plain_rule of test_rmcl_f64_abi.py, the row rule operation by operation; the float rule of the promotion
rows is compared with the C oracle's restatement of computeThreshold for QValue = float."""
import ctypes as C

import numpy as np
import pytest

import rmcl_rule_cases as rc
from helpers import po
from rmcl_f64_ref import row_rule64
from test_rmcl_f64_abi import plain_rule

DTYPES = [np.float32, np.float64]


def against_plain_rule(rows, what):
    """every row of a launch: threshold, kept positions and values of row_rule64 equal plain_rule's, bit for bit"""
    for r, (kind, c) in enumerate(rows):
        idx, kv, t = plain_rule(c)
        kept, th, _ = row_rule64([0, len(c)], np.arange(len(c)), c)
        assert th[0] == t or len(c) == 0, (what, r, kind)
        assert list(kept.colInd) == idx and list(kept.values) == kv, (what, r, kind)
        if kind.startswith("promotion"):
            continue
        assert rc.branch_of(c * c) == rc.BRANCH[kind], (what, r, kind)
        assert idx == list(np.flatnonzero(rc.expected_keep(kind, c))), (what, r, kind)
        if rc.BRANCH[kind] in ("floor-negative", "floor-small"):
            assert t == 1.0e-7 and 0 < len(idx) < len(c), (what, r, kind)
        if rc.BRANCH[kind] == "cap":
            assert t == max(c * c) < 1.0e-7 and all(c[i] * c[i] == t for i in idx), (what, r, kind)
        if kind in rc.EXACT:
            assert kv == [1.0 / len(idx)] * len(idx), (what, r, kind)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lanes", [16, 64])
def test_prune_launches(dtype, lanes):
    case = rc.PruneCase(rc.PRUNE_LENGTHS[lanes], dtype)
    assert case.lanes == lanes and case.C.rows % (256 // lanes) != 0          # dead rows in the last block take part in the ballots
    kinds = {k for k, _ in case.rows}
    assert kinds == set(rc.KINDS) | {"one", "one-b", "empty"}
    assert case.gap >= 1000.0 * case.bound
    print(f"prune L={lanes} {np.dtype(dtype).name}: {case.C.rows} rows, smallest counted gap {case.gap:.3e}, 1000 * bound {1000 * case.bound:.3e}")
    against_plain_rule(case.rows, f"prune {lanes}")


@pytest.mark.parametrize("name,mode", [(n, m) for n, (_, _, modes) in rc.FUSED_LAUNCHES.items() for m in modes if m != "float-symbolic"])
def test_fused_launches(name, mode):
    lengths, terms, _ = rc.FUSED_LAUNCHES[name]
    case = rc.FusedCase(lengths, rc.MODE_DTYPE[mode], terms)
    kinds = {k for k, _ in case.rows}
    assert kinds >= (set(rc.KINDS) - {"floor-edge"}) | {"one", "one-b", "empty"}
    assert case.gap >= 1000.0 * case.bound and sum(case.bin_rows) == len(case.rows)
    print(f"{name} {mode}: {len(case.rows)} rows, bins {case.bin_rows}, smallest counted gap {case.gap:.3e}, 1000 * bound {1000 * case.bound:.3e}")
    if max(lengths) <= 6145:                                                   # (a Python loop per entry: the longest row is left to the builder)
        against_plain_rule(case.rows, name)


def test_floor_edge_row_is_in_every_short_launch():
    """the row that tells a floor of 1e-7 from one of 1.1e-7 runs wherever 1000 * bound allows its gap of 0.0514"""
    for dtype in DTYPES:
        for name, (lengths, terms, modes) in rc.FUSED_LAUNCHES.items():
            if ("double" if dtype is np.float64 else "float") not in modes:
                continue
            bound = rc.step_bound(terms, max(lengths), rc.UNIT[dtype])
            assert ("floor-edge" in rc.kinds_at(max(lengths), bound)) == (1000.0 * bound <= rc.FLOOR_EDGE_GAP)
    short = [n for n, (l, t, _) in rc.FUSED_LAUNCHES.items() if "floor-edge" in rc.kinds_at(max(l), rc.step_bound(t, max(l), 2.0 ** -24))]
    assert short == ["g16-list", "g16-hashed", "wave-65"]
    v = (85 * 2.0 ** -18) ** 2
    assert 1.0e-7 < v < 1.1e-7 and np.float32(v) == v


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("below", [False, True])
def test_domain_edge_rows(dtype, below):
    rows = rc.domain_rows((5, 16, 65), dtype, below)
    tiny = np.finfo(dtype).tiny
    for kind, c in rows:
        if len(c):
            assert (c * c).max() == (tiny / 4 if below else tiny) and np.array_equal(c.astype(dtype).astype(np.float64), c)
    rc.check_rows(rows, rc.step_bound(2, 65, rc.UNIT[dtype]), "domain", exact32=False)
    against_plain_rule(rows, "domain")
    one = dtype(rows[2][1][0])
    with np.errstate(over="ignore"):
        inv = dtype(1) / (one * one)
    assert np.isinf(inv) == below                                              # the reciprocal of the kept sum leaves the type one step lower


@pytest.mark.parametrize("which", ["kept", "dropped"])
def test_promotion_rows(which):
    c, probe, tf, td = rc.promotion_row(which)
    v = c * c
    s = float(np.cumsum(v)[-1])
    avg, mx = np.float32(s / 8), np.float32(v.max())
    assert float(avg) == s / 8 and np.array_equal(v.astype(np.float32).astype(np.float64), v)      # nothing a float kernel adds is rounded
    assert tf == float(rc.threshold_f32(avg, mx)) and td == rc.threshold_all_f64(avg, mx) and tf != td
    ulp = float(np.spacing(np.float32(tf)))
    assert min(tf, td) < v[probe] < max(tf, td) and abs(v[probe] - tf) >= 1000 * ulp
    assert (v[probe] >= tf) == (which == "kept") and (v[probe] >= td) == (which != "kept")
    print(f"{which}: float rule {tf!r}, all-double {td!r}, all-float {float(rc.threshold_all_f32(avg, mx))!r}, "
          f"probe {v[probe]!r} is {(v[probe] - tf) / ulp:.0f} ulps from the float rule's threshold")
    # the double rule is plain_rule's; the float rule is the C oracle's (computeThreshold with QValue = float)
    idx, _, t = plain_rule(c)
    assert t == td and (probe in idx) == (which != "kept")
    rp = np.array([0, 8], np.int32)
    ci = np.arange(8, dtype=np.int32)
    val = c.astype(np.float32)
    n = po.lib().oracle_rmcl_prune_compact(C.c_int(1), po._ip(rp), po._ip(ci), po._fp(val))
    assert (probe in ci[:n].tolist()) == (which == "kept") and n == (8 if which == "kept" else 7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_loop_case(dtype):
    M, steps, bounds, floors = rc.loop_case(dtype)
    assert len(steps) <= rc.LOOP_MAX_ITERS and max(floors) > 0
    print(f"{np.dtype(dtype).name}: {M.rows} rows, nnz per iteration {[s.kept.nnz for s in steps]}, floor rows {floors}, "
          f"gap / (1000 * bound) per iteration {[round(float(s.gap.min() / (1000 * b)), 2) for s, b in zip(steps, bounds)]}")
    s = steps[max(range(len(floors)), key=floors.__getitem__)]
    p = s.product
    against_plain_rule([("promotion", p.values[p.rowPtr[r]:p.rowPtr[r + 1]]) for r in range(M.rows)], "loop")
