"""Rows that put the R-MCL row rule into each of its branches, for every kernel that applies it (no GPU import).

The rule (rmcl_f64_ref.py): v = c*c, mx, avg, f = 0.9*avg*(1 - 2*(mx - avg)), th = f raised to 1e-7 then lowered to mx,
keep v >= th, kept v / sum(kept v).  Branches, named by what the reference does to f:
  floor-negative   f < 0 (mx - avg > 0.5: one dominant entry, the converged state of an MCL run), th == 1e-7
  floor-small      0 < f <= 1e-7 < mx, th == 1e-7
  cap              mx < 1e-7, th == mx: only the entries equal to the maximum survive, and only by equality
  formula          th == f (here only the uniform row of large squares, whose avg equals its mx exactly)

Arithmetic.  Every stored value is a small integer times a power of two and exact in float32, so both value types see
the same inputs; every square is exact, and so are every maximum and every sum of equal squares (n * 2^-k with
n < 2^24, whatever the order of the partial sums).  In the fused form every product entry is the sum of `terms` equal
products a*b with a = 0.5/terms and b = 2c, terms a power of two: exact as well.  So the rows of a kind in EXACT come out
bit for bit: a `cap` row keeps k bit-identical maxima v, their sum k*v is exact and v/(k*v) = 1/k correctly rounded; a
uniform row of n entries has sum n*v, avg = v = mx exactly, keeps everything and gives 1/n correctly rounded.  The
reciprocal form v * (1/ks) of the fused epilogues gives the same bits there: v is a power of two, so 1/(k*v) is the rounded
1/k scaled by a power of two and the product with v only undoes the scaling.

Row kinds (functions of the row length n >= 3; a launch also holds two one-entry rows, which must become 1.0 exactly, and
an empty row, which must stay empty):
  dominant         0.9375 at position 0, then 2^-10 / 2^-13 / 2^-4 by position mod 3: squares 0.879, 9.5e-7 (kept),
                   1.49e-8 (dropped, gap 0.851), 3.9e-3 (kept).  floor-negative.
  small-floor      2^-11 at every fourth position, 2^-13 elsewhere: squares 2.38e-7 (kept, gap 1.38) and 1.49e-8
                   (dropped, gap 0.851); 0.9*avg <= 1e-7 because at most 0.43 n entries may be high.  floor-small.
  floor-edge       small-floor with 85 * 2^-18 at position 1: its square 7225 * 2^-36 = 1.0514e-7 is kept with gap
                   0.0514 -- it tells a floor of 1e-7 from one of 1.1e-7.  Only where 1000 * bound <= 0.0514.
  cap-one          2^-12 at position 0, 2^-14 elsewhere: mx = 2^-24 = 5.96e-8, the others mx/16 (gap 0.9375).
  cap-three        the same with three maxima: positions 0, n-1 and the first position of the second lane group
                   (64, or 16 in a shorter row, or the middle of one shorter still).
  uniform-high     all 2^-3: th = 0.9 v < v, formula branch, everything kept.
  uniform-low      all 2^-12: squares 5.96e-8 < 1e-7, th == mx == every entry, everything kept by equality.
  signs-and-zeros  dominant with every fifth entry negated and every seventh (from position 3) an explicit 0.0: the kept
                   set and values are those of the absolute values, the zeros are dropped (gap 1).

Preconditions, asserted here on the reference alone (check_rows): every row is in the branch it claims and keeps what
this text says; every entry has gap |v - th| / th >= 1000 * step_bound(N, n, u), except the entries whose equality with
th (or whose survival) follows from identical input bits: the maxima of a cap row and the entries of a uniform row."""
import numpy as np

from f64ref import Host64
from rmcl_f64_ref import row_rule64, step64, step_bound

UNIT = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
FLOOR = 1.0e-7
KINDS = ("dominant", "small-floor", "floor-edge", "cap-one", "cap-three", "uniform-high", "uniform-low", "signs-and-zeros")
BRANCH = {"dominant": "floor-negative", "small-floor": "floor-small", "floor-edge": "floor-small", "cap-one": "cap",
          "cap-three": "cap", "uniform-high": "formula", "uniform-low": "cap", "signs-and-zeros": "floor-negative",
          "one": "formula", "one-b": "formula", "one-low": "cap", "empty": "empty"}
EXACT = ("cap-one", "cap-three", "uniform-high", "uniform-low", "one", "one-b", "one-low")       # results known bit for bit
# one-entry rows: v / v is 1.0 for every v; v * (1 / v) with a rounded reciprocal is not for the squares of these two
# (11/64 in float, 7/64 in double)
ONE_ENTRY = {"one": 11 / 64, "one-b": 7 / 64}
FLOOR_EDGE_GAP = 7225 * 2.0 ** -36 / FLOOR - 1.0                           # 0.0514


def cap_positions(n):
    third = 64 if n > 65 else 16 if n > 17 else n // 2
    return sorted({0, n - 1, third})


def row_values(kind, n):
    """the stored values c of one row (float64 holding numbers exact in float32)"""
    i = np.arange(n)
    if kind in ONE_ENTRY:
        return np.array([ONE_ENTRY[kind]])
    if kind == "empty":
        return np.zeros(0)
    assert n >= 3, "the row kinds need three entries"
    if kind in ("dominant", "signs-and-zeros"):
        c = np.choose(i % 3, [2.0 ** -4, 2.0 ** -10, 2.0 ** -13])
        c[0] = 0.9375
        if kind == "signs-and-zeros":
            c[i % 5 == 4] *= -1.0
            c[(i % 7 == 3)] = 0.0
        return c
    if kind in ("small-floor", "floor-edge"):
        c = np.where(i % 4 == 0, 2.0 ** -11, 2.0 ** -13)
        if kind == "floor-edge":
            c[1] = 85 * 2.0 ** -18
        return c
    if kind in ("cap-one", "cap-three"):
        c = np.full(n, 2.0 ** -14)
        c[[0] if kind == "cap-one" else cap_positions(n)] = 2.0 ** -12
        return c
    if kind == "uniform-high":
        return np.full(n, 2.0 ** -3)
    if kind == "uniform-low":
        return np.full(n, 2.0 ** -12)
    raise KeyError(kind)


def kinds_at(n, bound):
    """the kinds a launch whose value bound is `bound` holds at row length n"""
    return [k for k in KINDS if k != "floor-edge" or 1000.0 * bound <= FLOOR_EDGE_GAP]


def branch_of(v):
    """the branch the reference takes on the squares v of one row, evaluated like threshold64"""
    if len(v) == 0:
        return "empty"
    mx = max(0.0, float(v.max()))
    avg = float(np.cumsum(v)[-1]) / len(v)
    f = 0.90 * avg * (1 - 2 * (mx - avg))
    if mx < FLOOR:
        return "cap"
    if f < 0:
        return "floor-negative"
    if f <= FLOOR:
        return "floor-small"
    return "formula"


def tie_mask(kind, c):
    """entries left out of the gap: equal to th, or kept, by identical input bits alone"""
    v = c * c
    if kind in ("cap-one", "cap-three"):
        return v == v.max()
    if kind in ("uniform-high", "uniform-low", "one", "one-b", "one-low"):
        return np.ones(len(c), bool)
    return np.zeros(len(c), bool)


def expected_keep(kind, c):
    """what the text above says the row keeps"""
    v = c * c
    if kind in ("dominant", "signs-and-zeros", "small-floor", "floor-edge"):
        return v >= FLOOR
    if kind in ("cap-one", "cap-three"):
        return v == v.max()
    return np.ones(len(c), bool)


def check_rows(rows, bound, what="", exact32=True):
    """rows: [(kind, values)].  Branch, kept set and gap of every row on the reference alone -> smallest counted gap"""
    worst = np.inf
    for r, (kind, c) in enumerate(rows):
        n = len(c)
        v = c * c
        if kind.startswith("promotion"):                                         # checked by promotion_row itself
            continue
        assert not exact32 or np.array_equal(c.astype(np.float32).astype(np.float64), c), f"{what} row {r} {kind}: not exact in float32"
        assert branch_of(v) == BRANCH[kind], f"{what} row {r} {kind} n={n}: branch {branch_of(v)}, not {BRANCH[kind]}"
        kept, th, _ = row_rule64([0, n], np.arange(n), c)
        if n == 0:
            assert kept.nnz == 0
            continue
        th = float(th[0])
        want = expected_keep(kind, c)
        assert np.array_equal(kept.colInd, np.flatnonzero(want)), f"{what} row {r} {kind} n={n}: kept set"
        if BRANCH[kind] in ("floor-negative", "floor-small"):
            assert th == FLOOR and 0 < kept.nnz < n, f"{what} row {r} {kind} n={n}: th {th!r}, kept {kept.nnz}"
        if BRANCH[kind] == "cap":
            assert th == v.max() < FLOOR, f"{what} row {r} {kind} n={n}: th {th!r}"
            assert kept.nnz == {"cap-one": 1, "cap-three": len(cap_positions(n)), "uniform-low": n, "one-low": 1}[kind]
            if kind not in ("uniform-low", "one-low"):
                assert np.all(v[~want] <= v.max() / 4)
        if kind in EXACT:
            assert np.array_equal(kept.values, np.full(kept.nnz, 1.0 / kept.nnz)), f"{what} row {r} {kind}: reference values"
        tie = tie_mask(kind, c)
        assert np.all(want[tie]), "an entry left out of the gap is not kept"
        if kind in ("cap-one", "cap-three", "uniform-low", "one-low"):
            assert np.all(v[tie] == th)                                          # equality with th by identical bits
        g = np.abs(v[~tie] - th) / th
        if len(g):
            worst = min(worst, float(g.min()))
            assert g.min() >= 1000.0 * bound, f"{what} row {r} {kind} n={n}: gap {g.min():.3e} < 1000 * bound {bound:.3e}"
    return worst


def launch_rows(lengths, bound):
    """every kind at every length of a launch (length 1: the one-entry row), an empty row behind the first row"""
    rows = []
    for n in lengths:
        if n == 0:
            rows.append(("empty", row_values("empty", 0)))
        elif n == 1:
            rows += [("one", row_values("one", 1)), ("one-b", row_values("one-b", 1))]
        else:
            rows += [(k, row_values(k, n)) for k in kinds_at(n, bound)]
    if not any(k == "one" for k, _ in rows):
        rows.insert(1, ("one", row_values("one", 1)))
        rows.insert(3, ("one-b", row_values("one-b", 1)))
    if not any(k == "empty" for k, _ in rows):
        rows.insert(1, ("empty", row_values("empty", 0)))
    return rows


# ---- the launches, shared by the CPU test of the preconditions and the GPU tests --------------------------------------------
# hip_rmcl_prune[_n][_f64]: lanes per row -> row lengths (16 lanes while nnz < 96 * m, asserted by the tests)
PRUNE_LENGTHS = {16: (1, 16, 17, 33), 64: (64, 65, 257)}
# the fused step: name -> (row lengths, terms per product entry, the modes that run it).  Modes: "float" (rows sized by
# their products, every row hashed and its distinct columns counted by the epilogue), "float-symbolic"
# (SPGEMM_RMCL_SYMBOLIC: rows without repeated columns staged as plain lists) and "double" (always with the symbolic pass).
ALL_MODES = ("float", "float-symbolic", "double")
FUSED_LAUNCHES = {
    "g16-list": ((15, 16, 17, 64), 1, ALL_MODES),          # prune_emit_group<16>, both table sizes
    "g16-hashed": ((7, 8, 9, 32), 2, ALL_MODES),           # ... 14, 16, 18 and 64 products on half as many columns
    "wave-65": ((65,), 1, ALL_MODES),                      # float: prune_emit_group<64>; double: k_num64_rows from here on
    "wave-512": ((512,), 1, ALL_MODES),
    "blocks": ((513, 2048, 2049, 4096), 1, ALL_MODES),     # float: prune_emit_block<4 | 8 waves, WaveSegments>; double: BlockStrided
    "over-4096": ((4097,), 1, ALL_MODES),                  # float: k_rmcl_fix_rows<float>; double: the 8192-slot table, one pass
    "fix-513x16": ((513,), 16, ("float", "float-symbolic")),   # k_rmcl_fix_rows<float> on a 513-entry row of 8208 products
    "fix-6145": ((6145,), 1, ("double",)),                 # k_rmcl_fix_rows<double>: past the last one-pass length, 6144
    "fix-65537": ((65537,), 1, ("double",)),               # ... and past 65536, through the device-memory table
}
F64_LDS_MAXL = 6144
MODE_DTYPE = {"float": np.float32, "float-symbolic": np.float32, "double": np.float64}


def launch_uses_fix_rows(name, mode):
    lengths, terms, _ = FUSED_LAUNCHES[name]
    return all(l * terms > 4096 for l in lengths) if mode != "double" else all(l > F64_LDS_MAXL for l in lengths)


# ---- the domain edge of the reciprocal ---------------------------------------------------------------------------------------
def domain_rows(lengths, dtype, below=False):
    """cap-one and uniform rows (and a one-entry row) scaled so that the largest square is the smallest normal number of
    dtype, 2^-126 or 2^-1022 -- or, below, a quarter of it, a subnormal number.  The kept sum of the cap-one and one-entry
    rows is that square: its reciprocal 2^126 (2^1022) is the last power of two of the type, and 2^128 (2^1024) is not one."""
    c = 2.0 ** -(63 if dtype is np.float32 else 511) * (0.5 if below else 1.0)
    rows = []
    for n in lengths:
        if n < 3:
            continue
        one = np.full(n, c / 4)
        one[0] = c
        rows += [("cap-one", one), ("uniform-low", np.full(n, c))]
    rows.insert(1, ("one-low", np.array([c])))
    rows.insert(1, ("empty", np.zeros(0)))
    return rows


def columns(n, ncols):
    """n distinct columns, not in ascending order"""
    assert ncols >= n and ncols % 5 != 0
    return ((np.arange(n, dtype=np.int64) * 5 + 1) % ncols).astype(np.int32)


def width(rows):
    w = max(7, max(len(c) for _, c in rows))
    return w + (w % 5 == 0)


class PruneCase:
    """a C for hip_rmcl_prune[_n][_f64]: rows as stored values, the reference result, the value bound.  rows: the rows
    themselves in place of every kind at every length"""

    def __init__(self, lengths, dtype, rows=None, exact32=True):
        self.dtype = dtype
        n = max(lengths) if rows is None else max(len(c) for _, c in rows)
        self.bound = step_bound(0, n, UNIT[dtype])
        self.rows = launch_rows(lengths, self.bound) if rows is None else rows
        self.gap = check_rows(self.rows, self.bound, f"prune {lengths}", exact32)
        w = width(self.rows)
        rp = np.zeros(len(self.rows) + 1, np.int32)
        np.cumsum([len(c) for _, c in self.rows], out=rp[1:])
        ci = np.concatenate([columns(len(c), w) for _, c in self.rows])
        self.C = Host64(rp, ci, np.concatenate([c for _, c in self.rows]), len(self.rows), w)
        self.want, self.th, _ = row_rule64(self.C.rowPtr, self.C.colInd, self.C.values)
        self.lanes = 64 if self.C.nnz >= 96 * self.C.rows else 16               # the form the library picks (row_lanes)


class FusedCase:
    """A * B whose product rows are the rows of the launch, each product entry the sum of `terms` equal products (terms a
    power of two): a = 0.5 / terms, b = 2 c.  bin_rows: the rows per bin of product counts the library must report."""
    BIN_EDGES = [0, 1, 4, 16, 64, 512, 2048, 4096]                              # spgemm_device.hpp bin_of: the last product count of bins 0..7

    def __init__(self, lengths, dtype, terms=1, rows=None, exact32=True):
        assert terms & (terms - 1) == 0
        self.dtype, self.terms = dtype, terms
        n = max(lengths) if rows is None else max(len(c) for _, c in rows)
        self.bound = step_bound(terms, n, UNIT[dtype])
        self.rows = launch_rows(lengths, self.bound) if rows is None else rows
        self.gap = check_rows(self.rows, self.bound, f"fused {lengths} x {terms}", exact32)
        w = width(self.rows)
        m = len(self.rows)
        live = [len(c) > 0 for _, c in self.rows]
        arp = np.zeros(m + 1, np.int32)
        np.cumsum([terms if l else 0 for l in live], out=arp[1:])               # the empty row: a row of A without entries
        self.A = Host64(arp, np.arange(arp[-1]), np.full(arp[-1], 0.5 / terms), m, arp[-1])
        brows = [c for (_, c), l in zip(self.rows, live) if l for _ in range(terms)]
        brp = np.zeros(len(brows) + 1, np.int32)
        np.cumsum([len(c) for c in brows], out=brp[1:])
        self.B = Host64(brp, np.concatenate([columns(len(c), w) for c in brows]), np.concatenate(brows) * 2.0, len(brows), w)
        self.step = step64(self.A, self.B)
        self.products = [terms * len(c) for _, c in self.rows]
        self.bin_rows = [int(sum(np.searchsorted(self.BIN_EDGES, p) == b for p in self.products)) for b in range(9)]
        # the product is what the rows say, bit for bit, and the step's bound is the case's
        assert self.step.N == terms and self.step.n == n
        for r, (_, c) in enumerate(self.rows):
            a, b = self.step.product.rowPtr[r], self.step.product.rowPtr[r + 1]
            order = np.argsort(columns(len(c), w), kind="stable")
            assert np.array_equal(self.step.product.values[a:b], c[order])


def kept_with(C, th):
    """the rule on the rows of C with the given per-row thresholds -> Host64 of the kept entries in input order"""
    rp = np.asarray(C.rowPtr, np.int64)
    v = C.values ** 2
    row_of = np.repeat(np.arange(C.rows), np.diff(rp))
    keep = v >= np.asarray(th, np.float64)[row_of]
    nrp = np.zeros(C.rows + 1, np.int32)
    np.cumsum(np.bincount(row_of[keep], minlength=C.rows), out=nrp[1:])
    ks = np.zeros(C.rows)
    np.add.at(ks, row_of[keep], v[keep])
    return Host64(nrp, C.colInd[keep], v[keep] / ks[row_of[keep]], C.rows, C.cols)


def exact_values(kind_rows, rowPtr, dtype):
    """{row: the values a row of a kind in EXACT must hold, bit for bit, in dtype}"""
    out = {}
    for r, (kind, _) in enumerate(kind_rows):
        k = int(rowPtr[r + 1] - rowPtr[r])
        if kind in EXACT and k:
            out[r] = np.full(k, dtype(1.0) / dtype(k), dtype=dtype)
    return out


# ---- the float threshold's promotions ------------------------------------------------------------------------------------
def threshold_f32(avg, mx):
    """computeThreshold with QValue = float, operation by operation: mx - avg, 2 * that and 1 - that in float, 0.90 * avg
    and the product in double, one rounding to float; the floor compares the float with the double 1.0e-7"""
    avg, mx = np.float32(avg), np.float32(mx)
    factor = np.float32(1) - np.float32(2) * np.float32(mx - avg)
    ret = np.float32(0.90 * float(avg) * float(factor))
    ret = ret if float(ret) > 1.0e-7 else np.float32(1.0e-7)
    return mx if ret > mx else ret


def threshold_all_f32(avg, mx):
    """the same with every operation in float"""
    avg, mx = np.float32(avg), np.float32(mx)
    ret = np.float32(np.float32(np.float32(0.90) * avg) * (np.float32(1) - np.float32(2) * np.float32(mx - avg)))
    ret = ret if ret > np.float32(1.0e-7) else np.float32(1.0e-7)
    return mx if ret > mx else ret


def threshold_all_f64(avg, mx):
    """the same with nothing rounded to float before the result (float inputs)"""
    avg, mx = float(avg), float(mx)
    ret = 0.90 * avg * (1 - 2 * (mx - avg))
    ret = ret if ret > 1.0e-7 else 1.0e-7
    return mx if ret > mx else ret


PROMOTION_WINDOWS = {"kept": (3201, 580, 200, 3), "dropped": (3210, 860, 230, 4)}      # k0, first k1, first k2, probe


def promotion_row(which):
    """A float row of eight entries k * 2^-12, k = (k0, k1, k2, 1024 x 4, probe), whose sum of squares is an integer below
    2^24 times 2^-24: exact in float32 in any order, and so are avg = sum / 8 and mx.  A float kernel's threshold is then
    known bit for bit.  mx - avg sits just below 0.5, so 1 - 2 * (mx - avg) is tiny and the rounding of mx - avg to
    float (computeThreshold's promotions) moves the threshold by thousands of its ulps against an evaluation that keeps
    mx - avg in double.  Searched over 64 x 64 candidates (k1, k2): the first whose probe entry lies between the two
    thresholds, at least 1000 float ulps of the threshold clear of the float rule's, on the side `which` names (kept or
    dropped by the float rule; the all-double rule decides the other way), every other entry a factor of two clear.
    -> (values, index of the probe, float-rule threshold, all-double threshold)"""
    k0, k1lo, k2lo, kp = PROMOTION_WINDOWS[which]
    for k1 in range(k1lo, k1lo + 64):
        for k2 in range(k2lo, k2lo + 64):
            k = np.array([k0, k1, k2, 1024, 1024, 1024, 1024, kp], np.int64)
            s = int((k * k).sum())
            if s >= 1 << 24:
                continue
            c = k * 2.0 ** -12
            v = c * c
            avg, mx = np.float32(s / 8 * 2.0 ** -24), np.float32(v.max())
            assert float(avg) == s / 8 * 2.0 ** -24 and float(mx) == v.max()
            tf, td = float(threshold_f32(avg, mx)), threshold_all_f64(avg, mx)
            if tf <= 1.0e-7 or td <= 1.0e-7:
                continue
            ulp = float(np.spacing(np.float32(tf)))
            lo, hi = min(tf, td), max(tf, td)
            if (lo < v[7] < hi and abs(v[7] - tf) >= 1000 * ulp and (v[7] >= tf) == (which == "kept")
                    and np.all((v[:7] > 2 * hi) | (v[:7] < lo / 2))):
                return c, 7, tf, td
    raise AssertionError("no row among the candidates")


# ---- a loop that lives in these branches ---------------------------------------------------------------------------------
LOOP_COMPONENTS = [((8, 3), (3, 9)), ((4, 4), (1, 5)), ((3, 8), (2, 8))]      # clique sizes, the edge that joins them
LOOP_MAX_ITERS = 15


def loop_graph():
    """what rmclInit makes (self loops, rows 1/deg) of three components, each two cliques joined by a single edge: cliques
    of 8 and 3, of 4 and 4, of 3 and 8.  Chosen on the reference alone (a search over such pairs): the loop converges to
    one 1.0 per row within ten iterations, rows pass through the floor branch on the way, and in every iteration k every
    gap is at least 1000 * k * the largest step bound in float."""
    blocks, n = [], 0
    for sizes, (a, b) in LOOP_COMPONENTS:
        k = sum(sizes)
        W = np.zeros((k, k))
        o = 0
        for s in sizes:
            W[o:o + s, o:o + s] = 1.0
            o += s
        W[a, b] = W[b, a] = 1.0
        blocks.append((n, W))
        n += k
    r = np.concatenate([o + np.nonzero(W)[0] for o, W in blocks])
    c = np.concatenate([o + np.nonzero(W)[1] for o, W in blocks])
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=n), out=rp[1:])
    return Host64(rp, c, (1.0 / np.diff(rp))[r], n, n)


def loop_case(dtype):
    """-> (M with dtype-rounded values, the reference's steps up to the first whose nnz equals the one before and the row
    count, per-iteration bounds k * largest step bound so far, rows in a floor branch per iteration); the preconditions
    are asserted"""
    from rmcl_f64_ref import loop64
    M = loop_graph()
    M = Host64(M.rowPtr, M.colInd, M.values.astype(dtype), M.rows, M.cols)
    _, steps = loop64(M, M, LOOP_MAX_ITERS)
    nn = [s.kept.nnz for s in steps]
    stop = [i for i in range(1, len(nn)) if nn[i] == nn[i - 1] == M.rows]
    assert stop, f"the loop does not reach one entry per row in {LOOP_MAX_ITERS} iterations: nnz {nn}"
    steps = steps[:stop[0] + 1]
    bounds, floors = [], []
    for k, s in enumerate(steps, 1):
        bounds.append(k * max(step_bound(t.N, t.n, UNIT[dtype]) for t in steps[:k]))
        assert float(s.gap.min()) >= 1000.0 * bounds[-1], f"iteration {k}: gap {s.gap.min():.3e} < 1000 * {bounds[-1]:.3e}"
        p = s.product
        floors.append(sum(branch_of(p.values[p.rowPtr[r]:p.rowPtr[r + 1]] ** 2) in ("floor-negative", "floor-small")
                          for r in range(M.rows)))
    final = steps[-1].kept
    assert max(floors) > 0, "no iteration has a row in the floor branch"
    assert np.all(np.diff(final.rowPtr) == 1) and np.all(final.values == 1.0), "the final rows are not single 1.0 entries"
    return M, steps, bounds, floors
