"""Float64 reference of the R-MCL step in double (hip_rmcl_prune_f64, hip_rmcl_expand_prune_f64, hip_gpuRmclIter*_f64),
built on f64ref.spgemm_f64.

The row rule (nlibs/tools/util.cc:4-69, nlibs/qrmcl.cc:96-117 with QValue = double), per row of `count` stored entries:
  v = c*c;  mx = max(0, v...);  avg = sum(v) / count;  th = 0.90*avg*(1 - 2*(mx - avg));  th = th if th > 1e-7 else 1e-7;
  th = mx if th > mx else th;  keep v >= th in input order;  kept v / sum(kept v).
An empty row stays empty: 0/0 is NaN, NaN > 1e-7 is false, so th = 1e-7 and then th = mx = 0.  A one-entry row has
avg = mx = v, th = min(max(0.9 v, 1e-7), v): the entry is kept and becomes 1.0.  A row with mx < 1e-7 has th = mx: exactly
its largest entries are kept.

Value bound of one step for non-negative inputs, in units of u = 2^-53, relative to the reference value.  A product entry
of N terms (all >= 0, so S = the value itself) computed in any order is within 2N u of the reference's (f64ref).  Its
square: (1 + 2N u)^2 and one rounding, within (4N + 1) u.  The kept sum adds at most n such terms (n = the longest product
row), each within (4N + 1) u, and two orders of that sum differ by at most 2n u: within (4N + 1 + 2n) u.  The quotient of a
square within (4N + 1) u and a sum within (4N + 1 + 2n) u, plus its own rounding, is within (8N + 2n + 3) u (one u more
where the device multiplies by the rounded reciprocal of the sum); the accepted bound (8N + 2n + 16) u leaves the
second-order terms their room.  For hip_rmcl_prune_f64 on a given C the products are the
same bits on both sides: N = 0.  A k-iteration loop is compared with k times the largest per-step bound.

The bound says nothing about WHICH entries are kept.  That is the gap's job: gap = min |v - th| / th over the entries of a
row.  The device's v and th are within the value bound of the reference's, so while every gap is far above the bound
(the tests demand 1000 times) a correct implementation keeps exactly the reference's entries.
"""
import numpy as np

from f64ref import EPS64, Host64, spgemm_f64


def threshold64(avg, mx):
    """computeThreshold for arrays of row averages and row maxima (NaN averages of empty rows included)"""
    with np.errstate(invalid="ignore"):
        th = 0.90 * avg * (1 - 2 * (mx - avg))
        th = np.where(th > 1.0e-7, th, 1.0e-7)
        th = np.where(th > mx, mx, th)
    return th


def row_rule64(rowPtr, colInd, values):
    """-> (Host64 of the kept entries in input order, per-row threshold, per-row gap min |v^2 - th| / th; inf for a row
    without entries or with th == 0)"""
    rp = np.asarray(rowPtr, np.int64)
    ci = np.asarray(colInd, np.int32)
    m = len(rp) - 1
    v = np.asarray(values, np.float64) ** 2
    cnt = np.diff(rp)
    live = cnt > 0
    starts = rp[:-1][live]
    mx = np.zeros(m)
    sm = np.zeros(m)
    if len(v):
        mx[live] = np.maximum(np.maximum.reduceat(v, starts), 0.0)
        # a plain left-to-right sum per row, as arraySum does (np.sum and reduceat add pairwise; np.cumsum does not)
        sm[live] = [np.cumsum(v[a:b])[-1] for a, b in zip(rp[:-1][live], rp[1:][live])]
    with np.errstate(invalid="ignore", divide="ignore"):
        th = threshold64(sm / cnt, mx)
    row_of = np.repeat(np.arange(m, dtype=np.int64), cnt)
    keep = v >= th[row_of]
    gap = np.full(m, np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.abs(v - th[row_of]) / th[row_of]
    g = np.where(np.isnan(g), np.inf, g)
    if len(v):
        gap[live] = np.minimum.reduceat(g, starts)
    kcnt = np.bincount(row_of[keep], minlength=m)
    nrp = np.zeros(m + 1, np.int32)
    np.cumsum(kcnt, out=nrp[1:])
    ksum = np.zeros(m)
    klive = kcnt > 0
    kv = v[keep]
    if len(kv):
        ksum[klive] = [np.cumsum(kv[a:b])[-1] for a, b in zip(nrp[:-1][klive], nrp[1:][klive])]
    out = kv / ksum[row_of[keep]]
    return Host64(nrp, ci[keep], out, m, 0), th, gap


class Step64:
    """one reference step: the kept matrix (rows column-sorted), thresholds, gaps, N, n, the value bound and the product"""

    def __init__(self, kept, th, gap, N, n, product):
        self.kept, self.th, self.gap, self.N, self.n, self.product = kept, th, gap, int(N), int(n), product
        self.bound = step_bound(N, n)


def step_bound(N, n, u=EPS64):
    """the value bound above; u = the unit roundoff of the device's value type (2^-24 for the float kernels)"""
    return (8 * int(N) + 2 * int(n) + 16) * u


def step64(Mgt, Mt):
    """row_rule64(spgemm_f64(Mgt, Mt)) with N = max terms per entry and n = the longest product row"""
    ref = spgemm_f64(Mgt, Mt)
    kept, th, gap = row_rule64(ref.rowPtr, ref.colInd, ref.values)
    kept.cols = Mt.cols
    N = int(ref.nterms.max()) if ref.nnz else 0
    n = int(np.diff(ref.rowPtr).max()) if ref.rows else 0
    return Step64(kept, th, gap, N, n, ref)


def loop64(Mgt, Mt, k):
    """k steps Mt <- step64(Mgt, Mt) -> (final Mt, list of the k Step64)"""
    steps = []
    cur = Mt
    for _ in range(k):
        s = step64(Mgt, cur)
        steps.append(s)
        cur = s.kept
    return cur, steps
