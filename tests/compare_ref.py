"""numpy restatement of the comparison members of the reference's CSR, row by row with plain loops and dicts:
  report            the fields of spgemm_csr_diff (include/spgemm_hip.h), every term one double operation on the stored values
  differs_f32       CSR::differs          nlibs/CSR.cc:210-240   (the sequential two-pointer merge, summed in float32)
  differs_stats     CSR::differsStats     nlibs/CSR.cc:381-415
  is_equal          CSR::isEqual          nlibs/CSR.h:195-245    (a dense row scatter)
  is_relative_equal CSR::isRelativeEqual  nlibs/CSR.h:284-320    (every row, not only the first the reference's loop reaches)
Operands expose rowPtr / colInd / values / rows / cols; rows strictly ascending by column."""
import math

import numpy as np

def _rows(M):
    """-> per row a dict column -> value (as a Python float, i.e. the stored value converted exactly to double)"""
    rp = np.asarray(M.rowPtr, np.int64)
    ci, v = np.asarray(M.colInd), np.asarray(M.values)
    return [dict(zip(ci[rp[i]:rp[i + 1]].tolist(), v[rp[i]:rp[i + 1]].astype(np.float64).tolist())) for i in range(M.rows)]


def report(A, B, rel=1e-6, abs_tol=0.0):
    """-> (dict of the spgemm_csr_diff fields except sum_sq, list of the double terms of sum_sq)"""
    assert (A.rows, A.cols) == (B.rows, B.cols)
    r = dict(rows_len_differ=0, first_len_row=-1, only_a=0, only_b=0, first_only_row=-1, beyond=0, first_beyond_row=-1,
             max_abs_err=0.0, max_rel_err=0.0, max_abs_only_a=0.0, max_abs_only_b=0.0)
    terms = []

    def first(key, i):
        if r[key] < 0:
            r[key] = i

    for i, (ra, rb) in enumerate(zip(_rows(A), _rows(B))):
        if len(ra) != len(rb):
            r["rows_len_differ"] += 1
            first("first_len_row", i)
        for c, a in ra.items():
            if c in rb:
                b = rb[c]
                d = abs(a - b)
                if not d <= abs_tol + rel * abs(b):
                    r["beyond"] += 1
                    first("first_beyond_row", i)
                if d > r["max_abs_err"]:
                    r["max_abs_err"] = d
                if b != 0.0 and d / abs(b) > r["max_rel_err"]:
                    r["max_rel_err"] = d / abs(b)
                terms.append((a - b) * (a - b))
            else:
                r["only_a"] += 1
                first("first_only_row", i)
                if abs(a) > r["max_abs_only_a"]:
                    r["max_abs_only_a"] = abs(a)
                terms.append(a * a)
        for c, b in rb.items():
            if c not in ra:
                r["only_b"] += 1
                first("first_only_row", i)
                if abs(b) > r["max_abs_only_b"]:
                    r["max_abs_only_b"] = abs(b)
                terms.append(b * b)
    return r, terms


def sum_sq(terms):
    return math.fsum(terms) if all(t == t for t in terms) else float("nan")


def differs_f32(A, B):
    """CSR::differs with QValue float (nlibs/CSR.cc:210-240): every operation rounded to float32, summed in storage order.
    (The reference's last loop stops at A's row end instead of B's; the merge is restated as its comment describes it.)"""
    f = np.float32
    s = f(0)
    arp, brp = np.asarray(A.rowPtr, np.int64), np.asarray(B.rowPtr, np.int64)
    ac, bc = np.asarray(A.colInd), np.asarray(B.colInd)
    av, bv = np.asarray(A.values, np.float32), np.asarray(B.values, np.float32)
    for i in range(A.rows):
        j, k = arp[i], brp[i]
        while j < arp[i + 1] and k < brp[i + 1]:
            if ac[j] == bc[k]:
                d = f(av[j] - bv[k])
                s = f(s + f(d * d))
                j += 1
                k += 1
            elif ac[j] < bc[k]:
                s = f(s + f(av[j] * av[j]))
                j += 1
            else:
                s = f(s + f(bv[k] * bv[k]))
                k += 1
        for q in range(j, arp[i + 1]):
            s = f(s + f(av[q] * av[q]))
        for q in range(k, brp[i + 1]):
            s = f(s + f(bv[q] * bv[q]))
    return float(s)


def differs_stats(arp, brp, percents, dtype=np.float32):
    """CSR::differsStats (nlibs/CSR.cc:381-415) on two row pointers; the division and the compare in `dtype` (QValue)"""
    q = np.dtype(dtype).type
    pc = [q(p) for p in percents]
    n = len(pc)
    counts = [0] * (n + 4)
    a_len, b_len = np.diff(np.asarray(arp, np.int64)), np.diff(np.asarray(brp, np.int64))
    for acount, bcount in zip(a_len.tolist(), b_len.tolist()):
        if acount == 0 and bcount > 0:
            counts[n + 1] += 1
        elif acount == 0 and bcount == 0:
            counts[n + 2] += 1
        elif acount == bcount:
            counts[n + 3] += 1
        else:
            percent = q(q(bcount - acount) / q(acount))
            for k in range(n):
                if percent < pc[k]:
                    counts[k] += 1
                    break
            else:
                counts[n] += 1
    assert sum(counts) == len(a_len)                        # nlibs/CSR.cc:409-413
    return counts


def is_equal(A, B):
    """CSR::isEqual (nlibs/CSR.h:195-245)"""
    if (A.rows, A.cols, len(A.colInd)) != (B.rows, B.cols, len(B.colInd)):
        return False
    if not np.array_equal(np.asarray(A.rowPtr), np.asarray(B.rowPtr)):
        return False
    for ra, rb in zip(_rows(A), _rows(B)):
        for c, b in rb.items():                             # rowVals[col] is 0.0 where A holds nothing
            if abs(ra.get(c, 0.0) - b) > 1e-7:
                return False
    return True


def is_relative_equal(A, B, max_rel):
    """CSR::isRelativeEqual (nlibs/CSR.h:284-320): entries of A with |a| <= 1e-8 count as absent; an entry of B with
    |b| > 1e-8 must be met within max_rel relative"""
    if (A.rows, A.cols) != (B.rows, B.cols):
        return False
    for ra, rb in zip(_rows(A), _rows(B)):
        for c, b in rb.items():
            a = ra.get(c, 0.0)
            if abs(a) <= 1e-8:
                a = 0.0
            if abs(b) > 1e-8 and abs((a - b) / b) > max_rel:
                return False
    return True
