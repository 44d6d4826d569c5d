"""CPU: the numpy restatement of the classification (tests/classify_ref.py) against the oracle on the same inputs."""
import numpy as np
import pytest

import classify_ref as cr
from helpers import po, random_csr, synth_csr


def _cases():
    yield "synth 20000", synth_csr(20000, 23, 2), None
    yield "synth 3001", synth_csr(3001, 5, 2), None
    A, B = random_csr(257, 300, 0.05, 3), random_csr(300, 4000, 0.2, 4)
    yield "rectangular, rows up to thousands of products", A, B
    yield "empty rows at both ends", random_csr(130, 130, 0.01, 9), None


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_row_products_and_histogram_match_the_oracle(case):
    _, A, B = case
    B = A if B is None else B
    want = po.row_flops(A, B)
    got = cr.row_products(A.rowPtr, A.colInd, B.rowPtr)
    assert np.array_equal(got, want)
    o_ids, o_scan, o_hv, o_len = po.gpu_classify(want)
    hv, hv_len = cr.hv_of(got)
    assert hv == [int(x) for x in o_hv] and hv_len == o_len
    # the oracle's order is the reference's (a stable sort by its seven bins); the layout order refines it: the same rows
    # in every reference bin, ascending inside every layout slot
    order = cr.row_order(got)
    assert sorted(order.tolist()) == list(range(A.rows))
    for b in range(1, 8):
        lo, hi = max(hv[b] - 1, 0), hv[b + 1] - 1
        assert np.array_equal(np.sort(order[lo:hi]), np.sort(o_ids[lo:hi])), b
    slots = cr.slot_of(got)[order]
    assert np.all(np.diff(slots) >= 0)
    assert np.all((np.diff(order) > 0) | (np.diff(slots) > 0))


def test_slot_edges():
    f = np.array([0, 1, 2, 4, 5, 16, 17, 64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096,
                  4097, 8191, 8192, 16383, 16384, 32767, 32768, 65535, 65536, 131071, 131072, 131073, 1 << 30])
    want = [0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9,
            15, 15, 14, 14, 13, 13, 12, 12, 11, 11, 10, 10, 10]
    assert cr.slot_of(f).tolist() == want
