"""A numpy restatement of the classification front end (per-row products, layout slots, stable row order, the
reference-shaped histogram) for exact comparison with the device: tests/test_gpu_classify_front.py.  The per-row products
are pinned against oracle/pyoracle.py by tests/test_classify_ref.py."""
import numpy as np

NSLOTS = 16
# upper product count of layout slots 0..9; rows above 4096 products take slots 10..15 by power of two, LARGEST FIRST
# (slot 15: 4097..8191, slot 14: 8192..16383, ..., slot 10: everything from 131072 on)
SLOT_MAX = [0, 1, 4, 16, 64, 256, 512, 1024, 2048, 4096]
# reference bins of gpuFlopsClassify (hv): {0} {1} {2..4} {5..16} {17..64} {65..512} {>512}
REF_BIN_MAX = [0, 1, 4, 16, 64, 512]


def row_products(IA, JA, IB):
    """products of every row of A*B: the sum of len(B[j]) over the row's entries (int64; a negative length counts 0)"""
    IA, JA, IB = (np.asarray(x, dtype=np.int64) for x in (IA, JA, IB))
    lens = np.maximum(IB[JA + 1] - IB[JA], 0) if len(JA) else np.zeros(0, dtype=np.int64)
    csum = np.concatenate([[0], np.cumsum(lens)])
    return csum[IA[1:]] - csum[IA[:-1]]


def slot_of(flops):
    f = np.asarray(flops, dtype=np.int64)
    slot = np.searchsorted(np.asarray(SLOT_MAX, dtype=np.int64), f, side="left")        # 0..9, 10 for f > 4096
    big = f > 4096
    lg = np.floor(np.log2(np.maximum(f, 1))).astype(np.int64)                            # exact for these magnitudes
    lg = np.clip(lg, 12, 17)
    return np.where(big, 10 + (5 - (lg - 12)), slot).astype(np.int64)


def row_order(flops):
    """row ids as the device lays them out: by layout slot, ascending row id inside a slot"""
    return np.argsort(slot_of(flops), kind="stable").astype(np.int32)


def slot_counts(flops):
    return np.bincount(slot_of(flops), minlength=NSLOTS)


def hv_of(flops):
    """(hv, hv_len) of gpuFlopsClassify: the reference counts a dummy row of 0 products in front of the first bin"""
    f = np.asarray(flops, dtype=np.int64)
    b = np.searchsorted(np.asarray(REF_BIN_MAX, dtype=np.int64), f, side="left") + 1   # 1..7
    cnt = np.bincount(b, minlength=8)
    cnt[1] += 1
    hv = np.concatenate([[0], np.cumsum(cnt)])
    maxbin = max(int(np.nonzero(cnt)[0].max()), 1)
    return [int(x) for x in hv], maxbin + 2


def dflops_of(flops, order):
    """the int32 scan of the products in layout order, wrapping modulo 2^32 like the device's"""
    f = np.asarray(flops, dtype=np.int64)[order]
    scan = np.concatenate([[0], np.cumsum(f)]) % (1 << 32)
    return scan.astype(np.uint32).view(np.int32)
