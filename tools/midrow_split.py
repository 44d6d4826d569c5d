#!/usr/bin/env python3
"""Which numeric kernel the rows of 513-4096 products take on the benchmark's SpGEMM workloads: C = A * A three times on a
fresh handle (the first call has no log), then Handle.midrow_paths() of the third call -- with the log's size and the
symbolic kernel that filled it (Handle.midrow_sym_paths()) -- one JSON line per workload.
The SPGEMM_* knobs in the environment apply (SPGEMM_MW_MINROWS=1 forces the wave-per-row kernel on a small bin 6).

    python tools/midrow_split.py [workload ...]          (default: the four SpGEMM workloads of bench.py)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import WORKLOADS, bin_of  # noqa: E402
from sparse_matrix_with_flops_amd import hipspgemm as hs, synth  # noqa: E402


def split(name):
    wl = WORKLOADS[name]
    if wl.get("gen") == "web":
        rp, ci, v = synth.webgraph_csr(wl["m"], wl["seed"])
    else:
        rp, ci, v = synth.powerlaw_csr(wl["m"], wl["seed"], wl["base"])
    m = wl["m"]
    upto = np.concatenate([[0], np.cumsum(np.diff(rp.astype(np.int64))[ci])])
    flops = upto[rp[1:]] - upto[rp[:-1]]                 # products per row of A * A
    bins = np.bincount(bin_of(flops), minlength=9)
    h = hs.Handle(0)
    dA = hs.CSR.from_arrays(rp, ci, v, m, m).toGpuCSR()
    try:
        for _ in range(3):
            hs.gpuSpMMWrapper(dA, dA, h).deviceDispose()
        p = h.midrow_paths()
        if hasattr(h, "midrow_sym_paths"):               # the symbolic kernel of bin 6 (SPGEMM_SYM_PAIR, SPGEMM_SP_MINROWS)
            p.update({"sym_" + k: v for k, v in h.midrow_sym_paths().items()})
    finally:
        dA.deviceDispose()
        h.close()
    return dict(workload=name, rows_bin6=int(bins[6]), rows_bin7=int(bins[7]), **p)


if __name__ == "__main__":
    names = sys.argv[1:] or ["synth_1m_16", "synth_256k_16", "web_google_surrogate", "synth_1m_32"]
    for n in names:
        print(json.dumps(split(n)), flush=True)
