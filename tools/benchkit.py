"""tools/benchkit.py — what the *_bench.py tools share: the workloads, the two clocks, the take-turns loop, the d2d arm,
the round-trip predicate of the parity gates and the command-line / JSON frame.  A library, not a tool: the tools import
it, and no tool imports another tool."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sparse_matrix_with_flops_amd import hipspgemm as hs  # noqa: E402
from sparse_matrix_with_flops_amd import synth  # noqa: E402

WORKLOADS = {
    "synth_1m_16": lambda: synth.powerlaw_csr(1 << 20, 43, 2)[:3],          # the matrix bench.py times
    "synth_256k_16": lambda: synth.powerlaw_csr(1 << 18, 43, 2)[:3],
    "web_google_surrogate": lambda: synth.webgraph_csr(916428, 46)[:3],
}
D2D = 3                                                     # hipMemcpyDeviceToDevice
HOST_CLOCK = "host clock around blocking calls, median"
HIP_EVENTS = "HIP events on the handle's stream around blocking calls, median"


def load(name):
    """-> the square workload `name` as a host hs.CSR (float32)"""
    rp, ci, v = WORKLOADS[name]()
    return hs.CSR.from_arrays(rp, ci, v, len(rp) - 1, len(rp) - 1)


# ---- the two clocks: both return (milliseconds, fn's result) ---------------------------------------------------------
def clock(fn):
    """host clock around a blocking call"""
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


class Events:
    """two HIP events on one stream: ms(fn) = device-timeline milliseconds from before fn() to after it"""

    def __init__(self, stream):
        try:
            self.hip = C.CDLL("libamdhip64.so")
        except OSError:
            self.hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.stream = C.c_void_p(stream)
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        for e in (self.e0, self.e1):
            self.ok(self.hip.hipEventCreate(C.byref(e)), "hipEventCreate")

    @staticmethod
    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"{what} failed with HIP error {rc}")

    def ms(self, fn):
        self.ok(self.hip.hipEventRecord(self.e0, self.stream), "hipEventRecord")
        out = fn()
        self.ok(self.hip.hipEventRecord(self.e1, self.stream), "hipEventRecord")
        self.ok(self.hip.hipEventSynchronize(self.e1), "hipEventSynchronize")
        t = C.c_float(0)
        self.ok(self.hip.hipEventElapsedTime(C.byref(t), self.e0, self.e1), "hipEventElapsedTime")
        return float(t.value), out

    def copy(self, dst, src, nbytes):
        self.ok(self.hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), nbytes, D2D, self.stream), "hipMemcpyAsync")

    def close(self):
        for e in (self.e0, self.e1):
            self.hip.hipEventDestroy(e)


def med(x):
    return round(float(np.median(x)), 4)


def rounded(x):
    return [round(t, 4) for t in x]


# ---- arms ------------------------------------------------------------------------------------------------------------
def release(out):
    """frees what a timed arm made: None, a list of device pointers, a BCSR / MCSR, or a device CSR / PCSR"""
    if out is None:
        return
    if isinstance(out, list):
        for p in out:
            hs.dev_free(p)
    elif hasattr(out, "dispose"):
        out.dispose()
    else:
        out.deviceDispose()


def take_turns(arms, reps, warmup, timer=clock, free=release):
    """arms: {name: fn}.  The arms take turns, each call timed by timer(fn) -> (ms, result) and its result handed to
    free() outside the timed region (free=None: kept).  -> ({name: [ms per repetition]}, {name: last result})"""
    times, last = {k: [] for k in arms}, {}
    for it in range(warmup + reps):
        for name, fn in arms.items():
            ms, last[name] = timer(fn)
            if free is not None:
                free(last[name])
            if it >= warmup:
                times[name].append(ms)
    return times, last


def copy_buffers(M):
    """three device buffers the size of device CSR M's arrays (release them with hs.dev_free)"""
    return [hs.dev_alloc(4 * (M.rows + 1)), hs.dev_alloc(4 * M.nnz), hs.dev_alloc(M.dtype.itemsize * M.nnz)]


def d2d_arm(M, copy, ev=None):
    """the ceiling arm: the three arrays of device CSR M copied device to device into `copy`.  With ev (an Events) the
    copies go on its stream, for its events to time; without, through the library and a device synchronise, since a
    device-to-device copy may return before it has run and the arm must block as the entry points beside it do."""
    sizes = (4 * (M.rows + 1), 4 * M.nnz, M.dtype.itemsize * M.nnz)

    def run():
        for dst, src, nbytes in zip(copy, (M.rowPtr, M.colInd, M.values), sizes):
            ev.copy(dst, src, nbytes) if ev else hs.d2d(dst, src, nbytes)
        if not ev:
            hs.device_synchronize()
    return run


def round_trip_differs(got, want, d):
    """the parity gates' rule on d = got.diff(want): another nnz, row length or column, or a value beyond the tolerance"""
    return bool(got.nnz != want.nnz or d.rows_len_differ or d.only_a or d.only_b or d.beyond)


# ---- the frame of a tool ---------------------------------------------------------------------------------------------
def parser(doc, tool):
    """--reps, --warmup and --out (default profiles/<tool>.json); the tool adds its own options"""
    ap = argparse.ArgumentParser(description=doc.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", tool + ".json"))
    return ap


def need_device(tool):
    if hs.device_count() < 1:
        raise SystemExit(f"{tool}.py needs a HIP device (there is no CPU fallback)")


def finish(tool, args, workloads, timing=HOST_CLOCK, **extra):
    """writes the tool's JSON document to args.out and prints it; call it only after every gate has passed"""
    res = {"tool": tool, "timing": timing, "reps": args.reps, "warmup": args.warmup, **extra, "workloads": workloads}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
