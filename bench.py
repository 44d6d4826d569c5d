#!/usr/bin/env python3
"""bench.py — the SpGEMM hot path on MI355X, measured per the driver contract.

    python bench.py --gpus N --steps K --warmup W [--workload NAME] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the result line (metric, value, unit, ms_per_step, ...).
--full adds everything else the line used to carry: the untimed per-kernel profiling pass and the roofline, the parity
gate against the CPU oracle, the CPU baseline, the host-array entry point and (default workload, N=1) the short runs of
the other workloads.  --dump-outputs DIR writes what the last timed step computed as .npy files (see dump_outputs).

N > 1 without a launcher (WORLD_SIZE unset): this process starts the N ranks itself as a child
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N ...` BEFORE it touches the GPU, waits, and relays
rank 0's JSON line (exit code = the child's).  Under a launcher (WORLD_SIZE set) the world size must equal --gpus.

A "step" is one pass of the hot path — per-row flop count, row binning, symbolic, scan, numeric (and for N>1 the
allgatherv of C) — over one synthetic matrix that is already resident in HBM when the timed region starts.
Metric (BASELINE.json): SpGEMM GFLOP/s = 2*P / t with P = intermediate products; output nnz/s is reported next to
it.  Rank 0 prints ONE JSON line.

Workloads (SURVEY.md §8d generator, sparse_matrix_with_flops_amd/synth.py):
  synth_1m_16    1 048 576^2, ~16 nnz/row, seed 43   <- default: the configuration the metric is quoted on
  synth_256k_16  262 144^2,  ~16 nnz/row, seed 42    (BASELINE.json configs[1])
  synth_1m_32    1 048 576^2, ~32 nnz/row, seed 44   (configs[3], the row-sharded multi-GPU case)
  web_google_surrogate  916 428^2, ~5.5 nnz/row, nnzC/P ~0.49 (configs[2] by shape; the real file is not available)
  rmcl_500k      configs[4]: the R-MCL loop (expand Mgt*Mt + inflate/prune/normalise fused: hip_rmcl_expand_prune) on the
                 500 000-node power-law graph (seed 45), 10 iterations per step, device-resident

N > 1: one process per GPU.  With --backend nccl (default) the ranks form a group INSIDE libspgemm_hip.so
(spgemm_hip_group_create_rank, RCCL loaded by the library; the id travels over torch.distributed) and the exchange is the
library's grouped ncclSend/ncclRecv; if that group cannot be made the step falls back to the torch.distributed exchange
of sparse_matrix_with_flops_amd/dist.py and says so in "transport".  --backend gloo rehearses the N>1 path on a box with
fewer GPUs than ranks.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "synth_1m_16": dict(m=1 << 20, seed=43, base=2, desc="synthetic power-law CSR 1048576^2, ~16 nnz/row, seed 43, C=A*A"),
    "synth_256k_16": dict(m=1 << 18, seed=42, base=2, desc="synthetic power-law CSR 262144^2, ~16 nnz/row, seed 42, C=A*A"),
    "synth_1m_32": dict(m=1 << 20, seed=44, base=4, desc="synthetic power-law CSR 1048576^2, ~32 nnz/row, seed 44, C=A*A"),
    "synth_64k_16": dict(m=1 << 16, seed=17, base=2, desc="synthetic power-law CSR 65536^2 (smoke-sized)"),
    # BASELINE.json configs[2] by shape (the real file is in neither container): synth.webgraph_csr, nnzC/P = 0.49
    "web_google_surrogate": dict(m=916428, seed=46, gen="web",
                                 desc="web-Google-shaped surrogate 916428^2, ~5.5 nnz/row, nnzC/P~0.49, seed 46, C=A*A "
                                      "(surrogate; reference totals unpinned)"),
    # BASELINE.json configs[4]: R-MCL, 10 iterations
    "rmcl_500k": dict(m=500000, seed=45, base=2, gen="rmcl", iters=10,
                      desc="R-MCL (expand Mgt*Mt + inflate/prune/normalise) on a 500000-node power-law graph, seed 45, "
                           "10 iterations per step, device-resident"),
    "rmcl_20k": dict(m=20000, seed=91, base=2, gen="rmcl", iters=3, desc="R-MCL, 20000 nodes, 3 iterations (smoke-sized)"),
}

# The contract is ONE JSON line on stdout.  Libraries in this process print there too (RCCL's version banner, the reference's
# own printf progress lines inside the cpu_baseline call): file descriptor 1 is pointed at stderr for the whole run and the
# result line goes to the saved descriptor.
_REAL_STDOUT = None


def protect_stdout():
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def emit(line):
    sys.stdout.flush()
    if _REAL_STDOUT is None:
        print(line)
        return
    os.write(_REAL_STDOUT, (line + "\n").encode())


HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
ALL_KERNELS = 0x1FFFFF


def bin_of(f):
    edges = np.array([0, 1, 4, 16, 64, 512, 2048, 4096], dtype=np.int64)   # bin b holds flops <= edges[b]; last bin beyond
    return np.searchsorted(edges, f, side="left").astype(np.int64)


# which bins each kernel covers, and whether it is a symbolic (keys only) or numeric launch
KERNEL_BINS = {
    "k_sym_g16<32,1>": ((2, 3), "sym"), "k_sym_g16": ((4,), "sym"), "k_sym_hash<1,1024>": ((5,), "sym"),
    "k_sym_hash<4,4096>": ((6,), "sym"), "k_sym_hash<8,8192>": ((7,), "sym"), "k_sym_big": ((8,), "sym"),
    "k_num_g16<32,1>": ((1, 2, 3), "num"), "k_num_g16": ((4,), "num"), "k_num_hash<1,1024>": ((5,), "num"),
    "k_num_hash<4,4096>": ((6,), "num"), "k_num_hash<8,8192>": ((7,), "num"), "k_num_big": ((8,), "num"),
    "k_num_bighash": ((8,), "num"),
    # round 4, the one-pass kernel: classification aside, everything BYTES_ALG credits for its rows happens in this launch
    "k_chain": ((0, 1, 2, 3, 4, 5), "num"), "k_wbatch<num>": ((0, 1, 2, 3, 4, 5), "num"), "k_wbatch<sym>": ((0, 1, 2, 3, 4, 5), "sym"),
}


def algorithmic_bytes(kind, rows, nnzA, P, nnzC):
    """Per-launch algorithmic bytes.  numeric: SURVEY.md §8(d) BYTES_ALG restricted to the rows of
    the launch = 8 rows + 16 nnzA + 8 P + 8 nnzC.  symbolic (not credited by BYTES_ALG, reported for completeness):
    rowPtr/rowIds 8 rows + A cols and two B.rowPtr reads 12 nnzA + B cols 4 P + counts 4 rows."""
    if kind == "num":
        return 8 * rows + 16 * nnzA + 8 * P + 8 * nnzC
    return 12 * rows + 12 * nnzA + 4 * P


def device_code_hashes():
    """sha256 of the kernel sources the shipped library was built from (its .buildinfo) -> {file: hash}"""
    info = os.path.join(ROOT, "sparse_matrix_with_flops_amd", "libspgemm_hip.so.buildinfo")
    out = {}
    try:
        lines = open(info).read().splitlines()
        for ln in lines[lines.index("sources sha256:") + 1:]:
            h_, name = ln.split()
            if name.endswith("_device.hpp"):
                out[name] = h_
    except (OSError, ValueError):
        pass
    return out


def traffic_for(workload, kernel, path=None):
    """PMC-derived HBM bytes per launch of `kernel` (profiles/collect.sh: separate --pmc FETCH_SIZE / WRITE_SIZE passes of
    this same command), newest round first.  -> ({raw, fetch_x2}, source) or (None, reason).
    A traffic file is only believed when it records the hashes of the kernel sources it was collected on AND they equal the
    hashes of the library in use (profiles/summarize.py writes them): bytes measured on other kernels are not reported."""
    cands = [path] if path else [os.path.join(ROOT, "profiles", f"r{r:02d}_{workload}_traffic.json") for r in (4, 3, 2, 1)]
    have = device_code_hashes()
    stale = None
    # one timer id of the library covers BOTH launches of a split bin (tables of two sizes): their traffic adds up
    parts = {"k_num_hash<1,1024>": ("k_num_hash<1,512>", "k_num_hash<1,1024>"), "k_sym_hash<1,1024>": ("k_sym_hash<1,512>", "k_sym_hash<1,1024>"),
             "k_num_hash<4,4096>": ("k_num_hash<4,2048>", "k_num_hash<4,4096>")}.get(kernel, (kernel,))
    for tj in cands:
        if tj and os.path.exists(tj):
            tjd = json.load(open(tj))
            if not have or tjd.get("device_code_sha256") != have:
                stale = stale or (f"{os.path.relpath(tj, ROOT)} was collected on other kernel sources than the library in use "
                                  "(device_code_sha256 differs or is not recorded): not reported")
                continue
            ks = tjd.get("kernels", {})
            found = [ks[p_] for p_ in parts if p_ in ks]
            if found:
                k = {f_: sum(x.get(f_, 0) for x in found) for f_ in ("hbm_bytes_raw", "hbm_bytes_fetch_x2")}
                return ({"raw": k.get("hbm_bytes_raw"), "fetch_x2": k.get("hbm_bytes_fetch_x2")},
                        f"{os.path.relpath(tj, ROOT)}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, collected "
                        "separately (not in this run) on the same kernel sources (device_code_sha256 checked)")
    return None, stale


DUMP_SEED = 20240601         # the fixed row sample of --dump-outputs
DUMP_SAMPLE_ROWS = 4096
DUMP_SAMPLE_NNZ = 2_000_000  # bound on the sampled entries: 24 MB, the whole dump stays below 64 MB at m <= 2 M


def dump_outputs(out_dir, rowPtr, colInd, values):
    """--dump-outputs: the CSR result C = (rowPtr, colInd, values) of the last timed step, as .npy files in DIR.  C itself
    is ~1.8 GB at the headline size, so the files hold
        row_nnz.npy         float64[m]  entries of every row (the structure's row lengths, exact)
        row_value_sum.npy   float64[m]  sum of every row's values, accumulated in float64
        sample_rows.npy     float64[k]  a fixed seeded sample of rows (DUMP_SEED; taken in sampled order while the
                                        entries stay within DUMP_SAMPLE_NNZ, then sorted)
        sample_rowPtr.npy   float64[k+1] offsets of the sampled rows inside the two arrays below
        sample_colInd.npy   float64     their columns, sorted inside each row (the order of a row's entries is not part
                                        of the result)
        sample_values.npy   float32     their values, in the same order"""
    os.makedirs(out_dir, exist_ok=True)
    rp = np.asarray(rowPtr, dtype=np.int64)
    m = len(rp) - 1
    lens = np.diff(rp)
    sums = np.zeros(m, dtype=np.float64)
    live = lens > 0
    if live.any():
        sums[live] = np.add.reduceat(np.asarray(values), rp[:-1][live], dtype=np.float64)
    rng = np.random.default_rng(DUMP_SEED)
    cand = rng.permutation(m)[:DUMP_SAMPLE_ROWS]
    rows = np.sort(cand[np.cumsum(lens[cand]) <= DUMP_SAMPLE_NNZ])
    idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows]) if len(rows) else np.zeros(0, dtype=np.int64)
    owner = np.repeat(np.arange(len(rows)), lens[rows])
    cols = np.asarray(colInd)[idx]
    order = np.lexsort((cols, owner))
    srp = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens[rows], out=srp[1:])
    out = {"row_nnz": lens.astype(np.float64), "row_value_sum": sums, "sample_rows": rows.astype(np.float64),
           "sample_rowPtr": srp.astype(np.float64), "sample_colInd": cols[order].astype(np.float64),
           "sample_values": np.asarray(values)[idx][order].astype(np.float32)}
    for name, arr in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), arr)


def self_launch(args):
    """--gpus N > 1 from a plain shell: start the ranks as a child torchrun (this process has made no GPU call)."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    line = None
    for ln in p.stdout.splitlines():
        if ln.startswith("{") and '"metric"' in ln:
            line = ln
    if p.returncode != 0 or line is None:
        sys.stderr.write(p.stdout[-4000:] + "\n" + p.stderr[-8000:])
        raise SystemExit(p.returncode if p.returncode != 0 else f"the {args.gpus}-rank run printed no result line")
    got = json.loads(line)
    if got.get("n_gpus") != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the process group had {got.get('n_gpus')} ranks")
    emit(line)
    raise SystemExit(0)


class Ctx:
    """what every workload needs: ranks, the process group, barriers"""

    def __init__(self, args):
        world = int(os.environ.get("WORLD_SIZE", "0"))
        if world == 0:
            if args.gpus > 1:
                self_launch(args)                            # never returns; before anything touches the GPU
            world = 1
        if world != args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.args = torch, dist, args
        self.world = world
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        from sparse_matrix_with_flops_amd import hipspgemm as hs
        self.hs = hs
        if not torch.cuda.is_available() or hs.device_count() < 1:
            raise SystemExit("bench.py needs an MI355X: the HIP SpGEMM path has no CPU fallback")
        if args.backend == "gloo":
            self.local_rank = self.local_rank % torch.cuda.device_count()
        torch.cuda.set_device(self.local_rank)
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if args.backend == "gloo":
                dist.init_process_group(backend="gloo")
            else:
                dist.init_process_group(backend="nccl", device_id=torch.device("cuda", self.local_rank))
            if dist.get_world_size() != args.gpus:
                raise SystemExit(f"--gpus {args.gpus} but the process group has {dist.get_world_size()} ranks")

    def barrier(self):
        self.torch.cuda.synchronize()
        if self.world > 1:
            self.dist.barrier()
            self.torch.cuda.synchronize()

    def reduce_max_sum(self, values):
        """-> (max over ranks, sum over ranks) of a list of floats"""
        if self.world == 1:
            return list(values), list(values)
        dev = "cuda" if self.args.backend == "nccl" else "cpu"
        tt = self.torch.tensor(values, dtype=self.torch.float64, device=dev)
        mx = tt.clone()
        self.dist.all_reduce(mx, op=self.dist.ReduceOp.MAX)
        self.dist.all_reduce(tt, op=self.dist.ReduceOp.SUM)
        return [float(x) for x in mx.tolist()], [float(x) for x in tt.tolist()]

    def all_ok(self, ok):
        """True only if every rank says so"""
        if self.world == 1:
            return bool(ok)
        mx, _ = self.reduce_max_sum([0.0 if ok else 1.0])
        return mx[0] == 0.0

    def broadcast_bytes(self, data, n):
        """rank 0's `n` bytes to everyone"""
        if self.world == 1:
            return data
        dev = "cuda" if self.args.backend == "nccl" else "cpu"
        t = self.torch.tensor(list(data) if self.rank == 0 else [0] * n, dtype=self.torch.uint8, device=dev)
        self.dist.broadcast(t, 0)
        return bytes(t.cpu().tolist())

    def finish(self):
        if self.world > 1:
            self.dist.barrier()
            self.dist.destroy_process_group()


# ----------------------------------------------------------------------------------------------------------------------
# the SpGEMM workloads
# ----------------------------------------------------------------------------------------------------------------------
class TorchRunner:
    """N = 1 (one-shot hip_gpuSpMM through dist.HipEngine) and the torch.distributed exchange for N > 1"""

    def __init__(self, ctx, host, chunks):
        from sparse_matrix_with_flops_amd.dist import HipEngine, ShardedSpGEMM
        self.ctx = ctx
        self.engine = HipEngine(ctx.local_rank, handles=chunks)
        self.engine.handle.selftest()
        self.job = ShardedSpGEMM(self.engine, host, None, chunks=chunks)
        self.P = self.job.total_flops
        self.handles = self.engine.handles[:max(1, chunks)]
        self.out = None
        self.transport = None if ctx.world == 1 else (
            "torch.distributed (%s): grouped isend/irecv pairs, sub-blocks overlapping the next one's numeric phase" % ctx.args.backend)

    def step(self, gather):
        self.out = None                                  # the consumer is done with the previous C: back to the allocator
        self.out = self.job.step(gather)

    def device_ms(self):
        return sum(h.stats()["ms_total"] for h in self.handles)

    def local_nnz(self):
        from sparse_matrix_with_flops_amd.dist import DeviceCSR
        return self.out.nnz if isinstance(self.out, DeviceCSR) else int(self.out[1].numel())

    def result_host(self):
        from sparse_matrix_with_flops_amd.dist import DeviceCSR
        if isinstance(self.out, DeviceCSR):
            return self.out.to_host()
        return tuple(x.cpu().numpy() for x in self.out)

    def local_rows(self):
        return self.job.r0, self.job.r1

    def local_row_flops(self):
        return self.engine.row_flops(self.job.A_local, self.job.B), self.job.A_local["rowPtr"].cpu().numpy().astype(np.int64)

    def release(self):
        self.out = None


class GroupRunner:
    """N > 1 behind the C ABI (dist.library_group / LibraryShardedSpGEMM): one-shard group per process
    (spgemm_hip_group_create_rank), partition, pipeline and the RCCL exchange inside the library"""

    def __init__(self, ctx, host):
        from sparse_matrix_with_flops_amd.dist import LibraryShardedSpGEMM, library_group
        self.ctx = ctx
        self.group = library_group(ctx.local_rank)
        self.sh = LibraryShardedSpGEMM(self.group, host)
        self.hA = self.sh.hA
        self.handles = [self.sh.handle]
        self.handles[0].selftest()
        self.P = None
        self.transport = "rccl inside libspgemm_hip.so (spgemm_hip_group_create_rank): grouped ncclSend/ncclRecv per peer"

    def step(self, gather):
        self.sh.step(gather)
        self.P = self.sh.total_flops

    def device_ms(self):
        return self.sh.info()["ms_compute"]

    def local_nnz(self):
        return int(self.sh.nnz)

    def result_host(self):
        c = self.sh.result_host()
        return c.rowPtr, c.colInd, c.values

    def local_rows(self):
        e = self.sh.info()["ends"]
        return e[self.ctx.rank], e[self.ctx.rank + 1]

    def local_row_flops(self):
        r0, r1 = self.local_rows()
        rp = self.hA.rowPtr.astype(np.int64)
        deg = np.diff(rp)
        cols = self.hA.colInd[rp[r0]:rp[r1]]
        f = np.zeros(r1 - r0, dtype=np.int64)
        np.add.at(f, np.repeat(np.arange(r1 - r0), deg[r0:r1]), deg[cols])
        return f, rp[r0:r1 + 1] - rp[r0]

    def release(self):
        pass


def bench_spgemm(ctx, args, wl):
    """-> the result line as a dict (rank 0; None elsewhere).  Stops the process if the parity gate fails."""
    from sparse_matrix_with_flops_amd import synth
    hs, world, rank = ctx.hs, ctx.world, ctx.rank
    t0 = time.time()
    if wl.get("gen") == "web":
        rp, ci, v = synth.webgraph_csr(wl["m"], wl["seed"])
    else:
        rp, ci, v = synth.powerlaw_csr(wl["m"], wl["seed"], wl["base"])
    m = wl["m"]
    gen_s = time.time() - t0
    host = (rp, ci, v, m, m)
    chunks = max(1, args.chunks) if world > 1 else 1
    runner, fallback = None, None
    # BENCH_FORCE_GROUP=1: rehearsal of the N>1 plumbing on one GPU (a group of ONE rank: its segment makes the round trip
    # through the library's RCCL transport to itself)
    if (world > 1 and args.backend == "nccl" and not args.torch_exchange) or os.environ.get("BENCH_FORCE_GROUP"):
        try:                                                              # (library_group asks every rank for RCCL first)
            runner = GroupRunner(ctx, host)
        except Exception as e:                                            # noqa: BLE001 -- any failure: the other transport
            fallback = f"{type(e).__name__}: {e}"
            runner = None
        if not ctx.all_ok(runner is not None):
            runner = None
            fallback = fallback or "another rank could not create its group"
            if not args.allow_torch_exchange:
                raise SystemExit(f"the library's RCCL group could not be made ({fallback}); an N>1 number has ONE provenance: "
                                 "pass --allow-torch-exchange to fall back to the torch.distributed exchange of dist.py")
        if runner is not None:                                            # and one whole step through its exchange
            ok = True
            try:
                runner.step(not args.no_gather)
            except Exception as e:                                        # noqa: BLE001
                ok, fallback = False, f"first step: {type(e).__name__}: {e}"
            if not ctx.all_ok(ok):
                runner = None
                fallback = fallback or "the first step failed on another rank"
                if not args.allow_torch_exchange:
                    raise SystemExit(f"the first step through the library's group failed ({fallback}); pass "
                                     "--allow-torch-exchange to fall back to the torch.distributed exchange of dist.py")
    if runner is None:
        runner = TorchRunner(ctx, host, chunks)

    def set_timing(mask):
        for hnd in runner.handles:
            hnd.set_kernel_timing(mask)

    gather = not args.no_gather
    for _ in range(max(1, args.warmup)):
        runner.step(gather)
    P = runner.P

    prof_avg, dom, dom_id, nprof = {}, None, None, 3
    if args.full:
        # ---- untimed profiling pass: every kernel bracketed by HIP events -> per-kernel averages, dominant kernel
        set_timing(ALL_KERNELS)
        prof_ms = {}
        for _ in range(nprof):
            runner.step(gather)
            for hnd in runner.handles:
                for kname, ms in hnd.stats()["ms_kernel"].items():
                    prof_ms[kname] = prof_ms.get(kname, 0.0) + ms
        prof_avg = {k_: v_ / nprof for k_, v_ in prof_ms.items()}
        cand = {k_: v_ for k_, v_ in prof_avg.items() if k_ in KERNEL_BINS}
        dom = max(cand, key=cand.get) if cand else None
        dom_id = next((i for i in range(hs.NKERNELS) if hs.kernel_name(i) == dom), None) if dom else None
    set_timing(ALL_KERNELS if args.time_all_kernels else ((1 << dom_id) if dom_id is not None else 0))

    # ---- timed region
    kern_ms = {}
    phase_ms = {"ms_classify": 0.0, "ms_symbolic": 0.0, "ms_scan_alloc": 0.0, "ms_numeric": 0.0, "ms_total": 0.0}
    ctx.barrier()
    t0 = time.perf_counter()
    dev_ms = 0.0
    for _ in range(args.steps):
        runner.step(gather)
        dev_ms += runner.device_ms()
        for hnd in runner.handles:
            st = hnd.stats()                           # HIP-event durations of this step's launches (handle's stream)
            for kname, ms in st["ms_kernel"].items():
                kern_ms[kname] = kern_ms.get(kname, 0.0) + ms
            for kk in phase_ms:
                phase_ms[kk] += st[kk]
    ctx.barrier()
    elapsed = time.perf_counter() - t0
    set_timing(0)

    nnz_local = runner.local_nnz()
    (elapsed, dev_ms, _), (_, _, nnz_sum) = ctx.reduce_max_sum([elapsed, dev_ms, float(nnz_local)])
    ms_per_step = elapsed * 1e3 / args.steps
    nnzC = nnz_local if (world == 1 or gather) else int(nnz_sum)
    nnzA = int(rp[-1])
    bytes_alg = synth.bytes_alg(m, nnzA, P, nnzC)
    gflops = 2.0 * P / (ms_per_step * 1e-3) / 1e9

    result = {
        "metric": "SpGEMM GFLOP/s (2*intermediate_nnz/sec), C=A*A on 1M-row CSR",
        "value": round(gflops, 3), "unit": "GFLOP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": wl["desc"], "name": wl["name"], "m": m, "nnzA": nnzA, "intermediate_nnz_P": P,
                   "nnzC": nnzC, "bytes_alg": bytes_alg,
                   "parallelism": ("single GPU" if world == 1 else f"A row-sharded by flops over {world} GPUs, B replicated, "
                                   "allgatherv of C's row segments over xGMI")},
        "rccl_ranks": (ctx.dist.get_world_size() if world > 1 else 1), "backend": (args.backend if world > 1 else None),
        "transport": runner.transport, "transport_fallback_reason": fallback,
        "output_nnz_per_s": round(nnzC / (ms_per_step * 1e-3), 1),
        # device time of the SpGEMM phases alone (max over ranks, HIP events): what the step costs without the allgatherv of C
        "compute_only": {"ms_per_step": round(dev_ms / args.steps, 4),
                         "value": round(2.0 * P / max(dev_ms / args.steps * 1e-3, 1e-12) / 1e9, 3), "unit": "GFLOP/s"},
        "gather_in_step": bool((world > 1 or isinstance(runner, GroupRunner)) and gather),
        "pipeline_bytes_alg_GBs": round(bytes_alg / (ms_per_step * 1e-3) / 1e9, 2),
        "pipeline_frac_of_hbm_peak": round(bytes_alg / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS / world, 4),
    }

    if rank == 0 and (args.full or args.dump_outputs):
        # ---- C of the last step on the host (--dump-outputs; parity gate and per-bin counts for the roofline)
        rpc, jc_h, cv_h = runner.result_host()
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, rpc, jc_h, cv_h)
    if rank == 0 and args.full:
        rpc = rpc.astype(np.int64)
        r0, r1 = runner.local_rows()
        flops_rows, rpl = runner.local_row_flops()
        cnt_rows = np.diff(rpc[r0:r1 + 1]) if (world > 1 and gather) else np.diff(rpc)
        b = bin_of(flops_rows)
        per_bin = {}
        for q in range(9):
            sel = b == q
            per_bin[q] = (int(sel.sum()), int(np.diff(rpl)[sel].sum()), int(flops_rows[sel].sum()), int(cnt_rows[sel].sum()))
        roof = None
        if dom and dom in kern_ms:
            avg_dom = kern_ms[dom] / args.steps
            bins, kind = KERNEL_BINS[dom]
            rows_ = sum(per_bin[q][0] for q in bins)
            nza_ = sum(per_bin[q][1] for q in bins)
            p_ = sum(per_bin[q][2] for q in bins)
            nzc_ = sum(per_bin[q][3] for q in bins)
            ab = algorithmic_bytes(kind, rows_, nza_, p_, nzc_)
            ach = ab / (avg_dom * 1e-3) / 1e9
            tr, tsrc = traffic_for(wl["name"], dom, args.traffic_json)
            roof = {"bound": "hbm", "kernel": dom, "avg_launch_ms": round(avg_dom, 4), "alg_bytes_per_launch": ab,
                    "achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                    # traffic: FETCH_SIZE corrected x2 as the guide prescribes for gfx950 (every fabric read request of these
                    # kernels is a 128-byte one: profiles/*tcc_counters*); the raw figure beside it
                    "traffic": (tr or {}).get("fetch_x2"), "traffic_raw": (tr or {}).get("raw"),
                    "traffic_fetch_x2": (tr or {}).get("fetch_x2"),
                    "traffic_over_alg": (round(tr["fetch_x2"] / ab, 3) if tr and tr.get("fetch_x2") else None),
                    "traffic_source": tsrc,
                    "rows": rows_, "products": p_, "nnzC": nzc_,
                    "timing": "dominant kernel: HIP events on the handle's stream inside the timed region; all_kernels_avg_ms: "
                              f"a separate untimed pass of {nprof} steps with every kernel bracketed",
                    "all_kernels_avg_ms": {k_: round(v_, 4) for k_, v_ in sorted(prof_avg.items(), key=lambda kv: -kv[1])},
                    "phases_avg_ms": {k_: round(v_ / args.steps, 4) for k_, v_ in phase_ms.items()},
                    "per_bin": {str(q): {"rows": per_bin[q][0], "nnzA": per_bin[q][1], "P": per_bin[q][2], "nnzC": per_bin[q][3]}
                                for q in range(9)}}
        result["roofline"] = roof

        # ---- parity gate (every N) + CPU baseline (N=1 only); the oracle is the checker, never the thing measured above
        from oracle import pyoracle as po
        A = po.CSRHost(rp, ci, v, m, m)
        if world == 1 and not args.no_cpu_baseline:
            ncpu = os.cpu_count() or 1
            use_ref = po.have_ref()
            times = []
            budget_t0 = time.time()
            for i in range(5):
                dt, _ = po.time_omp_spmm(A, A, use_ref)          # the C call alone, outputs freed unread
                times.append(dt)
                if time.time() - budget_t0 > 25.0 and i >= 1:
                    break
            best = float(np.median(times[1:])) if len(times) > 1 else times[0]
            threads = po.ref().ref_max_threads() if use_ref else po.lib().oracle_max_threads()
            result["cpu_baseline"] = {
                "value": round(2.0 * P / best / 1e9, 4), "unit": "GFLOP/s", "cores": int(threads),
                "kind": "reference" if use_ref else "port",
                "sample": (f"{'omp_CSR_SpMM (reference sources, oracle/_ref)' if use_ref else 'oracle_omp_spmm (C restatement of omp_CSR_SpMM)'} "
                           f"on the whole {wl['name']} matrix, stride 512, incl. per-thread scratch allocation as in the "
                           f"reference's 4-argument wrapper, {len(times)} runs (first = warm-up), median {best * 1e3:.1f} ms; "
                           f"OpenMP threads={int(threads)} of host cpus={ncpu}"),
                "ms": round(best * 1e3, 2)}
        if world == 1 and not args.no_host_api:
            # the drop-in a reference caller of CSR::*spmm gets (nlibs/CSR.cc:122-134): host arrays in, malloc()ed host
            # arrays out.  PCIe-inclusive, never `value`.
            runner.release()
            hA = hs.CSR.from_arrays(rp, ci, v, m, m)
            runs = hs.host_api_timed(hA, hA, reps=3)
            best = min(runs[1:], key=lambda r_: r_["ms_total"])          # first run: pinned slots are allocated
            result["host_api"] = {
                "entry": "hip_CSR_SpMM (host CSR in, malloc()ed host CSR out)", "ms": round(best["ms_total"], 2),
                "ms_h2d": round(best["ms_h2d"], 2), "ms_device": round(best["ms_device"], 2), "ms_d2h": round(best["ms_d2h"], 2),
                "GB_h2d": round(best["bytes_h2d"] / 1e9, 3), "GB_d2h": round(best["bytes_d2h"] / 1e9, 3),
                "d2h_GBs": round(best["bytes_d2h"] / max(best["ms_d2h"], 1e-9) / 1e6, 1),
                "GFLOPs_incl_pcie": round(2.0 * P / (best["ms_total"] * 1e-3) / 1e9, 2), "runs_ms": [round(r_["ms_total"], 1) for r_ in runs]}
        if not args.no_verify and (world == 1 or gather):
            want = po.omp_spmm(A, A)
            got = po.CSRHost(rpc, jc_h, cv_h, m, m)
            ok = np.array_equal(got.rowPtr, want.rowPtr)
            if ok:
                g2, w2 = got.canonical(), want.canonical()
                ok = np.array_equal(g2.colInd, w2.colInd)
                if ok:
                    a_, b_ = g2.values.astype(np.float64), w2.values.astype(np.float64)
                    ok = bool(np.all(np.abs(a_ - b_) <= 1e-6 * np.maximum(np.abs(a_), np.abs(b_))))
            result["parity"] = ("ok (rowPtr, sorted colInd bit-exact; values rel<=1e-6 vs CPU oracle"
                                + (f"; gathered C of {world} ranks checked on rank 0)" if world > 1 else ")")) if ok else "FAILED"
            if not ok:
                emit(json.dumps(result))
                raise SystemExit("parity gate failed")
    if rank == 0:
        result["setup"] = {"generate_s": round(gen_s, 2), "host_cpus": os.cpu_count()}
    runner.release()
    return result if rank == 0 else None


# ----------------------------------------------------------------------------------------------------------------------
# BASELINE configs[4]: the R-MCL loop
# ----------------------------------------------------------------------------------------------------------------------
def bench_rmcl(ctx, args, wl):
    """-> the result line as a dict (rank 0; None elsewhere).  A step = `iters` iterations of Mt <- prune(Mgt * Mt) from the initial Mt, device-resident (hip_rmcl_expand_prune per
    iteration: the product is never materialised).  value = 2 * (sum of the iterations' products) / t.
    N > 1: hip_gpuRmclIter_sharded over the library's group (host arrays in and out: the copies are inside the step)."""
    from oracle import pyoracle as po                       # graph construction (rmclInit restatement) + checker/baseline only
    from sparse_matrix_with_flops_amd import synth
    hs, world, rank = ctx.hs, ctx.world, ctx.rank
    m, iters = wl["m"], wl["iters"]
    t0 = time.time()
    rp, ci, v = synth.powerlaw_csr(m, wl["seed"], wl["base"])
    ri = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    Mt = po.rmcl_init(m, m, ci, ri, np.ones_like(v))        # transpose + self loops + 1/deg (nlibs/qrmcl.cc:126-134)
    gen_s = time.time() - t0
    H = hs.CSR.from_arrays(Mt.rowPtr, Mt.colInd, Mt.values, m, m)
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "golden_large.json"))).get(f"rmcl_{m}_{wl['seed']}")

    if world > 1 or os.environ.get("BENCH_FORCE_GROUP"):
        # (BENCH_FORCE_GROUP=1: rehearsal of this branch on one GPU -- a group of ONE rank, its block makes the round trip
        # through the library's RCCL transport to itself)
        # N > 1: the resident sharded loop of the library (hip_sharded_rmcl_create / run: Mgt's row blocks and the initial Mt
        # are uploaded once, a step = `iters` iterations on device arrays, the pruned blocks gathered over RCCL every iteration)
        from sparse_matrix_with_flops_amd.dist import library_group
        grp = library_group(ctx.local_rank)
        job = hs.ShardedRmcl(grp, H, H)
        for _ in range(max(1, args.warmup)):
            job.run(iters)
        ctx.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            final_nnz = job.run(iters)
        ctx.barrier()
        (elapsed,), _ = ctx.reduce_max_sum([time.perf_counter() - t0])
        per_iter_nnz = job.iter_nnz()
        # parity gate, every rank's own copy of the result (it was gathered): nnz after EVERY iteration against the
        # reference-made summary (threshold ties move a few entries), rows sum to 1, and one sampled iteration step by step
        # against the oracle (tests/helpers.assert_rmcl_step: equal rows, or rows that differ only in proven threshold ties)
        ok, why = True, ""
        if rank == 0 and args.dump_outputs:
            final = job.result(0)
            dump_outputs(args.dump_outputs, final.rowPtr, final.colInd, final.values)
        if args.full and not args.no_verify:
            final = job.result(0)
            rs = np.add.reduceat(final.values.astype(np.float64), final.rowPtr[:-1][np.diff(final.rowPtr) > 0])
            ok = bool(np.allclose(rs, 1.0, atol=1e-5)) and int(final.nnz) == final_nnz
            why = "" if ok else "rows of the final Mt do not sum to 1"
            if ok and gold:
                for it_, n_ in enumerate(per_iter_nnz):
                    g_ = gold["per_iter"][it_]["nnz"]
                    if abs(n_ - g_) > 5e-4 * g_ + 4096:
                        ok, why = False, f"nnz after iteration {it_ + 1}: {n_} vs reference {g_}"
                        break
            if ok and rank == 0:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from helpers import assert_rmcl_step
                k_ = min(iters, 7)                                       # a late iteration: a small product for the CPU oracle
                job.run(k_ - 1)
                before = job.result(0)
                job.run(1, restart=False)                                # ONE step of the same trajectory
                after = job.result(0)
                try:
                    assert_rmcl_step(po.CSRHost(after.rowPtr, after.colInd, after.values, m, m), Mt,
                                     po.CSRHost(before.rowPtr, before.colInd, before.values, m, m), what=f"iteration {k_} over {world} GPUs")
                except AssertionError as e:
                    ok, why = False, f"iteration {k_} differs from the oracle's step: {str(e)[:300]}"
            elif ok:                                                     # the other ranks run the same two loops (collectives)
                k_ = min(iters, 7)
                job.run(k_ - 1)
                job.run(1, restart=False)
        ok_all = ctx.all_ok(ok)
        result = None
        if rank == 0:
            ms = elapsed * 1e3 / args.steps
            Ptot = sum(p_["P"] for p_ in gold["per_iter"][:iters]) if gold and "P" in gold["per_iter"][0] else None
            result = {
                "metric": "R-MCL loop wall time (operands resident, hip_sharded_rmcl_run)", "value": round(ms, 3), "unit": "ms",
                "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": False,
                "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "config": {"workload": wl["desc"], "name": wl["name"], "m": m, "iterations": iters,
                           "parallelism": f"Mgt row-sharded by flops over {world} GPUs, Mt replicated, pruned blocks packed into "
                                          "their slice of the next Mt and gathered over RCCL every iteration; device-resident"},
                "GFLOPs": (round(2.0 * Ptot / (ms * 1e-3) / 1e9, 3) if Ptot else None),
                "per_iteration_nnz": per_iter_nnz, "final_nnz": int(final_nnz),
                "golden_final_nnz": (gold["per_iter"][iters - 1]["nnz"] if gold else None),
                "parity": (None if not args.full else
                           "ok (nnz after every iteration within the threshold-tie drift of the reference summary; rows sum to 1; "
                           "one iteration checked step by step against the oracle)" if ok_all else f"FAILED: {why}"),
                "roofline": None, "cpu_baseline": None}
        job.close()
        grp.close()
        if not ok_all:
            if rank == 0:
                emit(json.dumps(result))
            raise SystemExit("parity gate failed")
        return result

    h = hs.Handle(0)
    h.selftest()
    G_ = H.toGpuCSR()

    def loop(cur, collect):
        per = []
        for _ in range(iters):
            i_, j_, c_, nn = hs.rmcl_expand_prune_raw(h, G_.rowPtr, G_.colInd, G_.values, G_.nnz, cur.rowPtr, cur.colInd,
                                                      cur.values, cur.nnz, m, m, m)
            st = h.stats()
            if collect:
                per.append({"P": st["total_flops"], "nnz_in": cur.nnz, "kept": nn, "ms": st["ms_total"],
                            "ms_kernel": st["ms_kernel"]})
            else:
                per.append(st["ms_total"])
            cur.deviceDispose()
            cur = hs.CSR(c_, j_, i_, m, m, nn, True)
        return cur, per

    # Profiling pass: one iteration per call (hip_rmcl_expand_prune) for the per-iteration products, kept entries and kernel
    # times.  Timed region: the loop as ONE call on device arrays (hip_gpuRmclIter_device -- what hip_gpuRmclIter runs
    # between its upload and download; Mt stays in the epilogues' layout between iterations).  Mgt and the first Mt are
    # resident before the clock starts and are not modified.
    start = H.toGpuCSR()
    for _ in range(max(1, args.warmup)):
        hs.gpuRmclIter_device(iters, G_, start, h).deviceDispose()
    h.set_kernel_timing(ALL_KERNELS)
    fin, per = loop(H.toGpuCSR(), True)
    fin.deviceDispose()
    h.set_kernel_timing(0)
    P_total = sum(p_["P"] for p_ in per)
    ctx.barrier()
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        if last is not None:
            last.deviceDispose()
        last = hs.gpuRmclIter_device(iters, G_, start, h)
    ctx.barrier()
    elapsed = time.perf_counter() - t0
    ms_per_step = elapsed * 1e3 / args.steps
    # beside it: the same loop as one hip_rmcl_expand_prune call per iteration (Mt packed every time), for the record
    per_call_ms = None
    if args.full:
        nside = min(args.steps, 5)
        copies = [H.toGpuCSR() for _ in range(nside)]         # synchronous uploads
        t1 = time.perf_counter()
        for c_ in copies:
            fin, _ = loop(c_, False)
            fin.deviceDispose()
        per_call_ms = (time.perf_counter() - t1) * 1e3 / nside
    final = last.toCpuCSR() if (args.full or args.dump_outputs) else None
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, final.rowPtr, final.colInd, final.values)
    last.deviceDispose()
    start.deviceDispose()
    G_.deviceDispose()
    # the call the reference's driver makes: host CSRs in, host CSR out (upload + the loop above + download), never `value`
    host_api = None
    if args.full and not args.no_host_api:
        hs.gpuRmclIter(iters, H, H)
        t2 = time.perf_counter()
        nh = 3
        for _ in range(nh):
            R_ = hs.gpuRmclIter(iters, H, H)
        host_api = {"entry": "hip_gpuRmclIter (gpuRmclIter, nlibs/gpus/gpu_csr_kernel.cu:281-311): host arrays in and out",
                    "ms": round((time.perf_counter() - t2) * 1e3 / nh, 3), "final_nnz": int(R_.nnz),
                    "devices_used": int(hs.lib().spgemm_hip_rmcl_devices_used())}

    # algorithmic bytes of one fused iteration: read A (= Mgt) and the gathered B entries, write only what survives the prune
    nnzA = int(Mt.nnz)
    it_bytes = [8 * (m + 1) + 16 * nnzA + 8 * p_["P"] + 8 * p_["kept"] for p_ in per]
    kern_tot = {}
    for p_ in per:
        for k_, ms in p_["ms_kernel"].items():
            kern_tot[k_] = kern_tot.get(k_, 0.0) + ms
    cand = {k_: v_ for k_, v_ in kern_tot.items() if k_.startswith("k_num")}
    dom = max(cand, key=cand.get) if cand else None
    peak_it = max(range(iters), key=lambda i: per[i]["P"])
    result = {
        "metric": "SpGEMM GFLOP/s (2*intermediate_nnz/sec), R-MCL loop (expand + prune fused)",
        "value": round(2.0 * P_total / (ms_per_step * 1e-3) / 1e9, 3), "unit": "GFLOP/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": wl["desc"], "name": wl["name"], "m": m, "nnz_Mt0": nnzA, "iterations": iters,
                   "products_per_step": P_total, "parallelism": "single GPU"},
        "loop_one_call_per_iteration_ms": (round(per_call_ms, 3) if per_call_ms is not None else None),
        "host_api": host_api,
        "per_iteration": [{"P": p_["P"], "nnz_in": p_["nnz_in"], "kept": p_["kept"], "ms": round(p_["ms"], 3),
                           "alg_GBs": round(b_ / (p_["ms"] * 1e-3) / 1e9, 1)} for p_, b_ in zip(per, it_bytes)],
        "pipeline_bytes_alg_GBs": round(sum(it_bytes) / (ms_per_step * 1e-3) / 1e9, 2),
        "pipeline_frac_of_hbm_peak": round(sum(it_bytes) / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        "roofline": {"bound": "hbm",
                     "kernel": f"hip_rmcl_expand_prune, iteration {peak_it + 1} (largest product); dominant numeric kernel of the loop: {dom}",
                     "avg_launch_ms": round(per[peak_it]["ms"], 4), "alg_bytes_per_launch": it_bytes[peak_it],
                     "achieved": round(it_bytes[peak_it] / (per[peak_it]["ms"] * 1e-3) / 1e9, 2), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(it_bytes[peak_it] / (per[peak_it]["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                     "traffic": None,
                     "alg_bytes": "8(m+1) + 16 nnz(Mgt) + 8 P + 8 kept: the product is never written, only what survives the prune",
                     "loop_kernels_ms": {k_: round(v_, 3) for k_, v_ in sorted(kern_tot.items(), key=lambda kv: -kv[1])}},
    }
    if args.full and not args.no_verify:
        rs = np.add.reduceat(final.values.astype(np.float64), final.rowPtr[:-1][np.diff(final.rowPtr) > 0])
        ok = bool(np.allclose(rs, 1.0, atol=1e-5))
        if gold and iters <= len(gold["per_iter"]):                        # reference-made per-iteration summary
            g_last = gold["per_iter"][iters - 1]
            ok = ok and abs(int(final.nnz) - g_last["nnz"]) <= 5e-4 * g_last["nnz"] + 4096
            result["golden"] = {"final_nnz": int(final.nnz), "reference_final_nnz": g_last["nnz"],
                                "source": "tests/golden/golden_large.json (reference-pinned kernels, cross-checked against RMCL(file, 10, OMP))"}
        result["parity"] = (f"ok (rows sum to 1; nnz after {iters} iterations within the threshold-tie drift of the reference "
                            "summary; step-by-step parity: tests/test_gpu_rmcl.py)") if ok else "FAILED"
        if not ok:
            emit(json.dumps(result))
            raise SystemExit("parity gate failed")
    if args.full and not args.no_cpu_baseline:
        if po.have_ref():                                                  # the reference's own multi-threaded loop, 2 iterations
            sample_it = min(2, iters)
            _, dt = po.ref_mt_rmcl(Mt, Mt, sample_it, opt=1)
            Ps = sum(p_["P"] for p_ in per[:sample_it])
            threads = po.ref().ref_max_threads()
            result["cpu_baseline"] = {"value": round(2.0 * Ps / dt / 1e9, 4), "unit": "GFLOP/s", "cores": int(threads), "kind": "reference",
                                      "sample": f"mtRmclIter(OMP, stride 512) of the reference (oracle/_ref) on the first {sample_it} "
                                                f"iterations of the same graph ({Ps} products), {dt * 1e3:.0f} ms", "ms": round(dt * 1e3, 1)}
        else:
            t1 = time.perf_counter()
            po.rmcl_iters(Mt, Mt, 1)
            dt = time.perf_counter() - t1
            result["cpu_baseline"] = {"value": round(2.0 * per[0]["P"] / dt / 1e9, 4), "unit": "GFLOP/s", "cores": 1, "kind": "port",
                                      "sample": f"seqRmclIter restatement, first iteration only ({per[0]['P']} products), {dt * 1e3:.0f} ms",
                                      "ms": round(dt * 1e3, 1)}
    result["setup"] = {"generate_s": round(gen_s, 2), "host_cpus": os.cpu_count()}
    h.close()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="synth_1m_16", choices=sorted(WORKLOADS))
    ap.add_argument("--no-verify", action="store_true", help="skip the parity gate against the CPU oracle")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-host-api", action="store_true", help="skip the host-array entry point (hip_CSR_SpMM) timing")
    ap.add_argument("--no-gather", action="store_true",
                    help="N>1: leave C row-sharded (no allgatherv inside the timed step)")
    ap.add_argument("--chunks", type=int, default=4,
                    help="N>1, torch.distributed exchange: sub-blocks per rank whose exchange overlaps the next one's numeric phase")
    ap.add_argument("--torch-exchange", action="store_true",
                    help="N>1: exchange through torch.distributed (dist.py) instead of the library's own RCCL group")
    ap.add_argument("--allow-torch-exchange", action="store_true",
                    help="N>1: if the library's group cannot be made or its first step fails, fall back to the torch.distributed "
                         "exchange instead of stopping (default: stop -- an N>1 number has one provenance)")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="default workload, N=1: skip the short runs of the other BASELINE configs attached as other_workloads")
    ap.add_argument("--traffic-json", default=None, help="profiles/*.json with PMC-derived HBM bytes per kernel")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (one GPU per rank).  gloo: rehearsal of the N>1 path on a box with fewer GPUs "
                         "than ranks (ranks share devices; transport over host memory; not a performance number)")
    ap.add_argument("--time-all-kernels", action="store_true",
                    help="keep the HIP events of every kernel inside the timed region (diagnostic; costs ~3 %% of a step)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: profiling pass + roofline, parity gate, CPU baseline, host-array "
                         "entry point, other workloads (each still subject to its --no-* switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed to DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()
    if args.dump_outputs and args.gpus > 1 and args.no_gather:
        raise SystemExit("--dump-outputs needs the gathered C: drop --no-gather")
    os.environ.setdefault("OMP_NUM_THREADS", str(os.cpu_count() or 1))   # cpu_baseline: all host threads
    protect_stdout()
    ctx = Ctx(args)

    def run(name, a):
        wl = dict(WORKLOADS[name], name=name)
        return bench_rmcl(ctx, a, wl) if wl.get("gen") == "rmcl" else bench_spgemm(ctx, a, wl)

    result = run(args.workload, args)
    if args.full and args.workload == "synth_1m_16" and ctx.world == 1 and not args.no_other_workloads and result is not None:
        # The driver times ONE line: the other BASELINE configs ride on it as short runs (5 steps each, parity gate on, no
        # cpu baseline / host-api timing), so that their numbers are the driver's measurements too and not builder claims.
        # `value` stays the headline's.  (configs[3] = 1M/32 sharded over 2-8 GPUs is the N>1 run of this same script.)
        import copy
        others = {}
        for name in ("synth_256k_16", "web_google_surrogate", "rmcl_500k"):
            a = copy.copy(args)
            a.steps, a.warmup, a.no_cpu_baseline, a.no_host_api, a.dump_outputs = 5, 2, True, True, None
            t0 = time.time()
            r = run(name, a)
            roof = r.get("roofline") or {}
            others[name] = {"ms_per_step": r["ms_per_step"], "value": r["value"], "unit": r["unit"],
                            "pipeline_frac_of_hbm_peak": r.get("pipeline_frac_of_hbm_peak"),
                            "dominant_kernel": roof.get("kernel"), "dominant_avg_launch_ms": roof.get("avg_launch_ms"),
                            "dominant_frac": roof.get("frac"), "parity": (r.get("parity") or "")[:160],
                            "steps": a.steps, "wall_s": round(time.time() - t0, 1)}
        result["other_workloads"] = others
    if result is not None:
        emit(json.dumps(result))
    ctx.finish()


if __name__ == "__main__":
    main()
