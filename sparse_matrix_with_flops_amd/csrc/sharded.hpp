// sharded.hpp — multi-GPU behind the C ABI (included at the end of spgemm_hip.hip; uses its pool / handle / phases).
//
// The reference has no multi-device code; its GPU R-MCL entry is ONE call,
// gpuRmclIter(maxIter, Mgt, Mt) (nlibs/gpus/gpu_csr_kernel.cu:281-311, dispatched from nlibs/qrmcl.cc:149-152), and its
// CPU path cuts rows into contiguous ranges of equal flops for its threads (arrayEqualPartition64,
// nlibs/tools/util.cc:123-135, used by flops_omp_CSR_SpMM, nlibs/flops_csr_kernel.cc:59-63).  Here the same cut is made
// across GPUs: shard s owns the rows [ends[s], ends[s+1]) of A (or of Mgt), B (or Mt) is replicated, every shard runs the
// single-GPU pipeline on its block with its own handle/stream, and the row segments of the result are exchanged so that
// every shard ends up with the whole C (allgatherv).  For R-MCL each shard prunes its rows BEFORE the exchange: what
// crosses xGMI is the pruned matrix, which is also the next iteration's replicated operand.
//
// A GROUP is a set of shards.  In-process (spgemm_hip_group_create): all shards live in this process, one per device
// -- or several LOGICAL shards on one device, which is how the whole path is tested on a one-GPU box.  Multi-process
// (spgemm_hip_group_create_rank): one local shard per process, one process per GPU, wired with an RCCL unique id that
// the caller distributes (torchrun / MPI / a file).  Transports of the exchange:
//   RCCL  grouped ncclSend/ncclRecv per peer (xGMI is a full mesh: every segment travels its own link, no ring).  The
//         library loads librccl at run time (dlopen; no link-time dependency).  Shards must sit on distinct devices;
//         a group of one rank exchanges with itself through RCCL (exercises the transport on one GPU).
//   PEER  hipMemcpyPeerAsync between the shards' devices (in-process only; plain d2d copies when shards share a device).
//   HOST  staged through pinned host memory (in-process only; SURVEY.md 8e "replicas only" fallback).
#pragma once
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <condition_variable>
#include <functional>
#include <string>
#include <thread>

namespace {

struct RcclApi {
  void* so = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  std::string why;
  bool ok = false;
};

RcclApi& rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    const char* env = getenv("SPGEMM_RCCL_LIB");
    // absolute paths first: a process that also hosts PyTorch already has the wheel's own librccl (linked against the
    // wheel's HIP runtime) loaded under the same soname; this library talks to the system runtime and wants the system RCCL
    const char* cand[] = {env, "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so", "librccl.so.1", "librccl.so"};
    for (const char* c : cand) {
      if (!c || !c[0]) continue;
      api.so = dlopen(c, RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND);   // DEEPBIND: its own symbols before another loaded RCCL's
      if (api.so) break;
      api.why = dlerror();
    }
    if (!api.so) return;
#define SMF_SYM(field, name)                                                                  \
  api.field = reinterpret_cast<decltype(api.field)>(dlsym(api.so, name));                     \
  if (!api.field) { api.why = std::string("missing symbol ") + name; return; }
    SMF_SYM(GetUniqueId, "ncclGetUniqueId") SMF_SYM(CommInitRank, "ncclCommInitRank") SMF_SYM(CommDestroy, "ncclCommDestroy")
    SMF_SYM(GroupStart, "ncclGroupStart") SMF_SYM(GroupEnd, "ncclGroupEnd") SMF_SYM(Send, "ncclSend") SMF_SYM(Recv, "ncclRecv")
    SMF_SYM(AllGather, "ncclAllGather") SMF_SYM(GetErrorString, "ncclGetErrorString")
#undef SMF_SYM
    api.ok = true;
  });
  return api;
}

#define NCCLCHK(expr)                                                                                              \
  do {                                                                                                             \
    ncclResult_t r__ = (expr);                                                                                     \
    if (r__ != ncclSuccess) return fail(SPGEMM_ERR_HIP, "%s failed: %s", #expr, rccl().GetErrorString(r__));       \
  } while (0)

__global__ void k_offset_copy(int n, const int* __restrict__ src, int off, int* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i] + off;
}

}  // namespace

struct spgemm_shard {
  int device = 0;
  int grank = 0;                                  // global rank of this shard
  spgemm_handle* h = nullptr;
  ncclComm_t comm = nullptr;
  DevBlock<long long> dSizes;                     // nranks int64 on the device (multi-process size exchange)
  PinBlock<long long> hSizes;                     // pinned twin
  std::string err;                                // message of a failure inside this shard's worker thread
  int rc = 0;
};

// One worker thread per local shard, started with the first phase that has several shards to run and kept until the
// group goes (round 3 created and joined N threads per phase: twice per R-MCL iteration, where an iteration is a
// fraction of a millisecond per GPU).  A phase = one function run for every shard index, concurrently.
struct ShardWorkers {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable go, done;
  std::function<void(int)> job;
  unsigned long long gen = 0;
  int pending = 0;
  bool quit = false;
  void start(int n) {
    for (int i = 0; i < n; ++i)
      th.emplace_back([this, i] {
        unsigned long long seen = 0;
        for (;;) {
          std::function<void(int)> fn;
          {
            std::unique_lock<std::mutex> lk(mu);
            go.wait(lk, [&] { return quit || gen != seen; });
            if (quit) return;
            seen = gen;
            fn = job;
          }
          fn(i);
          {
            std::lock_guard<std::mutex> lk(mu);
            if (--pending == 0) done.notify_all();
          }
        }
      });
  }
  void run(int n, const std::function<void(int)>& fn) {
    if (th.empty()) start(n);
    std::unique_lock<std::mutex> lk(mu);
    job = fn;
    pending = n;
    ++gen;
    go.notify_all();
    done.wait(lk, [&] { return pending == 0; });
  }
  void stop() {
    { std::lock_guard<std::mutex> lk(mu); quit = true; }
    go.notify_all();
    for (auto& t : th) t.join();
    th.clear();
  }
};

struct spgemm_group {
  int nranks = 0;                                 // shards of the whole job
  int transport = SPGEMM_XCHG_PEER;
  std::vector<spgemm_shard> sh;                   // LOCAL shards (all of them in-process, one in multi-process mode)
  ShardWorkers workers;
  bool all_local() const { return (int)sh.size() == nranks; }
};

// ------------------------------------------------------------------------------------------------
// group life cycle
// ------------------------------------------------------------------------------------------------
static int group_init_comms(spgemm_group* g, const ncclUniqueId& id) {
  RcclApi& R = rccl();
  if (!R.ok) return fail(SPGEMM_ERR_HIP, "RCCL is not available: %s", R.why.c_str());
  NCCLCHK(R.GroupStart());
  for (auto& s : g->sh) {
    HIPCHK(hipSetDevice(s.device));
    ncclResult_t r = R.CommInitRank(&s.comm, g->nranks, id, s.grank);
    if (r != ncclSuccess) { R.GroupEnd(); return fail(SPGEMM_ERR_HIP, "ncclCommInitRank(rank %d of %d) failed: %s", s.grank, g->nranks, R.GetErrorString(r)); }
  }
  NCCLCHK(R.GroupEnd());
  clear_stale_hip_error();                         // (RCCL's device probing leaves errors in the thread's slot)
  return SPGEMM_OK;
}

static int group_make_shards(spgemm_group* g) {
  for (auto& s : g->sh) {
    CHK(spgemm_hip_create(&s.h, s.device));
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(s.dSizes.reserve((size_t)g->nranks));
    HIPCHK(s.hSizes.reserve((size_t)g->nranks));
  }
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_group_destroy(spgemm_group* g) {
  if (!g) return SPGEMM_OK;
  g->workers.stop();
  for (auto& s : g->sh) {
    hipSetDevice(s.device);
    if (s.comm && rccl().ok) rccl().CommDestroy(s.comm);
    spgemm_hip_destroy(s.h);
  }
  delete g;
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_group_create(spgemm_group** out, int nshards, const int* devices, int transport) {
  if (!out) return fail(SPGEMM_ERR_ARG, "group out-pointer is null");
  *out = nullptr;
  if (nshards < 1 || nshards > 64) return fail(SPGEMM_ERR_ARG, "nshards=%d out of range [1,64]", nshards);
  if (transport < SPGEMM_XCHG_AUTO || transport > SPGEMM_XCHG_HOST) return fail(SPGEMM_ERR_ARG, "unknown transport %d", transport);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SPGEMM_ERR_NODEVICE, "no HIP device visible: libspgemm_hip has no CPU fallback");
  spgemm_group* g = new spgemm_group();
  g->nranks = nshards;
  g->sh.resize((size_t)nshards);
  bool distinct = true;
  for (int i = 0; i < nshards; ++i) {
    const int d = devices ? devices[i] : i % ndev;
    if (d < 0 || d >= ndev) { delete g; return fail(SPGEMM_ERR_ARG, "shard %d: device %d out of range [0,%d)", i, d, ndev); }
    g->sh[i].device = d;
    g->sh[i].grank = i;
    for (int j = 0; j < i; ++j) distinct = distinct && g->sh[j].device != d;
  }
  if (transport == SPGEMM_XCHG_RCCL && !distinct) { delete g; return fail(SPGEMM_ERR_ARG, "the RCCL transport needs every shard on its own device"); }
  if (transport == SPGEMM_XCHG_AUTO) transport = (distinct && nshards > 1 && rccl().ok) ? SPGEMM_XCHG_RCCL : SPGEMM_XCHG_PEER;
  g->transport = transport;
  int rc = group_make_shards(g);
  if (rc == SPGEMM_OK && transport == SPGEMM_XCHG_RCCL) {
    RcclApi& R = rccl();
    if (!R.ok) rc = fail(SPGEMM_ERR_HIP, "RCCL is not available: %s", R.why.c_str());
    else {
      ncclUniqueId id;
      ncclResult_t r = R.GetUniqueId(&id);
      if (r != ncclSuccess) rc = fail(SPGEMM_ERR_HIP, "ncclGetUniqueId failed: %s", R.GetErrorString(r));
      else rc = group_init_comms(g, id);
    }
  }
  if (rc) { spgemm_hip_group_destroy(g); return rc; }
  *out = g;
  return SPGEMM_OK;
}

// SPGEMM_OK when librccl could be loaded into this process (every rank of a multi-process job asks before any of them
// enters ncclCommInitRank, where a missing peer means waiting forever)
extern "C" int spgemm_hip_rccl_available(void) {
  RcclApi& R = rccl();
  if (!R.ok) return fail(SPGEMM_ERR_HIP, "RCCL is not available: %s", R.why.c_str());
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_unique_id(void* id128) {
  if (!id128) return fail(SPGEMM_ERR_ARG, "id buffer is null");
  static_assert(sizeof(ncclUniqueId) == SPGEMM_UNIQUE_ID_BYTES, "ncclUniqueId is 128 bytes");
  RcclApi& R = rccl();
  if (!R.ok) return fail(SPGEMM_ERR_HIP, "RCCL is not available: %s", R.why.c_str());
  ncclUniqueId id;
  NCCLCHK(R.GetUniqueId(&id));
  memcpy(id128, &id, sizeof(id));
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_group_create_rank(spgemm_group** out, int nranks, int rank, int device, const void* id128) {
  if (!out) return fail(SPGEMM_ERR_ARG, "group out-pointer is null");
  *out = nullptr;
  if (nranks < 1 || rank < 0 || rank >= nranks || !id128) return fail(SPGEMM_ERR_ARG, "bad rank %d of %d / null id", rank, nranks);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SPGEMM_ERR_NODEVICE, "no HIP device visible: libspgemm_hip has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(SPGEMM_ERR_ARG, "device %d out of range [0,%d)", device, ndev);
  spgemm_group* g = new spgemm_group();
  g->nranks = nranks;
  g->transport = SPGEMM_XCHG_RCCL;
  g->sh.resize(1);
  g->sh[0].device = device;
  g->sh[0].grank = rank;
  int rc = group_make_shards(g);
  if (rc == SPGEMM_OK) {
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    rc = group_init_comms(g, id);
  }
  if (rc) { spgemm_hip_group_destroy(g); return rc; }
  *out = g;
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_group_info(const spgemm_group* g, int* nranks, int* nlocal, int* transport) {
  if (!g) return fail(SPGEMM_ERR_ARG, "null group");
  if (nranks) *nranks = g->nranks;
  if (nlocal) *nlocal = (int)g->sh.size();
  if (transport) *transport = g->transport;
  return SPGEMM_OK;
}

// ------------------------------------------------------------------------------------------------
// helpers shared by the sharded SpGEMM and the sharded R-MCL
// ------------------------------------------------------------------------------------------------
// arrayEqualPartition64 (nlibs/tools/util.cc:123-135): prefix = exclusive scan of the per-row flops, prefix[n] = total;
// part p owns rows [ends[p], ends[p+1]); every part but the last gets at least one row while rows remain.
static void equal_partition64(const std::vector<long long>& prefix, int parts, std::vector<int>& ends) {
  const int n = (int)prefix.size() - 1;
  const long long total = prefix[n];
  const long long chunk = (total + parts - 1) / parts;
  ends.assign((size_t)parts + 1, 0);
  int now = 0;
  for (int i = 0; i < parts - 1; ++i) {
    const long long target = std::min<long long>((long long)(i + 1) * chunk, total);
    const int upper = (int)(std::upper_bound(prefix.begin() + now, prefix.begin() + n + 1, target) - prefix.begin());
    int e = std::max(upper - 1, now + 1);
    e = std::min(e, n);
    ends[i + 1] = e;
    now = e;
  }
  ends[parts] = n;
}

static void host_row_flops_prefix(const int* IA, const int* JA, const int* IB, int m, std::vector<long long>& prefix) {
  prefix.assign((size_t)m + 1, 0);
  for (int i = 0; i < m; ++i) {
    long long f = 0;
    for (int p = IA[i]; p < IA[i + 1]; ++p) f += IB[JA[p] + 1] - IB[JA[p]];
    prefix[i + 1] = prefix[i] + f;
  }
}

// run fn(local shard index) for every local shard, concurrently when there are several; collects the first failure
template <class F>
static int for_each_shard(spgemm_group* g, F&& fn) {
  const int n = (int)g->sh.size();
  auto body = [&](int i) {
    spgemm_shard& s = g->sh[i];
    s.rc = fn(i);
    s.err = s.rc ? spgemm_hip_last_error() : "";
  };
  if (n == 1) body(0);
  else g->workers.run(n, body);
  for (int i = 0; i < n; ++i)
    if (g->sh[i].rc) return fail(g->sh[i].rc, "shard %d (device %d): %s", g->sh[i].grank, g->sh[i].device, g->sh[i].err.c_str());
  return SPGEMM_OK;
}

static int upload_csr(int device, const int* I, const int* J, const float* V, int r0, int r1, int cols, DevCSR* out) {
  HIPCHK(hipSetDevice(device));
  const int rows = r1 - r0;
  const int base = I[r0], nnz = I[r1] - base;
  out->rows = rows; out->cols = cols; out->nnz = nnz;
  HIPCHK(out->I.alloc((size_t)rows + 1));
  HIPCHK(out->alloc_entries(nnz));
  std::vector<int> rp((size_t)rows + 1);
  for (int i = 0; i <= rows; ++i) rp[i] = I[r0 + i] - base;
  HIPCHK(hipMemcpy(out->I, rp.data(), sizeof(int) * ((size_t)rows + 1), hipMemcpyHostToDevice));
  if (nnz > 0) {
    HIPCHK(hipMemcpy(out->J, J + base, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(out->V, V + base, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice));
  }
  return SPGEMM_OK;
}

// per-rank entry counts -> every rank knows all of them.  In-process: they are all in this process's memory.
// Multi-process: one ncclAllGather of an int64 per rank.  A rank whose local phase FAILED enters the exchange all the same,
// with -1: a rank that returned before the collective would leave every other rank waiting in it forever; this way all of
// them see the sentinel and leave the step with an error together (any_failed below).
static int exchange_sizes(spgemm_group* g, const std::vector<long long>& localCounts, std::vector<long long>& all) {
  all.assign((size_t)g->nranks, 0);
  if (g->all_local()) {
    for (size_t i = 0; i < g->sh.size(); ++i) all[(size_t)g->sh[i].grank] = localCounts[i];
    return SPGEMM_OK;
  }
  RcclApi& R = rccl();
  spgemm_shard& s = g->sh[0];
  HIPCHK(hipSetDevice(s.device));
  s.hSizes[0] = localCounts[0];
  HIPCHK(hipMemcpyAsync(s.dSizes + s.grank, s.hSizes, sizeof(long long), hipMemcpyHostToDevice, s.h->stream));
  NCCLCHK(R.AllGather(s.dSizes + s.grank, s.dSizes, 1, ncclInt64, s.comm, s.h->stream));
  HIPCHK(hipMemcpyAsync(s.hSizes, s.dSizes, sizeof(long long) * (size_t)g->nranks, hipMemcpyDeviceToHost, s.h->stream));
  HIPCHK(hipStreamSynchronize(s.h->stream));
  for (int r = 0; r < g->nranks; ++r) all[(size_t)r] = s.hSizes[r];
  return SPGEMM_OK;
}

static int any_failed(const std::vector<long long>& all) {
  for (size_t r = 0; r < all.size(); ++r) if (all[r] < 0) return (int)r;
  return -1;
}
// multi-process groups: one more tiny exchange before a data collective, carrying only "my part is ready" (0) or "I failed" (-1)
static int vote_ready(spgemm_group* g, int localRc, const char* what) {
  if (g->all_local()) return localRc;
  const std::string msg = localRc ? spgemm_hip_last_error() : "";
  std::vector<long long> mine(1, localRc ? -1 : 0), all;
  CHK(exchange_sizes(g, mine, all));
  const int bad = any_failed(all);
  if (localRc) return fail(localRc, "%s", msg.c_str());
  if (bad >= 0) return fail(SPGEMM_ERR_INTERNAL, "rank %d failed %s: no exchange", bad, what);
  return SPGEMM_OK;
}

// The allgatherv.  Every local shard holds full-size arrays gI[m+1], gJ[total], gV[total] in which ITS OWN segment is
// already in place: rows [ends[r], ends[r+1]) of gI (global offsets; the last rank also wrote gI[m]) and entries
// [offs[r], offs[r+1]) of gJ / gV.  After the call every shard holds every segment.
struct GatherView { int* gI; int* gJ; float* gV; };
static int allgatherv_segments(spgemm_group* g, const std::vector<int>& ends, const std::vector<long long>& offs,
                               int m, const std::vector<GatherView>& view) {
  const int G = g->nranks;
  auto rows_of = [&](int r) { return (size_t)(ends[r + 1] - ends[r]) + (r == G - 1 ? 1u : 0u); };   // the last rank carries gI[m]
  auto cnt_of = [&](int r) { return (size_t)(offs[r + 1] - offs[r]); };
  (void)m;
  if (g->transport == SPGEMM_XCHG_RCCL) {
    RcclApi& R = rccl();
    if (G == 1) {
      // a group of one rank has nobody to exchange with; its segment makes the round trip through RCCL all the same
      // (ncclSend to itself, ncclRecv into scratch, scratch copied back over the segment), so that a one-GPU box
      // exercises the transport and a broken one shows up as a wrong C
      spgemm_shard& s = g->sh[0];
      const GatherView& v = view[0];
      HIPCHK(hipSetDevice(s.device));
      hipStream_t st = s.h->stream;
      DevBuf<int> tI, tJ;
      DevBuf<float> tV;
      if (tI.alloc(std::max<size_t>(rows_of(0), 1)) != hipSuccess || tJ.alloc(std::max<size_t>(cnt_of(0), 1)) != hipSuccess ||
          tV.alloc(std::max<size_t>(cnt_of(0), 1)) != hipSuccess)
        return fail(SPGEMM_ERR_HIP, "scratch allocation for the self exchange failed");
      ncclResult_t r = R.GroupStart();
      if (r == ncclSuccess && rows_of(0)) r = R.Send(v.gI, rows_of(0), ncclInt32, 0, s.comm, s.h->stream);
      if (r == ncclSuccess && rows_of(0)) r = R.Recv(tI, rows_of(0), ncclInt32, 0, s.comm, s.h->stream);
      if (r == ncclSuccess && cnt_of(0)) r = R.Send(v.gJ, cnt_of(0), ncclInt32, 0, s.comm, s.h->stream);
      if (r == ncclSuccess && cnt_of(0)) r = R.Recv(tJ, cnt_of(0), ncclInt32, 0, s.comm, s.h->stream);
      if (r == ncclSuccess && cnt_of(0)) r = R.Send(v.gV, cnt_of(0), ncclFloat32, 0, s.comm, s.h->stream);
      if (r == ncclSuccess && cnt_of(0)) r = R.Recv(tV, cnt_of(0), ncclFloat32, 0, s.comm, s.h->stream);
      const ncclResult_t r2 = R.GroupEnd();
      if (r != ncclSuccess || r2 != ncclSuccess)
        return drained(st, fail(SPGEMM_ERR_HIP, "RCCL self exchange failed: %s", R.GetErrorString(r != ncclSuccess ? r : r2)));
      if (hipMemcpyAsync(v.gI, tI, sizeof(int) * rows_of(0), hipMemcpyDeviceToDevice, s.h->stream) != hipSuccess ||
          hipMemcpyAsync(v.gJ, tJ, sizeof(int) * cnt_of(0), hipMemcpyDeviceToDevice, s.h->stream) != hipSuccess ||
          hipMemcpyAsync(v.gV, tV, sizeof(float) * cnt_of(0), hipMemcpyDeviceToDevice, s.h->stream) != hipSuccess ||
          hipStreamSynchronize(s.h->stream) != hipSuccess)
        return drained(st, fail(SPGEMM_ERR_HIP, "RCCL self exchange: copy back failed: %s", hipGetErrorString(hipGetLastError())));
      return SPGEMM_OK;
    }
    NCCLCHK(R.GroupStart());
    for (size_t li = 0; li < g->sh.size(); ++li) {
      spgemm_shard& s = g->sh[li];
      const GatherView& v = view[li];
      const int me = s.grank;
      HIPCHK(hipSetDevice(s.device));
      for (int p = 0; p < G; ++p) {
        if (p == me) continue;
        // my segment to p, p's segment from p: three messages per peer and direction, all inside ONE group, so RCCL
        // runs them concurrently -- every pair of GPUs has its own xGMI link
        ncclResult_t r = ncclSuccess;
        if (r == ncclSuccess && rows_of(me)) r = R.Send(v.gI + ends[me], rows_of(me), ncclInt32, p, s.comm, s.h->stream);
        if (r == ncclSuccess && cnt_of(me)) r = R.Send(v.gJ + offs[me], cnt_of(me), ncclInt32, p, s.comm, s.h->stream);
        if (r == ncclSuccess && cnt_of(me)) r = R.Send(v.gV + offs[me], cnt_of(me), ncclFloat32, p, s.comm, s.h->stream);
        if (r == ncclSuccess && rows_of(p)) r = R.Recv(v.gI + ends[p], rows_of(p), ncclInt32, p, s.comm, s.h->stream);
        if (r == ncclSuccess && cnt_of(p)) r = R.Recv(v.gJ + offs[p], cnt_of(p), ncclInt32, p, s.comm, s.h->stream);
        if (r == ncclSuccess && cnt_of(p)) r = R.Recv(v.gV + offs[p], cnt_of(p), ncclFloat32, p, s.comm, s.h->stream);
        if (r != ncclSuccess) { R.GroupEnd(); return fail(SPGEMM_ERR_HIP, "ncclSend/ncclRecv failed: %s", R.GetErrorString(r)); }
      }
    }
    NCCLCHK(R.GroupEnd());
    for (auto& s : g->sh) { HIPCHK(hipSetDevice(s.device)); HIPCHK(hipStreamSynchronize(s.h->stream)); }
    return SPGEMM_OK;
  }
  if (!g->all_local()) return fail(SPGEMM_ERR_ARG, "a multi-process group exchanges over RCCL only");
  if (g->transport == SPGEMM_XCHG_PEER) {
    for (size_t d = 0; d < g->sh.size(); ++d) {          // pull: the destination's stream copies from every source
      spgemm_shard& dst = g->sh[d];
      HIPCHK(hipSetDevice(dst.device));
      for (size_t q = 0; q < g->sh.size(); ++q) {
        if (q == d) continue;
        spgemm_shard& src = g->sh[q];
        const int r = src.grank;
        auto cp = [&](void* to, const void* from, size_t bytes) -> hipError_t {
          if (!bytes) return hipSuccess;
          if (src.device == dst.device) return hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, dst.h->stream);
          return hipMemcpyPeerAsync(to, dst.device, from, src.device, bytes, dst.h->stream);
        };
        HIPCHK(cp(view[d].gI + ends[r], view[q].gI + ends[r], rows_of(r) * sizeof(int)));
        HIPCHK(cp(view[d].gJ + offs[r], view[q].gJ + offs[r], cnt_of(r) * sizeof(int)));
        HIPCHK(cp(view[d].gV + offs[r], view[q].gV + offs[r], cnt_of(r) * sizeof(float)));
      }
    }
    for (auto& s : g->sh) { HIPCHK(hipSetDevice(s.device)); HIPCHK(hipStreamSynchronize(s.h->stream)); }
    return SPGEMM_OK;
  }
  // HOST: every segment once to pinned host memory, then to every other shard
  size_t need = 0;
  for (int r = 0; r < G; ++r) need = std::max(need, std::max(rows_of(r) * sizeof(int), cnt_of(r) * sizeof(float)));
  PinBlock<char> stage;
  HIPCHK(stage.reserve(std::max<size_t>(need, 16)));
  auto bounce = [&](size_t q, int which) -> int {
    spgemm_shard& src = g->sh[q];
    const int r = src.grank;
    const size_t bytes = which == 0 ? rows_of(r) * sizeof(int) : cnt_of(r) * 4;
    if (!bytes) return SPGEMM_OK;
    auto at = [&](const GatherView& v) -> char* {
      return which == 0 ? (char*)(v.gI + ends[r]) : which == 1 ? (char*)(v.gJ + offs[r]) : (char*)(v.gV + offs[r]);
    };
    HIPCHK(hipSetDevice(src.device));
    HIPCHK(hipMemcpy(stage, at(view[q]), bytes, hipMemcpyDeviceToHost));
    for (size_t d = 0; d < g->sh.size(); ++d) {
      if (d == q) continue;
      HIPCHK(hipSetDevice(g->sh[d].device));
      HIPCHK(hipMemcpy(at(view[d]), stage, bytes, hipMemcpyHostToDevice));
    }
    return SPGEMM_OK;
  };
  int rc = SPGEMM_OK;
  for (size_t q = 0; q < g->sh.size() && !rc; ++q)
    for (int which = 0; which < 3 && !rc; ++which) rc = bounce(q, which);
  return rc;
}

// ------------------------------------------------------------------------------------------------
// sharded SpGEMM job: operands resident, one step = SpGEMM on every shard + allgatherv of C
// ------------------------------------------------------------------------------------------------
struct spgemm_sharded {
  spgemm_group* g = nullptr;
  int m = 0, k = 0, n = 0;
  bool sameB = false;
  std::vector<int> ends;                          // row cut, nranks+1
  long long totalP = 0;
  struct Local {
    DevCSR A;                                     // this shard's row block of A
    DevCSR B;                                     // replica of B
    DevBuf<int> lIC;                              // local rowPtr of the block (m_s + 1)
    DevBuf<int> gI, gJ; DevBuf<float> gV;         // gathered C (or the block alone when not gathered)
    size_t capC = 0;
    long long nnz = 0;                            // entries the arrays hold after the last step
    bool gathered = false;
  };
  std::vector<Local> loc;
  float ms_compute = 0.f, ms_exchange = 0.f;      // last step: slowest local shard's device time; wall time of the exchange
};

extern "C" int hip_sharded_spmm_destroy(spgemm_sharded* job) {
  if (!job) return SPGEMM_OK;
  for (size_t i = 0; i < job->loc.size(); ++i) {
    hipSetDevice(job->g->sh[i].device);
    hipStreamSynchronize(job->g->sh[i].h->stream);   // (a step whose symbolic phase failed may have left kernels queued)
    job->loc[i] = spgemm_sharded::Local();
  }
  delete job;
  return SPGEMM_OK;
}

extern "C" int hip_sharded_spmm_create(spgemm_group* g, const int* IA, const int* JA, const float* A, int nnzA,
                                       const int* IB, const int* JB, const float* B, int nnzB, int m, int k, int n,
                                       spgemm_sharded** out) {
  if (!out) return fail(SPGEMM_ERR_ARG, "job out-pointer is null");
  *out = nullptr;
  if (!g) return fail(SPGEMM_ERR_ARG, "null group");
  if (m < 0 || k < 0 || n < 0) return fail(SPGEMM_ERR_ARG, "negative dimension");
  CHK(check_common(IA, JA, A, nnzA, "A"));
  const bool same = !IB || (IB == IA && JB == JA && B == A);
  if (same) { IB = IA; JB = JA; B = A; nnzB = nnzA; if (m != k) return fail(SPGEMM_ERR_ARG, "B omitted but A is not square"); }
  CHK(check_common(IB, JB, B, nnzB, "B"));
  CHK(validate_host_csr(IA, JA, m, k, nnzA, "A"));
  if (!same) CHK(validate_host_csr(IB, JB, k, n, nnzB, "B"));
  spgemm_sharded* job = new spgemm_sharded();
  job->g = g; job->m = m; job->k = k; job->n = n; job->sameB = same;
  std::vector<long long> prefix;
  host_row_flops_prefix(IA, JA, IB, m, prefix);
  job->totalP = prefix[(size_t)m];
  equal_partition64(prefix, g->nranks, job->ends);
  job->loc.resize(g->sh.size());
  int rc = for_each_shard(g, [&](int i) -> int {
    spgemm_shard& s = g->sh[i];
    auto& L = job->loc[i];
    const int r0 = job->ends[s.grank], r1 = job->ends[s.grank + 1];
    CHK(upload_csr(s.device, IA, JA, A, r0, r1, k, &L.A));
    CHK(upload_csr(s.device, IB, JB, B, 0, k, n, &L.B));
    HIPCHK(L.lIC.alloc((size_t)(r1 - r0) + 1));
    HIPCHK(L.gI.alloc((size_t)m + 1));
    CHK(ws_ensure(s.h, r1 - r0));
    return SPGEMM_OK;
  });
  if (rc) { hip_sharded_spmm_destroy(job); return rc; }
  *out = job;
  return SPGEMM_OK;
}

static int ensure_cap(spgemm_sharded::Local& L, size_t entries) {
  if (entries <= L.capC && L.gJ) return SPGEMM_OK;
  L.gJ.reset(); L.gV.reset(); L.capC = 0;
  const size_t cap = entries + entries / 16 + 1024;
  HIPCHK(L.gJ.alloc(cap));
  HIPCHK(L.gV.alloc(cap));
  L.capC = cap;
  return SPGEMM_OK;
}

extern "C" int hip_sharded_spmm_step(spgemm_sharded* job, int gather, long long* nnzC, long long* totalP) {
  if (!job) return fail(SPGEMM_ERR_ARG, "null job");
  spgemm_group* g = job->g;
  const int G = g->nranks;
  std::vector<long long> localNnz(g->sh.size(), -1), all;
  // phase 1 on every shard: classification + symbolic of its block (a shard that fails keeps its -1)
  const int rc1 = for_each_shard(g, [&](int i) -> int {
    spgemm_shard& s = g->sh[i];
    auto& L = job->loc[i];
    HIPCHK(hipSetDevice(s.device));
    int nz = 0;
    CHK(symbolic_phase(s.h, L.A.I, L.A.J, L.A.nnz, L.B.I, L.B.J, L.A.rows, job->k, job->n, nullptr, L.lIC, &nz));
    localNnz[i] = nz;
    return SPGEMM_OK;
  });
  const std::string msg1 = rc1 ? spgemm_hip_last_error() : "";
  if (gather && G > 1 && !g->all_local()) {
    CHK(exchange_sizes(g, localNnz, all));             // always entered: the other ranks are in it
    if (rc1) return fail(rc1, "%s", msg1.c_str());
    const int bad = any_failed(all);
    if (bad >= 0) return fail(SPGEMM_ERR_INTERNAL, "rank %d failed its symbolic phase: step abandoned on every rank", bad);
  } else {
    if (rc1) return fail(rc1, "%s", msg1.c_str());
    all.assign((size_t)G, 0);
    for (size_t i = 0; i < g->sh.size(); ++i) all[(size_t)g->sh[i].grank] = localNnz[i];
  }
  std::vector<long long> offs((size_t)G + 1, 0);
  for (int r = 0; r < G; ++r) offs[(size_t)r + 1] = offs[(size_t)r] + all[(size_t)r];
  const bool doGather = gather != 0;
  const long long total = doGather ? offs[(size_t)G] : 0;
  if (doGather && total > 0x7fffffffLL) return fail(SPGEMM_ERR_OVERFLOW, "nnz(C)=%lld does not fit int32 CSR", total);
  // phase 2: numeric straight into the shard's slice of the gathered arrays; rowPtr with the global offset
  const int rc2 = for_each_shard(g, [&](int i) -> int {
    spgemm_shard& s = g->sh[i];
    auto& L = job->loc[i];
    HIPCHK(hipSetDevice(s.device));
    const long long off = doGather ? offs[(size_t)s.grank] : 0;
    CHK(ensure_cap(L, (size_t)std::max<long long>(doGather ? total : localNnz[i], 1)));
    CHK(numeric_phase(s.h, L.A.I, L.A.J, L.A.V.p, L.B.I, L.B.J, L.B.V.p, L.A.rows, job->n, L.lIC, L.gJ.p + off, L.gV.p + off));
    const int r0 = doGather ? job->ends[s.grank] : 0;
    const int cnt = L.A.rows + ((!doGather || s.grank == G - 1) ? 1 : 0);
    clear_stale_hip_error();
    if (cnt > 0) hipLaunchKernelGGL(k_offset_copy, dim3(cdiv(cnt, 256)), dim3(256), 0, s.h->stream, cnt, L.lIC.p, (int)off, L.gI.p + r0);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s.h->stream) != hipSuccess)
      return drained(s.h->stream, fail(SPGEMM_ERR_HIP, "sharded SpGEMM: row pointer of the block: %s", hipGetErrorString(hipGetLastError())));
    L.nnz = doGather ? total : localNnz[i];
    L.gathered = doGather;
    return SPGEMM_OK;
  });
  if (doGather && G > 1) CHK(vote_ready(g, rc2, "its numeric phase"));   // (multi-process: nobody enters the allgatherv alone)
  else if (rc2) return rc2;
  float ms = 0.f;
  for (auto& s : g->sh) ms = std::max(ms, s.h->stats.ms_total);
  job->ms_compute = ms;
  job->ms_exchange = 0.f;
  if (doGather && (G > 1 || g->transport == SPGEMM_XCHG_RCCL)) {
    std::vector<GatherView> view(g->sh.size());
    for (size_t i = 0; i < g->sh.size(); ++i) view[i] = GatherView{job->loc[i].gI, job->loc[i].gJ, job->loc[i].gV};
    const auto t0 = std::chrono::steady_clock::now();
    CHK(allgatherv_segments(g, job->ends, offs, job->m, view));
    job->ms_exchange = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  long long sum = 0;
  for (long long v : all) sum += v;
  if (nnzC) *nnzC = doGather ? total : sum;           // not gathered: the entries held by this process's shards
  if (totalP) *totalP = job->totalP;
  return SPGEMM_OK;
}

extern "C" int hip_sharded_spmm_result(spgemm_sharded* job, int local_shard, int** IC, int** JC, float** C, int* nnzC, int* rows) {
  if (!job || !IC || !JC || !C || !nnzC) return fail(SPGEMM_ERR_ARG, "null argument");
  if (local_shard < 0 || local_shard >= (int)job->loc.size()) return fail(SPGEMM_ERR_ARG, "local shard %d out of range", local_shard);
  auto& L = job->loc[(size_t)local_shard];
  HIPCHK(hipSetDevice(job->g->sh[(size_t)local_shard].device));
  const int nr = L.gathered ? job->m : L.A.rows;
  const size_t nz = (size_t)L.nnz;
  int* hI = (int*)malloc(sizeof(int) * ((size_t)nr + 1));
  int* hJ = (int*)malloc(sizeof(int) * std::max<size_t>(nz, 1));
  float* hV = (float*)malloc(sizeof(float) * std::max<size_t>(nz, 1));
  if (!hI || !hJ || !hV) { free(hI); free(hJ); free(hV); return fail(SPGEMM_ERR_NOMEM, "host malloc of C failed"); }
  if (hipMemcpy(hI, L.gI, sizeof(int) * ((size_t)nr + 1), hipMemcpyDeviceToHost) != hipSuccess ||
      (nz && hipMemcpy(hJ, L.gJ, sizeof(int) * nz, hipMemcpyDeviceToHost) != hipSuccess) ||
      (nz && hipMemcpy(hV, L.gV, sizeof(float) * nz, hipMemcpyDeviceToHost) != hipSuccess)) {
    free(hI); free(hJ); free(hV);
    return fail(SPGEMM_ERR_HIP, "copy of C to the host failed: %s", hipGetErrorString(hipGetLastError()));
  }
  *IC = hI; *JC = hJ; *C = hV; *nnzC = (int)nz;
  if (rows) *rows = nr;
  return SPGEMM_OK;
}

// the handle local shard `local_shard` computes with (per-call statistics, per-kernel timing); owned by the group
extern "C" spgemm_handle* hip_sharded_spmm_handle(spgemm_sharded* job, int local_shard) {
  if (!job || local_shard < 0 || local_shard >= (int)job->loc.size()) return nullptr;
  return job->g->sh[(size_t)local_shard].h;
}

extern "C" int hip_sharded_spmm_info(spgemm_sharded* job, int* ends, float* ms_compute, float* ms_exchange) {
  if (!job) return fail(SPGEMM_ERR_ARG, "null job");
  if (ends) for (size_t i = 0; i < job->ends.size(); ++i) ends[i] = job->ends[i];
  if (ms_compute) *ms_compute = job->ms_compute;
  if (ms_exchange) *ms_exchange = job->ms_exchange;
  return SPGEMM_OK;
}

// ------------------------------------------------------------------------------------------------
// sharded R-MCL: Mgt's row blocks stay resident per shard, Mt is replicated; per iteration every shard expands and
// PRUNES its own rows, then the pruned blocks are gathered into the next replicated Mt.
//
// Round 4: a JOB keeps the operands resident (create / run / result / destroy), so that a caller -- bench.py at N > 1 --
// times the loop and not the upload and download around it.  An iteration on a shard is the fused step in its BLOCK form
// (rmcl_expand_prune_core, RMCL_BLOCK: the kept entries stay in the scratch rows, their counts are scanned), one exchange
// of the block sizes, and ONE pass that packs the scratch rows straight into the shard's slice of the next Mt
// (k_rmcl_move; row pointers shifted by the slice's offset) -- no packed copy of the block, no device-to-device copies, no
// per-iteration allocation once the two Mt buffers have grown to size -- and the allgatherv.  Waits per iteration: the
// size of the block (the host needs it for the exchange) and the end of the allgatherv.
// ------------------------------------------------------------------------------------------------
struct spgemm_sharded_rmcl {
  spgemm_group* g = nullptr;
  int rows = 0, cols = 0;
  std::vector<int> ends;
  struct MtBuf { DevBuf<int> I, J; DevBuf<float> V; size_t cap = 0; int nnz = 0;
                 CsrView view() const { return {I, J, V, nnz}; } };
  struct Local {
    DevCSR Mg;                                    // this shard's row block of Mgt
    DevCSR Mt0;                                   // replica of the initial Mt (every run starts from it)
    MtBuf buf[2];                                 // the replicated Mt of the current / next iteration
    DevCSR blk;                                   // one iteration's block between its two phases: block form (nnz = kept
  };                                              // entries), or packed when the step gave up on the fused form
  std::vector<Local> loc;
  int cur = -1;                                   // buf index holding the result of the last run, -1 = the initial Mt
  std::vector<long long> iterNnz;                 // nnz(Mt) after every iteration of the last run
};

extern "C" int hip_sharded_rmcl_destroy(spgemm_sharded_rmcl* job) {
  if (!job) return SPGEMM_OK;
  for (size_t i = 0; i < job->loc.size(); ++i) {
    const int dev = job->g->sh[i].device;
    hipSetDevice(dev);
    hipStreamSynchronize(job->g->sh[i].h->stream);
    job->loc[i] = spgemm_sharded_rmcl::Local();   // every block of the shard goes back, behind the drained stream
  }
  delete job;
  return SPGEMM_OK;
}

extern "C" int hip_sharded_rmcl_create(spgemm_group* g, int rows, int cols, const int* gIA, const int* gJA, const float* gA,
                                       int gnnz, const int* tIA, const int* tJA, const float* tA, int tnnz,
                                       spgemm_sharded_rmcl** out) {
  if (!out) return fail(SPGEMM_ERR_ARG, "job out-pointer is null");
  *out = nullptr;
  if (!g) return fail(SPGEMM_ERR_ARG, "null group");
  if (rows < 0 || cols != rows) return fail(SPGEMM_ERR_ARG, "R-MCL needs a square matrix");
  CHK(check_common(gIA, gJA, gA, gnnz, "Mgt"));
  CHK(check_common(tIA, tJA, tA, tnnz, "Mt"));
  CHK(validate_host_csr(gIA, gJA, rows, cols, gnnz, "Mgt"));
  CHK(validate_host_csr(tIA, tJA, rows, cols, tnnz, "Mt"));
  spgemm_sharded_rmcl* job = new spgemm_sharded_rmcl();
  job->g = g; job->rows = rows; job->cols = cols;
  // the cut: flops of the first expansion (the blocks stay where they are for all iterations)
  std::vector<long long> prefix;
  host_row_flops_prefix(gIA, gJA, tIA, rows, prefix);
  equal_partition64(prefix, g->nranks, job->ends);
  job->loc.resize(g->sh.size());
  int rc = for_each_shard(g, [&](int i) -> int {
    spgemm_shard& s = g->sh[i];
    CHK(upload_csr(s.device, gIA, gJA, gA, job->ends[s.grank], job->ends[s.grank + 1], cols, &job->loc[i].Mg));
    CHK(upload_csr(s.device, tIA, tJA, tA, 0, rows, cols, &job->loc[i].Mt0));
    return SPGEMM_OK;
  });
  if (rc) { hip_sharded_rmcl_destroy(job); return rc; }
  *out = job;
  return SPGEMM_OK;
}

static int rmcl_ensure_buf(spgemm_sharded_rmcl::MtBuf& b, int rows, size_t entries) {
  if (!b.I) HIPCHK(b.I.alloc((size_t)rows + 1));
  if (entries <= b.cap && b.J) return SPGEMM_OK;
  b.J.reset(); b.V.reset(); b.cap = 0;
  const size_t cap = entries + entries / 8 + 1024;
  HIPCHK(b.J.alloc(cap));
  HIPCHK(b.V.alloc(cap));
  b.cap = cap;
  return SPGEMM_OK;
}

// maxIter iterations from the initial Mt (fromCurrent: from the result of the previous run -- how a caller checks ONE step of
// a trajectory); the result stays on every shard (hip_sharded_rmcl_result brings it to the host)
static int sharded_rmcl_run(spgemm_sharded_rmcl* job, int maxIter, int* nnzOut, bool fromCurrent) {
  if (!job || maxIter < 0) return fail(SPGEMM_ERR_ARG, "null job / negative iteration count");
  spgemm_group* g = job->g;
  const int G = g->nranks, m = job->rows, cols = job->cols;
  const std::vector<int>& ends = job->ends;
  if (!fromCurrent) job->iterNnz.clear();
  int cur = fromCurrent ? job->cur : -1;
  auto abandon = [&](int rc) {                     // a failed iteration: drain, give the blocks back, no result
    const std::string msg = spgemm_hip_last_error();
    for (size_t i = 0; i < job->loc.size(); ++i) {
      hipSetDevice(g->sh[i].device);
      hipStreamSynchronize(g->sh[i].h->stream);
      job->loc[i].blk.reset();
    }
    job->cur = -1;
    return fail(rc, "%s", msg.c_str());
  };
  for (int it = 0; it < maxIter; ++it) {
    std::vector<long long> localNnz(g->sh.size(), -1), all;
    // phase A: expand + prune of the shard's rows, kept entries left in the scratch rows, their counts scanned
    const int rcA = for_each_shard(g, [&](int i) -> int {
      spgemm_shard& s = g->sh[i];
      auto& L = job->loc[i];
      HIPCHK(hipSetDevice(s.device));
      const CsrView Mt = cur < 0 ? L.Mt0.view() : L.buf[cur].view();
      // (no rows / no products / product too large: a packed block comes back, L.blk.packed())
      CHK(rmcl_expand_prune_core(s.h, L.Mg.view(), Mt, L.Mg.rows, cols, cols, RMCL_BLOCK, &L.blk));
      localNnz[i] = L.blk.nnz;
      return SPGEMM_OK;
    });
    const std::string msgA = rcA ? spgemm_hip_last_error() : "";
    if (!g->all_local()) {
      if (int rc = exchange_sizes(g, localNnz, all)) return abandon(rc);   // always entered: the other ranks are in it
      if (rcA) { fail(rcA, "%s", msgA.c_str()); return abandon(rcA); }
      const int bad = any_failed(all);
      if (bad >= 0) { fail(SPGEMM_ERR_INTERNAL, "rank %d failed iteration %d: loop abandoned on every rank", bad, it); return abandon(SPGEMM_ERR_INTERNAL); }
    } else {
      if (rcA) { fail(rcA, "%s", msgA.c_str()); return abandon(rcA); }
      all.assign((size_t)G, 0);
      for (size_t i = 0; i < g->sh.size(); ++i) all[(size_t)g->sh[i].grank] = localNnz[i];
    }
    std::vector<long long> offs((size_t)G + 1, 0);
    for (int r = 0; r < G; ++r) offs[(size_t)r + 1] = offs[(size_t)r] + all[(size_t)r];
    const long long total = offs[(size_t)G];
    if (total > 0x7fffffffLL) { fail(SPGEMM_ERR_OVERFLOW, "nnz(Mt)=%lld does not fit int32 CSR", total); return abandon(SPGEMM_ERR_OVERFLOW); }
    const int nxt = cur < 0 ? 0 : 1 - cur;
    std::vector<GatherView> view(g->sh.size());
    // phase B: the block packed straight into its slice of the next Mt, row pointers shifted by the slice's offset
    const int rcB = for_each_shard(g, [&](int i) -> int {
      spgemm_shard& s = g->sh[i];
      auto& L = job->loc[i];
      const DevCSR& K = L.blk;
      HIPCHK(hipSetDevice(s.device));
      auto& N = L.buf[nxt];
      CHK(rmcl_ensure_buf(N, m, (size_t)std::max<long long>(total, 1)));
      N.nnz = (int)total;
      const long long off = offs[(size_t)s.grank];
      const int ml = L.Mg.rows;
      const int cnt = ml + (s.grank == G - 1 ? 1 : 0);
      hipStream_t st = s.h->stream;
      clear_stale_hip_error();
      const int* ptr = K.packed() ? K.I : K.len;      // row pointer of the packed block (ml + 1 entries)
      if (cnt > 0) hipLaunchKernelGGL(k_offset_copy, dim3(cdiv(cnt, 256)), dim3(256), 0, st, cnt, ptr, (int)off, N.I.p + ends[s.grank]);
      if (K.nnz > 0 && K.packed()) {
        HIPCHK(hipMemcpyAsync(N.J.p + off, K.J, sizeof(int) * (size_t)K.nnz, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(N.V.p + off, K.V, sizeof(float) * (size_t)K.nnz, hipMemcpyDeviceToDevice, st));
      } else if (K.nnz > 0) {
        const RowLanes rl = row_lanes(s.h, ml, K.nnz);
        RMCL_ROWS(k_rmcl_move, float, rl, st, ml, K.I.p, K.len.p, K.J.p, K.V.p, N.J.p + off, N.V.p + off);
      }
      HIPCHK(hipGetLastError());
      // RCCL runs on this same stream, behind the move; the other transports read the slice from other streams
      if (g->transport != SPGEMM_XCHG_RCCL) HIPCHK(hipStreamSynchronize(st));
      view[i] = GatherView{N.I, N.J, N.V};
      return SPGEMM_OK;
    });
    if (int rc = vote_ready(g, rcB, "to place its block")) return abandon(rc);
    if (G > 1 || g->transport == SPGEMM_XCHG_RCCL) {
      if (int rc = allgatherv_segments(g, ends, offs, m, view)) return abandon(rc);   // returns with every stream drained
    } else {
      for (auto& s : g->sh) { hipSetDevice(s.device); if (hipStreamSynchronize(s.h->stream) != hipSuccess) { fail(SPGEMM_ERR_HIP, "sharded R-MCL: iteration %d", it); return abandon(SPGEMM_ERR_HIP); } }
    }
    for (auto& L : job->loc) L.blk.reset();           // the streams are idle: the scratch blocks go back to the pool
    cur = nxt;
    job->iterNnz.push_back(total);
  }
  job->cur = cur;
  if (nnzOut) *nnzOut = cur < 0 ? job->loc[0].Mt0.nnz : job->loc[0].buf[cur].nnz;
  return SPGEMM_OK;
}

extern "C" int hip_sharded_rmcl_run(spgemm_sharded_rmcl* job, int maxIter, int* nnzOut) {
  return sharded_rmcl_run(job, maxIter, nnzOut, false);
}
extern "C" int hip_sharded_rmcl_continue(spgemm_sharded_rmcl* job, int iters, int* nnzOut) {
  return sharded_rmcl_run(job, iters, nnzOut, true);
}

// nnz(Mt) after every iteration of the last run (the per-iteration check of bench.py against the reference-made summary)
extern "C" int hip_sharded_rmcl_iter_nnz(const spgemm_sharded_rmcl* job, long long* out, int cap) {
  if (!job || (cap > 0 && !out)) return fail(SPGEMM_ERR_ARG, "null argument");
  const int n = (int)job->iterNnz.size();
  for (int i = 0; i < n && i < cap; ++i) out[i] = job->iterNnz[(size_t)i];
  return n;
}

extern "C" int hip_sharded_rmcl_info(const spgemm_sharded_rmcl* job, int* ends) {
  if (!job) return fail(SPGEMM_ERR_ARG, "null job");
  if (ends) for (size_t i = 0; i < job->ends.size(); ++i) ends[i] = job->ends[i];
  return SPGEMM_OK;
}

// the result of the last run as held by local shard `local_shard`: malloc()ed host arrays (every shard holds the whole Mt)
extern "C" int hip_sharded_rmcl_result(spgemm_sharded_rmcl* job, int local_shard, int** oIA, int** oJA, float** oA, int* onnz) {
  if (!job || !oIA || !oJA || !oA || !onnz) return fail(SPGEMM_ERR_ARG, "null argument");
  if (local_shard < 0 || local_shard >= (int)job->loc.size()) return fail(SPGEMM_ERR_ARG, "local shard %d out of range", local_shard);
  auto& L = job->loc[(size_t)local_shard];
  HIPCHK(hipSetDevice(job->g->sh[(size_t)local_shard].device));
  const CsrView Mt = job->cur < 0 ? L.Mt0.view() : L.buf[job->cur].view();
  const int nz = Mt.nnz;
  const int rows = job->rows;
  int* hI = (int*)malloc(sizeof(int) * ((size_t)rows + 1));
  int* hJ = (int*)malloc(sizeof(int) * (size_t)std::max(nz, 1));
  float* hA = (float*)malloc(sizeof(float) * (size_t)std::max(nz, 1));
  if (!hI || !hJ || !hA) { free(hI); free(hJ); free(hA); return fail(SPGEMM_ERR_NOMEM, "host malloc failed"); }
  if (hipMemcpy(hI, Mt.I, sizeof(int) * ((size_t)rows + 1), hipMemcpyDeviceToHost) != hipSuccess ||
      (nz && hipMemcpy(hJ, Mt.J, sizeof(int) * (size_t)nz, hipMemcpyDeviceToHost) != hipSuccess) ||
      (nz && hipMemcpy(hA, Mt.V, sizeof(float) * (size_t)nz, hipMemcpyDeviceToHost) != hipSuccess)) {
    free(hI); free(hJ); free(hA);
    return fail(SPGEMM_ERR_HIP, "copy of Mt to the host failed: %s", hipGetErrorString(hipGetLastError()));
  }
  *oIA = hI; *oJA = hJ; *oA = hA; *onnz = nz;
  return SPGEMM_OK;
}

// gpuRmclIter over a group, host arrays in and out (nlibs/gpus/gpu_csr_kernel.cu:281-311): create + run + result + destroy
extern "C" int hip_gpuRmclIter_sharded(spgemm_group* g, int maxIter, int rows, int cols,
                                       const int* gIA, const int* gJA, const float* gA, int gnnz,
                                       const int* tIA, const int* tJA, const float* tA, int tnnz,
                                       int** oIA, int** oJA, float** oA, int* onnz) {
  if (!oIA || !oJA || !oA || !onnz) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  if (maxIter < 0) return fail(SPGEMM_ERR_ARG, "R-MCL needs maxIter >= 0");
  spgemm_sharded_rmcl* job = nullptr;
  CHK(hip_sharded_rmcl_create(g, rows, cols, gIA, gJA, gA, gnnz, tIA, tJA, tA, tnnz, &job));
  int rc = hip_sharded_rmcl_run(job, maxIter, nullptr);
  if (!rc) rc = hip_sharded_rmcl_result(job, 0, oIA, oJA, oA, onnz);
  const std::string msg = rc ? spgemm_hip_last_error() : "";
  hip_sharded_rmcl_destroy(job);
  if (rc) return fail(rc, "%s", msg.c_str());
  return SPGEMM_OK;
}
