// spgemm_hip.hip — host side of libspgemm_hip.so: the extern "C" boundary declared in
// include/spgemm_hip.h, the workspace/handle, and the launch sequence of the kernels in
// spgemm_device.hpp.  gfx950 only.  There is NO CPU fallback in this library: without a HIP device
// every entry point fails with SPGEMM_ERR_NODEVICE / SPGEMM_ERR_HIP.
#include "spgemm_device.hpp"
#include "spgemm_f64_device.hpp"
#include "rmcl_rows_device.hpp"
#include "chain_device.hpp"
#include "../../include/spgemm_hip.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <sys/mman.h>
#include <thread>
#include <type_traits>
#include <vector>

using namespace smf;

static_assert(NBINS == SPGEMM_NBINS, "bin count of the kernels and of the C ABI differ");
#ifdef SMF_ABLATE
constexpr bool kAblate = true;      // diagnostic build: the ablated float kernels break their invariants on purpose
#else
constexpr bool kAblate = false;
#endif

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIPCHK(expr)                                                                               \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess)                                                                         \
      return fail(SPGEMM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)

#define CHK(expr)                                                                                  \
  do {                                                                                             \
    int rc__ = (expr);                                                                             \
    if (rc__ != SPGEMM_OK) return rc__;                                                            \
  } while (0)

extern "C" const char* spgemm_hip_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------
// caching device allocator behind spgemm_hip_malloc/free (the role cudaMalloc/cudaFree play in
// CSR::toGpuCSR/deviceDispose, nlibs/CSR.cc:342-379).  Freed blocks are kept (bounded) and reused,
// so the per-call allocation of C costs a map lookup in steady state instead of a hipMalloc.
// ------------------------------------------------------------------------------------------------
namespace {
// Blocks are cached PER DEVICE: a block freed on device 0 is never handed to an allocation made for device 1.
// INVARIANT the reuse relies on: every entry point of this library returns only after the work it queued has completed
// (hipStreamSynchronize on the handle's stream before the function returns), so a block that comes back through
// spgemm_hip_free / release() is idle; callers that queue their own work on such a block must finish it before freeing
// (the same rule cudaFree imposes implicitly by synchronising).  SPGEMM_POOL_CHECK=1 makes release() synchronise the
// device first (debugging aid for foreign streams).
// One entry point queues work and returns before it has completed: an iteration of hip_gpuRmclIter_device that leaves Mt
// unpacked.  The loop keeps the blocks those kernels read out of the pool until a later wait has covered them.
struct DevPool {
  struct Blk { size_t size; int dev; };
  std::mutex mu;
  std::map<void*, Blk> live;                                   // ptr -> rounded size, owning device
  std::map<int, std::multimap<size_t, void*>> free_blocks;     // device -> rounded size -> ptr
  size_t cached_bytes = 0;
  bool check = false;
  static constexpr size_t kMaxCached = size_t(64) << 30;   // 64 GiB of 288 GiB HBM
  DevPool() { const char* e = getenv("SPGEMM_POOL_CHECK"); check = e && e[0] == '1'; }
  static size_t round_up(size_t b) {
    if (b < 512) b = 512;
    if (b <= (size_t(1) << 20)) return (b + 511) & ~size_t(511);
    const size_t g = size_t(2) << 20;            // 2 MiB granules for big blocks
    return (b + g - 1) / g * g;
  }
  hipError_t alloc(void** p, size_t bytes) {
    const size_t r = round_up(bytes);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    {
      std::lock_guard<std::mutex> lk(mu);
      auto& fb = free_blocks[dev];
      auto it = fb.lower_bound(r);
      // best fit, and a cached block up to 4x the request is still better than a hipMalloc (tens of ms for GB-sized
      // blocks; 288 GB of HBM make the slack affordable): R-MCL shrinks its matrices from one iteration to the next
      if (it != fb.end() && it->first <= 4 * r + (size_t(2) << 20)) {
        *p = it->second;
        live[*p] = Blk{it->first, dev};
        cached_bytes -= it->first;
        fb.erase(it);
        return hipSuccess;
      }
    }
    hipError_t e = hipMalloc(p, r);
    if (e != hipSuccess) {                       // give cached memory back and retry once
      trim(dev);
      e = hipMalloc(p, r);
    }
    if (e == hipSuccess) { std::lock_guard<std::mutex> lk(mu); live[*p] = Blk{r, dev}; }
    return e;
  }
  hipError_t release(void* p) {
    if (!p) return hipSuccess;
    if (check) (void)hipDeviceSynchronize();
    Blk blk{0, 0};
    {
      std::lock_guard<std::mutex> lk(mu);
      auto it = live.find(p);
      if (it == live.end()) return hipFree(p);   // not ours: plain hipFree
      blk = it->second;
      live.erase(it);
      if (cached_bytes + blk.size <= kMaxCached) {
        free_blocks[blk.dev].emplace(blk.size, p);
        cached_bytes += blk.size;
        return hipSuccess;
      }
    }
    return hipFree(p);
  }
  // give the cached (idle) blocks of one device back to the driver
  void trim(int dev) {
    std::lock_guard<std::mutex> lk(mu);
    auto& fb = free_blocks[dev];
    for (auto& kv : fb) { cached_bytes -= kv.first; (void)hipFree(kv.second); }
    fb.clear();
  }
  size_t cached_on(int dev) {
    std::lock_guard<std::mutex> lk(mu);
    size_t t = 0;
    for (auto& kv : free_blocks[dev]) t += kv.first;
    return t;
  }
};
DevPool& pool() { static DevPool* p = new DevPool(); return *p; }

// One pool block with one owner: released when the owner goes, or handed on with release().  Move-only: a block that
// went back twice would be hipFree'd under whoever holds it by then.
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.release()) {}
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.release(); } return *this; }
  ~DevBuf() { reset(); }
  hipError_t alloc(size_t n) { reset(); return pool().alloc((void**)&p, sizeof(T) * n); }   // on the current device
  void reset() { pool().release(p); p = nullptr; }
  T* release() { T* q = p; p = nullptr; return q; }             // the caller owns the block now
  operator T*() const { return p; }
};

// One block of the driver's with one owner and a capacity in elements: device memory (hipMalloc), or pinned host memory
// when Pinned.  The workspaces of a handle, a shard and the copy lanes are such blocks and NOT pool blocks: they live as
// long as their owner, and the pool's cached bytes stay what the calls leave there.  One operation: room for n elements,
// the contents discarded (n = 0: no block).  A failed reserve leaves no block and the error in the thread's slot.
template <class T, bool Pinned = false>
struct Block {
  T* p = nullptr;
  size_t cap = 0;
  Block() = default;
  Block(Block&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  Block& operator=(Block&& o) noexcept { if (this != &o) { reserve(0); std::swap(p, o.p); std::swap(cap, o.cap); } return *this; }
  ~Block() { reserve(0); }
  hipError_t reserve(size_t n) {
    if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr; cap = 0;
    if (n == 0) return hipSuccess;
    const hipError_t e = Pinned ? hipHostMalloc((void**)&p, sizeof(T) * n, hipHostMallocDefault) : hipMalloc((void**)&p, sizeof(T) * n);
    if (e == hipSuccess) cap = n; else p = nullptr;
    return e;
  }
  operator T*() const { return p; }
  T* operator->() const { return p; }
};
template <class T> using DevBlock = Block<T, false>;
template <class T> using PinBlock = Block<T, true>;

// A CSR matrix as a kernel reads it; nothing is owned.  len == nullptr: packed, row r is [I[r], I[r + 1]).  Otherwise row r
// is [I[r], I[r] + len[r]) of (J, V), se[r] is the same extent as one {start, end} pair (what the classification gathers)
// and nnz is the extent of the arrays.
struct CsrView {
  const int* I; const int* J; const float* V; int nnz;
  const int* len = nullptr; const int2* se = nullptr;
};

// A device matrix that owns its pool blocks, in one of the three forms R-MCL keeps:
//   packed   (no len)      I = row pointer, nnz entries in (J, V);
//   extents  (len and se)  the rows lie where the fused epilogues wrote them: I = scratch row starts, len = kept entries per
//                          row, se = {start, end} per row, nnz = extent of (J, V).  The next iteration reads it as it is;
//   block    (len, no se)  scratch rows too, but len = the SCANNED counts = the row pointer of the packed block (rows + 1
//                          entries, len[rows] = nnz = kept entries): the sharded loop packs the rows into its slice of Mt.
// Values of type T; the double loop packs after every step, so a DevCSRT<double> is always packed (len, se unused).
template <class T>
struct DevCSRT {
  DevBuf<int> I, J; DevBuf<T> V; DevBuf<int> len; DevBuf<int2> se;
  int rows = 0, cols = 0, nnz = 0;                  // rows, cols: set by upload_csr; a step knows them from its arguments
  bool packed() const { return !len; }
  CsrView view() const { return {I, J, V, nnz, len, se}; }   // (float only: instantiated where it is called)
  hipError_t alloc_entries(long long n) {           // (J, V) for n entries; never a zero-sized block
    const hipError_t e = J.alloc((size_t)std::max(n, 1ll));
    return e != hipSuccess ? e : V.alloc((size_t)std::max(n, 1ll));
  }
  void reset() { *this = DevCSRT(); }
  void give(int** oI, int** oJ, T** oV, int* onnz) {   // a packed matrix leaves the library (spgemm_hip_free takes it back)
    *oI = I.release(); *oJ = J.release(); *oV = V.release(); *onnz = nnz;
    reset();
  }
};
using DevCSR = DevCSRT<float>;

// The pool hands a released block to other handles and streams, so a block goes back only when no queued kernel can still
// touch it.  The owners above release when they leave scope; two rules make that late enough.
// Rule A: a failure may leave kernels queued that write the blocks of the failed step, so every error return of a function
// that has queued work is `return drained(stream, rc)`: the stream is idle before the locals are destroyed.  It holds for
// the whole library -- the product routes, the classification calls and the sharded jobs as much as R-MCL -- so a failed
// call costs one stream wait; a call that succeeds waits where it always did.
static int drained(hipStream_t s, int rc) {
  if (rc) (void)hipStreamSynchronize(s);
  return rc;
}
// Rule B: a step of the R-MCL loop that leaves its result as extents returns WITHOUT waiting for its numeric kernels, and
// they read the step's operand.  The operand is parked here and released one step later, when a call has waited for an
// event recorded behind those kernels (stream order alone does not protect a block once it is back in the pool).
struct Retired {
  DevCSR m;
  void park(DevCSR&& operand) { m = std::move(operand); }   // call only after a step that waited: releases the one parked before
};
}  // namespace

// ------------------------------------------------------------------------------------------------
// handle / workspace
// ------------------------------------------------------------------------------------------------
struct HostMirror {                 // one small device block + its pinned host twin, copied once per phase
  int binPtr[NBINS + 1];
  int err;
  int scratch2[4];                  // counts of the 513-2048 / 2049-4096 / 65-256 / 513-1024 rows when a classification is unpacked
  // work-queue heads of the block-per-row kernels (zeroed with the rest per call).  One 128-byte line EACH: the kernels
  // of a phase run side by side and every dequeue is an atomic on its word -- eight words in one line (next to binPtr /
  // slotBase, which every block reads when it starts) made all of them queue up behind one another in the L2.
  alignas(128) int qctr[10 * 32];
  alignas(128) int qpad_;
  int slotBase[NSLOTS + 1];         // first position of every layout slot in rowIds, [NSLOTS] = m (k_scatter_rows)
  int slotTot[NSLOTS];              // rows of every layout slot (k_bin_scan)
  unsigned long long totalP;
  unsigned long long nnzC64;
  unsigned long long kept64;        // entries that survive the fused R-MCL prune
  unsigned long long cutTotal;      // one-pass path (chain_device.hpp): total of the cut scan (unused), batches, ticket counter
  int nBatches;
  alignas(128) int chainTicket;
  alignas(128) int chainPad_;
  // big rows of a logging symbolic pass (k_sym_big<true>) that stay with k_num_bighash: {0, rows}, read by that kernel as
  // the "bin" of the fallback list (spgemm_handle::bigFallback)
  alignas(128) int fbBin[2];
  // the same for the rows of bins 6 and 7 that a logging k_sym_hash leaves to k_num_hash: {0, rows} of bin 6, {0, rows} of
  // bin 7 (lists: spgemm_handle::midFallback); then the log cursor (ints reserved, whether the log had them or not) and the
  // re-hits logged by the rows that stay direct
  alignas(128) int fbMid[4];
  alignas(128) unsigned long long mrCursor;
  unsigned long long mrLogged[2];   // (bin 6, bin 7)
  // rows of bin 6 the numeric launches took: k_num_midwave, k_num_middirect (test hook; written after the mirror is
  // taken, read from the device by spgemm_hip_debug_midrow_kernels)
  unsigned long long mdTook[2];
  // rows of bin 6 that k_sym_midpair processed: written by the symbolic pass, so the mirror has it
  unsigned long long spTook;
  // {0, rows}: the logged rows of bin 6 that k_num_midwave leaves to k_num_middirect, read by that kernel as the "bin" of
  // their list (the third part of spgemm_handle::midFallback)
  alignas(128) int mwRest[2];
  alignas(128) int fbPad_;
};

struct spgemm_handle {
  int device = 0;
  int numCU = 256;
  hipStream_t stream = nullptr;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // device workspace, sized for cap_m rows
  int cap_m = -1;
  DevBlock<int> rowFlops;
  DevBlock<unsigned char> binId;
  DevBlock<int> blockHist;
  DevBlock<int> blockOff;
  DevBlock<int> rowIds;
  DevBlock<unsigned long long> tileSum;
  DevBlock<unsigned long long> blockP;       // per-block sums of row flops (reduced by k_bin_scan)
  DevBlock<int2> sbl;                        // per A entry {B-row start, B-row length} (k_entry_lens); sized by nnz(A)
  DevBlock<int> batchStart;                  // one-pass path: first row of every batch (3*cap_m + 64 entries)
  DevBlock<unsigned long long> chainWords;   // ... and the batches' words of the chained prefix
  int pathMode = 0;                          // SPGEMM_PATH: 0 per-row kernels for every row (rounds 1-3); 1 rows up to smallMax
                                             // products through the wave-per-batch kernels, two passes; 2 the same in ONE pass
  int chainCfg = 0;                          // SPGEMM_CHAIN_CFG: kernel geometry (experiments)
  DevBlock<HostMirror> dsmall;
  PinBlock<HostMirror> hsmall;
  HostMirror mirror;                 // host copy taken at the end of the symbolic phase
  const int* cur_rowIds = nullptr;   // row list of the pending symbolic phase (workspace or caller's)
  int sym_m = -1;                    // rows of the pending symbolic phase, -1 = none
  hipEvent_t kev[2 * SPGEMM_NKERNELS] = {};
  bool kused[SPGEMM_NKERNELS] = {};
  unsigned ktiming = 0;              // bit i: launches of kernel i are bracketed by events (spgemm_hip_set_kernel_timing)
  hipEvent_t evMid = nullptr;        // "classification is on the host" marker of the one-shot path
  PinBlock<HostMirror> hmid;         // pinned copy taken right after the classify kernels
  // side streams: the per-bin kernels of one phase are independent; SPGEMM_CONCURRENT=1 runs them concurrently
  // (default off: the 155 KB-LDS big-row kernel owns the CUs it runs on, overlap measured slower than serial)
  static constexpr int NSIDE = 4;
  hipStream_t side[NSIDE] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t fork_ev = nullptr;
  hipEvent_t join_ev[NSIDE] = {nullptr, nullptr, nullptr, nullptr};
  bool serial = true;
  int U = 2;                         // rounds in flight per wave in the hash kernels (SPGEMM_U=2|4|8)
  // column bitmaps of the big rows, saved by the symbolic pass for the rank kernel (n <= BIG_WC).  Sized from
  // the previous calls (the number of big rows is only known on the host after the symbolic phase).
  DevBlock<unsigned> bigBitmaps;
  int bm_cap() const { return (int)(bigBitmaps.cap / BIG_WORDS); }          // big rows it has room for
  DevBlock<int2> spill;
  int spill_blocks() const { return (int)(spill.cap / BH_SPILL); }
  int bhCap = BH_CAP;
  int bhMargin = 125;                // parking region per hash class, % of products/npass (SPGEMM_BHMARGIN; tests force overflows)
  // direct big-row kernel (n > BIG_WC, float): the symbolic pass logs the re-hit columns of the big rows into rlLog (numCU
  // regions of rl_region ints) and {first entry, count} per row of the bin into rlMeta (rl_rows slots).  Sized from the
  // previous calls like the bitmaps above (grow_rehit_log): a call that finds no workspace, too few metadata slots or a
  // full region sends those rows down k_num_bighash.
  bool bigDirect = true;             // SPGEMM_BIGDIRECT=0: every big row takes k_num_bighash (A/B runs; keeps the fallback tested)
  int bdCfg = 1;                     // SPGEMM_BD_CFG: waves x table slots of k_num_bigdirect {0: 4x4096, 1: 8x4096, 2: 4x8192, 3: 8x8192,
                                     // 4: 16x4096}; 1 measured best (three blocks per CU; profiles/README.md)
  int bdMinRows = 0;                 // SPGEMM_BD_MINROWS: calls with fewer rows in the last bin keep k_num_bighash for all of them.  Default: the
                                     // CU count -- below it every row has a CU to itself in either kernel and the second launch costs more
                                     // than it saves (web surrogate: the bin 0.018 -> 0.023 ms); the tests set 1
  int rlRegionEnv = 0;               // SPGEMM_RLREGION: ints per block region instead of the computed size (tests fill a region)
  DevBlock<int2> rlMeta;             // (the two come and go together: grow_rehit_log)
  DevBlock<int> rlLog;
  int rl_rows() const { return (int)rlMeta.cap; }
  int rl_region() const { return (int)(rlLog.cap / (size_t)numCU); }
  DevBlock<int> bigFallback;         // rows of the fallback list (workspace block, one int per row of A)
  bool bdLogged = false;             // the pending / current product's symbolic pass logged (launch_symbolic)
  bool bdRan = false;                // the latest numeric launch used k_num_bigdirect
  // direct kernel of bins 6-7 (513-4096 products, float, any n): k_sym_hash<.., true> logs the rows' re-hit columns into mrLog
  // (mr_cap ints, handed out in chunks from HostMirror::mrCursor) and {first entry, count} into mrMeta[row id].  The log is
  // sized from the previous call's cursor (grow_midrow_log): a handle's first call with such rows finds none, counts what it
  // would have used and keeps today's kernels for all of them.
  bool midDirect = true;             // SPGEMM_MIDDIRECT=0: bins 6-7 keep k_sym_hash / k_num_hash as they were
  int mdCfg = -1;                    // SPGEMM_MD_CFG: waves x table slots of k_num_middirect {0: 4x1024, 1: 8x1024, 2: 4x2048, 3: 8x2048} for
                                     // both bins; default: 4x1024 for bin 6 and 8x1024 for bin 7, the waves of their hash kernels
                                     // (measured: profiles/README.md; four waves are too few for a row of 2049-4096 products when the
                                     // bin has only one or two rows per resident block)
  int mdCap = 0;                     // re-hits a row may log: bd_cap(slots), or less with SPGEMM_MD_CAP (tests)
  int mdMinRows = 0;                 // SPGEMM_MD_MINROWS: a bin with fewer rows keeps k_num_hash for all of them.  Default: 4 x the CU count --
                                     // below it every row of the bin is resident at once in either kernel, the launch lasts as long as
                                     // its slowest row, and a row with many re-hits is slower direct than hashed (web surrogate, 862
                                     // rows of 2049-4096 products with 30-50 % re-hits: 0.033 -> 0.066 ms); the tests set 1
  bool mdWave = true;                // SPGEMM_MD_WAVE=0: bin 6 keeps k_num_middirect for every direct row (A/B runs, tests)
  int mwMinRows = 0;                 // SPGEMM_MW_MINROWS: a bin 6 with fewer rows keeps k_num_middirect for all its direct rows.  Default:
                                     // 32 x the CU count -- one wave per row puts 16 rows on a CU (mwPerCU), and a bin of one or two rows
                                     // per wave lasts as long as its slowest row on ONE wave (profiles/README.md, "Mid rows: one wave per row")
  int mwPerCU = 16;                  // SPGEMM_MW_PERCU: blocks (= waves) of k_num_midwave per CU (measured 4 / 8 / 12 / 16 / 24: 0.301 /
                                     // 0.189 / 0.149 / 0.152 / 0.163 ms per launch on the headline matrix)
  bool mwRan = false;                // the latest numeric launch used k_num_midwave for bin 6
  // bin 6 of a logging symbolic pass by k_sym_midpair (one statically scheduled launch, two light rows at a time) instead of
  // k_sym_hash<4,4096,2,true>.  Measured equal at best on the headline matrix (profiles/README.md, "Mid rows, symbolic"): off
  bool symPair = false;              // SPGEMM_SYM_PAIR=1 turns it on
  int spWaves = 4;                   // SPGEMM_SP_WAVES=2|4: waves per block (per heavy row; half as many per light row)
  int spPerCU = 0;                   // SPGEMM_SP_PERCU: its blocks per CU; 0 = 6 -- a seventh block of four waves (158 KB of LDS in all) and an
                                     // eighth of two do not become resident, and under a static schedule the blocks that wait start their
                                     // whole share when the others end (measured: 5 / 6 / 7 blocks of four waves 0.280 / 0.271 / 0.322 ms)
  int spMinRows = 0;                 // SPGEMM_SP_MINROWS: the static schedule pays only with many rows per wave, and the bin's size is on the
                                     // device when the symbolic launches are queued.  The one-shot product takes the kernel when the handle's
                                     // previous product had the same m, n and nnz(A) and at least this many rows in bin 6 (default: 32 x the
                                     // CU count, mwMinRows' default; a wrong guess costs time only).  0: take it without asking (tests)
  int spPrevM = -1, spPrevN = -1;    // the previous one-shot product: shape, nnz(A), rows of bin 6
  long long spPrevNnzA = -1;
  int spPrevRows6 = 0;
  bool spRan = false;                // the latest symbolic launch used k_sym_midpair
  long long mrLogEnv = 0;            // SPGEMM_MRLOG: ints of the log instead of the computed size (tests run it out of space)
  DevBlock<int2> mrMeta;             // workspace block, one pair per row of A
  DevBlock<int> midFallback;         // workspace block, three ints per row of A: bin 6's list, then (at cap_m) bin 7's, then (at
                                     // 2 cap_m) the rows of bin 6 that k_num_midwave passes on to k_num_middirect
  DevBlock<int> mrLog;
  long long mr_cap() const { return (long long)mrLog.cap; }
  bool mdLogged = false;             // the pending / current product's symbolic pass logged bins 6-7
  bool mdRan[2] = {false, false};    // the latest numeric launch used k_num_middirect for bin 6 / bin 7
  int h1sym = 32;                    // blocks per CU of the wave-per-row symbolic kernel (SPGEMM_H1SYM, experiments)
  int h1num = 24;                    // ... of the wave-per-row numeric kernel on its 512-slot tables (SPGEMM_H1NUM)
  spgemm_stats stats;
  spgemm_host_api_stats host_api = {};   // phases of the latest hip_CSR_SpMM
  int failNext = 0;                  // test hook (spgemm_hip_debug_fail_next): the next symbolic phase / R-MCL step on this handle fails
  long long topkRows[4] = {0, 0, 0, 0};  // hip_csr_row_topk calls on this handle so far: rows copied / cut by the wave, block, stream path
  int prev_m = -1;                   // shape and sizes of the previous one-shot SpGEMM (allocation policy of the next one)
  unsigned long long prev_P = 0;
  long long prev_nnzC = -1;
  // The handle owns its streams, events and workspace blocks: the streams are waited for and destroyed with the events here
  // (whichever of them a failed spgemm_hip_create got as far as making), the block owners above free the rest.
  ~spgemm_handle() {
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    for (auto& st : side) if (st && st != stream) { hipStreamSynchronize(st); hipStreamDestroy(st); }
    if (evMid) hipEventDestroy(evMid);
    for (auto& e : ev) if (e) hipEventDestroy(e);
    for (auto& e : kev) if (e) hipEventDestroy(e);
    if (fork_ev) hipEventDestroy(fork_ev);
    for (auto& e : join_ev) if (e) hipEventDestroy(e);
    if (stream) hipStreamDestroy(stream);
  }
};

static std::mutex g_count_mu;
static std::map<int, int> g_handles_on;          // device -> live handles (the pool is trimmed when the last one goes)

// the workspace blocks sized by the row count: f(block, its elements for `cap` rows) for each of the twelve, until one fails
template <class F>
static int ws_blocks(spgemm_handle* h, size_t cap, F f) {
  const size_t nblk = (cap + K1_THREADS - 1) / K1_THREADS;
  const size_t ntile = (cap + 1 + SCAN_TILE - 1) / SCAN_TILE + 1;
  int rc;
  if ((rc = f(h->rowFlops, cap)) || (rc = f(h->binId, cap)) || (rc = f(h->blockHist, nblk * NSLOTS)) ||
      (rc = f(h->blockOff, nblk * NSLOTS)) || (rc = f(h->rowIds, cap)) || (rc = f(h->tileSum, ntile)) ||
      (rc = f(h->blockP, nblk)) || (rc = f(h->bigFallback, cap)) || (rc = f(h->mrMeta, cap)) ||
      (rc = f(h->midFallback, 3 * cap)) || (rc = f(h->batchStart, 3 * cap + 64)) || (rc = f(h->chainWords, 3 * cap + 64)))
    return rc;
  return SPGEMM_OK;
}

static int ws_ensure_entries(spgemm_handle* h, long long nnzA) {
  if (h->sbl && nnzA <= (long long)h->sbl.cap) return SPGEMM_OK;
  HIPCHK(h->sbl.reserve((size_t)(nnzA + nnzA / 8 + 1024)));
  return SPGEMM_OK;
}

static int ws_ensure(spgemm_handle* h, int m) {
  if (m <= h->cap_m) return SPGEMM_OK;
  const size_t cap = (size_t)m + (size_t)m / 8 + 1024;
  h->cap_m = -1;
  ws_blocks(h, cap, [](auto& b, size_t) { b.reserve(0); return SPGEMM_OK; });   // all of them go before the first comes back
  CHK(ws_blocks(h, cap, [](auto& b, size_t n) { HIPCHK(b.reserve(n)); return SPGEMM_OK; }));
  h->cap_m = (int)std::min<size_t>(cap, 0x7fffffff);
  return SPGEMM_OK;
}

// The direct kernels' geometries, waves x table slots, in the order of their knob's values
template <int NW, int S> struct Geo {};
template <class... G> struct GeoTable {};
typedef GeoTable<Geo<4, 4096>, Geo<8, 4096>, Geo<4, 8192>, Geo<8, 8192>, Geo<16, 4096>> BdGeos;   // SPGEMM_BD_CFG 0..4: k_num_bigdirect
typedef GeoTable<Geo<4, 1024>, Geo<8, 1024>, Geo<4, 2048>, Geo<8, 2048>> MdGeos;                  // SPGEMM_MD_CFG 0..3: k_num_middirect
// entry `cfg` of a table as compile-time constants: f(waves, table slots)
template <class F, int NW, int S, class... Gs>
static auto with_geometry(GeoTable<Geo<NW, S>, Gs...>, int cfg, F f) {
  if constexpr (sizeof...(Gs) > 0) if (cfg > 0) return with_geometry(GeoTable<Gs...>(), cfg - 1, f);
  return f(std::integral_constant<int, NW>(), std::integral_constant<int, S>());
}
template <class Table> static int slots_of(Table t, int cfg) { return with_geometry(t, cfg, [](auto, auto slots) { return (int)slots; }); }
// blocks per CU of a kernel with `lds` bytes per block and nw waves: what 160 KB of LDS and 32 waves hold
static int blocks_per_cu(int lds, int nw) { return std::max(1, std::min((160 * 1024) / lds, 32 / nw)); }

// an integer knob of the handle from the environment; a value outside [lo, hi] is ignored
static void env_int(const char* name, int lo, int hi, int* field) {
  if (const char* e = getenv(name)) { const int v = atoi(e); if (v >= lo && v <= hi) *field = v; }
}

extern "C" int spgemm_hip_device_count(int* count) {
  if (!count) return fail(SPGEMM_ERR_ARG, "count is null");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return fail(SPGEMM_ERR_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
  *count = n;
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_create(spgemm_handle** out, int device) {
  if (!out) return fail(SPGEMM_ERR_ARG, "handle out-pointer is null");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(SPGEMM_ERR_NODEVICE, "no HIP device visible: libspgemm_hip has no CPU fallback");
  if (device < 0 || device >= n) return fail(SPGEMM_ERR_ARG, "device %d out of range [0,%d)", device, n);
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<spgemm_handle> h(new spgemm_handle());   // a failed step below leaves nothing behind
  h->device = device;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  h->numCU = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  for (auto& e : h->ev) HIPCHK(hipEventCreate(&e));
  for (auto& e : h->kev) HIPCHK(hipEventCreate(&e));
  { const char* e = getenv("SPGEMM_CONCURRENT"); h->serial = !(e && e[0] == '1'); }
#ifdef SMF_ABLATE
  { int v = 0; env_int("SPGEMM_ABLATE", INT_MIN, INT_MAX, &v); HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(smf::g_ablate), &v, sizeof(int))); }
#endif
  env_int("SPGEMM_H1SYM", 1, 32, &h->h1sym);
  env_int("SPGEMM_H1NUM", 1, 32, &h->h1num);
  env_int("SPGEMM_BHMARGIN", 10, 400, &h->bhMargin);
  env_int("SPGEMM_BHCAP", 1024, BH_CAP_MAX, &h->bhCap);
  { int v = 1; env_int("SPGEMM_BIGDIRECT", 0, 1, &v); h->bigDirect = v != 0; }
  env_int("SPGEMM_BD_CFG", 0, 4, &h->bdCfg);
  h->bdMinRows = h->numCU;
  env_int("SPGEMM_BD_MINROWS", 1, 1 << 30, &h->bdMinRows);
  env_int("SPGEMM_RLREGION", 64, 1 << 24, &h->rlRegionEnv);
  { int v = 1; env_int("SPGEMM_MIDDIRECT", 0, 1, &v); h->midDirect = v != 0; }
  env_int("SPGEMM_MD_CFG", 0, 3, &h->mdCfg);
  h->mdCap = bd_cap(slots_of(MdGeos(), h->mdCfg));
  env_int("SPGEMM_MD_CAP", 0, h->mdCap, &h->mdCap);
  h->mdMinRows = 4 * h->numCU;
  env_int("SPGEMM_MD_MINROWS", 1, 1 << 30, &h->mdMinRows);
  { int v = 1; env_int("SPGEMM_MD_WAVE", 0, 1, &v); h->mdWave = v != 0; }
  h->mwMinRows = 32 * h->numCU;
  env_int("SPGEMM_MW_MINROWS", 1, 1 << 30, &h->mwMinRows);
  env_int("SPGEMM_MW_PERCU", 1, 32, &h->mwPerCU);
  { int v = 0; env_int("SPGEMM_SYM_PAIR", 0, 1, &v); h->symPair = v != 0; }
  { int v = h->spWaves; env_int("SPGEMM_SP_WAVES", 2, 4, &v); if (v == 2 || v == 4) h->spWaves = v; }
  env_int("SPGEMM_SP_PERCU", 1, 8, &h->spPerCU);
  h->spMinRows = 32 * h->numCU;
  env_int("SPGEMM_SP_MINROWS", 0, 1 << 30, &h->spMinRows);
  { int v = 0; env_int("SPGEMM_MRLOG", 1, 1 << 30, &v); h->mrLogEnv = v; }
  env_int("SPGEMM_PATH", 0, 2, &h->pathMode);
  env_int("SPGEMM_CHAIN_CFG", INT_MIN, INT_MAX, &h->chainCfg);   // unchecked: chain_cfg() maps anything else to 0
  { int u = h->U; env_int("SPGEMM_U", 2, 8, &u); if (u == 2 || u == 4 || u == 8) h->U = u; }
  for (auto& st : h->side) {
    if (h->serial) st = h->stream;
    else HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  }
  HIPCHK(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
  for (auto& e : h->join_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(h->dsmall.reserve(1));
  HIPCHK(h->hsmall.reserve(1));
  HIPCHK(h->hmid.reserve(1));
  HIPCHK(hipEventCreateWithFlags(&h->evMid, hipEventDisableTiming));
  { const char* e = getenv("SPGEMM_KTIMING"); if (e) h->ktiming = (unsigned)strtoul(e, nullptr, 0); }
  memset(&h->stats, 0, sizeof(h->stats));
  // the big-row kernels use more than the default 64 KB of dynamic LDS
  HIPCHK(hipFuncSetAttribute((const void*)k_sym_big<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(BigSymShared)));
  HIPCHK(hipFuncSetAttribute((const void*)k_sym_big<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(BigSymShared)));
  HIPCHK(with_geometry(BdGeos(), h->bdCfg, [&](auto nw, auto slots) {
    return hipFuncSetAttribute((const void*)k_num_bigdirect<nw, slots>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)sizeof(BigDirectShared<nw, slots>)); }));
  HIPCHK(hipFuncSetAttribute((const void*)k_num_big, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(BigNumShared)));
  HIPCHK(hipFuncSetAttribute((const void*)k_num_bighash, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(BigHashShared)));
  { std::lock_guard<std::mutex> lk(g_count_mu); ++g_handles_on[device]; }
  *out = h.release();
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_destroy(spgemm_handle* h) {
  if (!h) return SPGEMM_OK;
  const int device = h->device;
  delete h;
  bool last = false;
  { std::lock_guard<std::mutex> lk(g_count_mu); last = --g_handles_on[device] <= 0; }
  if (last) pool().trim(device);                 // cached blocks are idle by the pool's invariant
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_get_stats(const spgemm_handle* h, spgemm_stats* out) {
  if (!h || !out) return fail(SPGEMM_ERR_ARG, "null argument");
  *out = h->stats;
  return SPGEMM_OK;
}

extern "C" void* spgemm_hip_stream(spgemm_handle* h) { return h ? (void*)h->stream : nullptr; }

extern "C" int spgemm_hip_handle_device(const spgemm_handle* h) { return h ? h->device : -1; }

// test hook: the next `count` symbolic phases / fused R-MCL steps on this handle return SPGEMM_ERR_INTERNAL before they queue
// anything (how the tests make ONE rank of a multi-rank group fail: every rank must then leave the step with an error)
// test hook: how the latest product on this handle split its rows of more than 4096 products between k_num_bigdirect and
// k_num_bighash (n > BIG_WC only; the counts are those of the mirror the call read last), and the two sizes that decide it
extern "C" int spgemm_hip_debug_bigrow_paths(spgemm_handle* h, int* direct_rows, int* fallback_rows, int* rehit_cap, int* region_ints) {
  if (!h || !direct_rows || !fallback_rows || !rehit_cap || !region_ints) return fail(SPGEMM_ERR_ARG, "null argument");
  const int nbig = h->mirror.binPtr[NBINS] - h->mirror.binPtr[NBINS - 1];
  *fallback_rows = h->bdRan ? h->mirror.fbBin[1] : nbig;
  *direct_rows = nbig - *fallback_rows;
  *rehit_cap = bd_cap(slots_of(BdGeos(), h->bdCfg));
  *region_ints = h->rl_region();
  return SPGEMM_OK;
}

// ... and its rows of 513-4096 products (bins 6-7) between k_num_middirect (expanded rows included) and k_num_hash
extern "C" int spgemm_hip_debug_midrow_paths(spgemm_handle* h, int* rows, int* direct_rows, int* fallback_rows, int* rehit_cap) {
  if (!h || !rows || !direct_rows || !fallback_rows || !rehit_cap) return fail(SPGEMM_ERR_ARG, "null argument");
  *rows = h->mirror.binPtr[8] - h->mirror.binPtr[6];
  *fallback_rows = 0;
  for (int b = 0; b < 2; ++b) *fallback_rows += h->mdRan[b] ? h->mirror.fbMid[2 * b + 1] : h->mirror.binPtr[7 + b] - h->mirror.binPtr[6 + b];
  *direct_rows = *rows - *fallback_rows;
  *rehit_cap = h->mdCap;
  return SPGEMM_OK;
}
// ... with the log behind it: re-hits logged by the direct rows, ints the call reserved (or would have), ints the log had
extern "C" int spgemm_hip_debug_midrow_log(spgemm_handle* h, long long* logged, long long* reserved, long long* capacity) {
  if (!h || !logged || !reserved || !capacity) return fail(SPGEMM_ERR_ARG, "null argument");
  *logged = 0;
  for (int b = 0; b < 2; ++b) if (h->mdRan[b]) *logged += (long long)h->mirror.mrLogged[b];
  *reserved = h->mdLogged ? (long long)h->mirror.mrCursor : 0;
  *capacity = h->mr_cap();
  return SPGEMM_OK;
}

// ... and which of the two direct kernels took the direct rows of 513-2048 products: counted on the device by the kernels
// themselves, behind the host mirror, so this hook waits for the handle's stream and reads the two counters
extern "C" int spgemm_hip_debug_midrow_kernels(spgemm_handle* h, long long* wave_rows, long long* multiwave_rows) {
  if (!h || !wave_rows || !multiwave_rows) return fail(SPGEMM_ERR_ARG, "null argument");
  *wave_rows = 0; *multiwave_rows = 0;
  if (!h->mdRan[0]) return SPGEMM_OK;                  // (bin 6 ran k_num_hash alone: the counters are not this product's)
  unsigned long long v[2] = {0ull, 0ull};
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(v, h->dsmall->mdTook, sizeof(v), hipMemcpyDeviceToHost));
  *wave_rows = h->mwRan ? (long long)v[0] : 0;
  *multiwave_rows = (long long)v[1];
  return SPGEMM_OK;
}

// ... and which symbolic kernel counted (and logged) the rows of 513-2048 products of a logging pass: k_sym_midpair
// counts its rows on the device, in the block the host mirrors at the end of the product
extern "C" int spgemm_hip_debug_midrow_sym_paths(spgemm_handle* h, long long* pair_rows, long long* multiwave_rows) {
  if (!h || !pair_rows || !multiwave_rows) return fail(SPGEMM_ERR_ARG, "null argument");
  const long long rows6 = h->mirror.binPtr[7] - h->mirror.binPtr[6];
  *pair_rows = h->spRan ? (long long)h->mirror.spTook : 0;
  *multiwave_rows = h->mdLogged && !h->spRan ? rows6 : 0;
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_debug_fail_next(spgemm_handle* h, int count) {
  if (!h) return fail(SPGEMM_ERR_ARG, "null handle");
  h->failNext = count;
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_set_kernel_timing(spgemm_handle* h, unsigned mask) {
  if (!h) return fail(SPGEMM_ERR_ARG, "null handle");
  h->ktiming = mask;
  return SPGEMM_OK;
}

static std::mutex g_default_mu;
static spgemm_handle* g_default = nullptr;
static int default_handle(spgemm_handle** out) {
  std::lock_guard<std::mutex> lk(g_default_mu);
  if (!g_default) CHK(spgemm_hip_create(&g_default, 0));
  *out = g_default;
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_malloc(void** dptr, size_t bytes) {
  if (!dptr) return fail(SPGEMM_ERR_ARG, "dptr is null");
  *dptr = nullptr;
  HIPCHK(pool().alloc(dptr, bytes ? bytes : 1));
  return SPGEMM_OK;
}
extern "C" int spgemm_hip_pool_cached_bytes(int device, size_t* bytes) {
  if (!bytes) return fail(SPGEMM_ERR_ARG, "bytes is null");
  *bytes = pool().cached_on(device);
  return SPGEMM_OK;
}
// give the idle cached blocks of `device` back to the driver (blocks in use are not touched)
extern "C" int spgemm_hip_pool_trim(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return fail(SPGEMM_ERR_ARG, "device %d out of range", device);
  int cur = 0;
  const bool had = hipGetDevice(&cur) == hipSuccess;
  HIPCHK(hipSetDevice(device));
  pool().trim(device);
  if (had) (void)hipSetDevice(cur);
  return SPGEMM_OK;
}
extern "C" int spgemm_hip_free(void* dptr) {
  HIPCHK(pool().release(dptr));
  return SPGEMM_OK;
}
// (copies of 8 MB and more between pageable host memory and the device go through the parallel pinned lanes further down:
//  CSR::toGpuCSR / toCpuCSR of a large matrix then run at the link rate instead of the runtime's single staging thread)
struct CopyJob { void* host; void* dev; size_t bytes; };
static int copy_pageable(int dev, const CopyJob* jobs, int njobs, bool toDevice);
static constexpr size_t kLaneCopyMin = size_t(8) << 20;
static int device_of(const void* dptr) {           // the device a pointer lives on (the current one if the runtime cannot say)
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, dptr) == hipSuccess) return a.device;
  (void)hipGetLastError();
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev;
}

extern "C" int spgemm_hip_memcpy_h2d(void* dst, const void* src, size_t bytes) {
  if (bytes && (!dst || !src)) return fail(SPGEMM_ERR_ARG, "null pointer in h2d copy");
  if (bytes >= kLaneCopyMin) {
    const CopyJob j{const_cast<void*>(src), dst, bytes};
    return copy_pageable(device_of(dst), &j, 1, true);
  }
  if (bytes) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return SPGEMM_OK;
}
extern "C" int spgemm_hip_memcpy_d2h(void* dst, const void* src, size_t bytes) {
  if (bytes && (!dst || !src)) return fail(SPGEMM_ERR_ARG, "null pointer in d2h copy");
  if (bytes >= kLaneCopyMin) {
    const CopyJob j{dst, const_cast<void*>(src), bytes};
    return copy_pageable(device_of(src), &j, 1, false);
  }
  if (bytes) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_memcpy_d2d(void* dst, const void* src, size_t bytes) {
  if (bytes && (!dst || !src)) return fail(SPGEMM_ERR_ARG, "null pointer in d2d copy");
  if (bytes) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
  return SPGEMM_OK;
}

// hipMemcpy device-to-device may return before the copy has run; this waits for everything queued on the current device
extern "C" int spgemm_hip_device_synchronize(void) {
  HIPCHK(hipDeviceSynchronize());
  return SPGEMM_OK;
}

// ------------------------------------------------------------------------------------------------
// launch sequence
// ------------------------------------------------------------------------------------------------
// hipGetLastError() after a batch of launches is how launch failures are noticed; the slot it reads is per thread and keeps
// the last error of ANY earlier HIP call, ours or another library's in this process (RCCL probing devices leaves
// "invalid device ordinal" behind: seen as a spurious failure of the next SpGEMM).  Every launch sequence therefore
// starts by emptying the slot.
// What this can hide: a NON-sticky error left by this library's own previous launch on the thread (a bad launch
// configuration) if that launch site did not look at it.  Every launch sequence here ends with HIPCHK(hipGetLastError())
// before its function returns, so there is no such site -- keep it that way: the post-launch check is mandatory wherever
// this call opens a sequence.  Sticky errors (a fault) are not cleared by reading them and still fail the next call.
static inline void clear_stale_hip_error() { (void)hipGetLastError(); }
static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline int clampi(long long v, int lo, int hi) { return (int)std::max<long long>(lo, std::min<long long>(v, hi)); }
// grid of a statically scheduled kernel: a multiple of 8 (one contiguous eighth of the work per XCD: xcd_range)
static inline int grid8(long long want, int hi) { return (clampi(want, 8, hi) + 7) & ~7; }

// Tiles up to which every block of k_scan_apply adds up the sums of the tiles before its own (two launches); above, a
// one-block launch scans the sums in between.  A block reads its share of the sums in one round of loads up to 1024 tiles
// and in four at the limit; the work of all blocks together grows with the square of the tiles, so it has a limit.
// -DSMF_SCAN_FOLD_MAX=0: always three launches.
#ifndef SMF_SCAN_FOLD_MAX
#define SMF_SCAN_FOLD_MAX 4096
#endif
// the launches of an in-place exclusive scan of cnt[0..m), cnt[m] = total (clamped to INT_MAX or wrapping: k_scan_apply);
// tileSum: one word per tile of SCAN_TILE ints, *dTotal: the exact total
static inline void scan_launches(hipStream_t s, int* cnt, int m, unsigned long long* tileSum, unsigned long long* dTotal,
                                 bool clampTotal) {
  const int ntiles = std::max(1, cdiv(m, SCAN_TILE));
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(ntiles), dim3(SCAN_THREADS), 0, s, m, cnt, tileSum);
  if (ntiles <= SMF_SCAN_FOLD_MAX) {
    hipLaunchKernelGGL(k_scan_apply<true>, dim3(ntiles), dim3(SCAN_THREADS), 0, s, m, cnt, tileSum, dTotal, clampTotal ? 1 : 0);
  } else {
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, ntiles, tileSum, dTotal);
    hipLaunchKernelGGL(k_scan_apply<false>, dim3(ntiles), dim3(SCAN_THREADS), 0, s, m, cnt, tileSum, dTotal, clampTotal ? 1 : 0);
  }
}

static const char* kKernelNames[SPGEMM_NKERNELS] = {
    "k_row_flops", "k_bin_scan", "k_scatter_rows", "k_sym_g16<32,1>", "k_sym_g16", "k_sym_hash<1,1024>",
    "k_sym_hash<4,4096>", "k_sym_hash<8,8192>", "k_sym_big", "k_scan(3 launches)", "k_num_g16<32,1>", "k_num_g16",
    "k_num_hash<1,1024>", "k_num_hash<4,4096>", "k_num_hash<8,8192>", "k_num_big", "k_num_bighash", "k_cut(3 launches)",
    "k_chain", "k_wbatch<sym>", "k_wbatch<num>"};
extern "C" const char* spgemm_hip_kernel_name(int id) { return (id >= 0 && id < SPGEMM_NKERNELS) ? kKernelNames[id] : ""; }

// every launch is bracketed by two events on its stream (per-kernel durations for bench.py's roofline)
// (only for the kernels selected with spgemm_hip_set_kernel_timing: an event record costs a few microseconds of
// stream time, 40 of them per SpGEMM were 3 % of a step)
struct KTimer {
  spgemm_handle* h; int id; hipStream_t s; bool on;
  KTimer(spgemm_handle* h_, int id_, hipStream_t s_ = nullptr)
      : h(h_), id(id_), s(s_ ? s_ : h_->stream), on((h_->ktiming >> id_) & 1u) {
    if (on) { hipEventRecord(h->kev[2 * id], s); h->kused[id] = true; }
  }
  ~KTimer() { if (on) hipEventRecord(h->kev[2 * id + 1], s); }
};

static void collect_kernel_times(spgemm_handle* h, bool reset) {
  for (int i = 0; i < SPGEMM_NKERNELS; ++i) {
    if (reset) h->stats.ms_kernel[i] = 0.f;
    if (h->kused[i]) { float ms = 0.f; if (hipEventElapsedTime(&ms, h->kev[2 * i], h->kev[2 * i + 1]) == hipSuccess) h->stats.ms_kernel[i] = ms; }
    h->kused[i] = false;
  }
}

// fork: the side streams wait for everything queued on the main stream so far
static void fork_streams(spgemm_handle* h) {
  if (h->serial) return;
  hipEventRecord(h->fork_ev, h->stream);
  for (auto& st : h->side) hipStreamWaitEvent(st, h->fork_ev, 0);
}
// join: the main stream waits for the side streams
static void join_streams(spgemm_handle* h) {
  if (h->serial) return;
  for (int i = 0; i < spgemm_handle::NSIDE; ++i) {
    hipEventRecord(h->join_ev[i], h->side[i]);
    hipStreamWaitEvent(h->stream, h->join_ev[i], 0);
  }
}

#define LAUNCH_U(KERN, NW, TBL, grid, block, st, ...)                                              \
  do {                                                                                             \
    if (h->U == 8) hipLaunchKernelGGL((KERN<NW, TBL, 8>), grid, block, 0, st, __VA_ARGS__);        \
    else if (h->U == 4) hipLaunchKernelGGL((KERN<NW, TBL, 4>), grid, block, 0, st, __VA_ARGS__);   \
    else hipLaunchKernelGGL((KERN<NW, TBL, 2>), grid, block, 0, st, __VA_ARGS__);                  \
  } while (0)

// The numeric kernels take the fused R-MCL prune as a template argument: 0 plain SpGEMM, 1 prune, 2 prune with no symbolic
// pass below bin 8.  This is the one place it is derived from pcnt/pmode: f is called with it as a compile-time constant.
template <class F>
static void with_prune_arg(const int* pcnt, int pmode, F f) {
  if (pcnt && pmode == 2) f(std::integral_constant<int, 2>());
  else if (pcnt) f(std::integral_constant<int, 1>());
  else f(std::integral_constant<int, 0>());
}

// k_num_hash: the rounds-in-flight variants (SPGEMM_U) exist for the plain kernel only
#define LAUNCH_NUM(NW, TBL, grid, block, st, ...)                                                                  \
  with_prune_arg(pcnt, pmode, [&](auto prune) {                                                                    \
    if constexpr (prune != 0) hipLaunchKernelGGL((k_num_hash<NW, TBL, 2, prune>), grid, block, 0, st, __VA_ARGS__, pcnt); \
    else LAUNCH_U(k_num_hash, NW, TBL, grid, block, st, __VA_ARGS__, (int*)nullptr);                               \
  })

// flops + bins: K1, K2, K3.  Also presets IC[row] for rows with 0 / 1 products.
// nnzA >= 0: the per-entry records h->sbl are (re)built first and the row sums read them; nnzA < 0 (entry points of
// the C ABI that are not told nnz(A)): the sums gather through JA -> IB directly.
static int launch_classify(spgemm_handle* h, const int* dIA, const int* dJA, const int* dIB, int m, long long nnzA, int* dIC,
                           const int2* dIBse = nullptr) {
  const int nblk = cdiv(m, K1_THREADS);
  clear_stale_hip_error();
  HIPCHK(hipMemsetAsync(h->dsmall, 0, sizeof(HostMirror), h->stream));
  if (nnzA >= 0) CHK(ws_ensure_entries(h, nnzA));
  if (m > 0) {
    { KTimer t(h, SPGEMM_K_ROW_FLOPS);           // also writes the per-entry records h->sbl when nnz(A) is known
      int2* const sbl = nnzA >= 0 ? h->sbl : (int2*)nullptr;
      const int cap = (int)std::max(nnzA, 0ll);
      if (dIBse) hipLaunchKernelGGL(k_row_flops<true>, dim3(nblk), dim3(K1_THREADS), 0, h->stream, m, dIA, dJA, dIB, dIBse,
                                    sbl, cap, h->rowFlops, h->binId, h->blockHist, h->blockP, dIC);
      else hipLaunchKernelGGL(k_row_flops<false>, dim3(nblk), dim3(K1_THREADS), 0, h->stream, m, dIA, dJA, dIB, dIBse,
                              sbl, cap, h->rowFlops, h->binId, h->blockHist, h->blockP, dIC); }
    { KTimer t(h, SPGEMM_K_BIN_SCAN);
      hipLaunchKernelGGL(k_bin_scan, dim3(NSLOTS), dim3(K2_THREADS), 0, h->stream, nblk, h->blockHist, h->blockOff,
                         h->dsmall->slotTot, h->blockP, &h->dsmall->totalP); }
    { KTimer t(h, SPGEMM_K_SCATTER);             // also turns the slot totals into slotBase / binPtr
      hipLaunchKernelGGL(k_scatter_rows, dim3(nblk), dim3(K1_THREADS), 0, h->stream, m, h->binId, h->blockOff,
                         h->dsmall->slotTot, h->dsmall->slotBase, h->dsmall->binPtr, h->rowIds); }
  }
  HIPCHK(hipGetLastError());
  return SPGEMM_OK;
}

// symbolic pass over bins 2..8 (bins 0/1 were preset by K1).  Bin sizes are not known on the host
// here (no sync): grids are capped by the CU count and every block strides / dequeues over its bin.
static int launch_symbolic(spgemm_handle* h, const int* dIA, const int* dJB,
                           int m, int n, const int* rowIds, int* dIC, int minBin = 0, bool skipH1A = false, bool logBig = false,
                           bool pairOk = false) {
  const int2* sbl = h->sbl;
  // logBig: a float product's big rows may take k_num_bigdirect -- the symbolic kernel logs their re-hit columns
  h->bdLogged = logBig && h->bigDirect && n > BIG_WC && m > 0;
  // ... and its rows of bins 6-7 k_num_middirect, for any n (the plain pipeline with its default rounds in flight only)
  h->mdLogged = logBig && h->midDirect && m > 0 && minBin == 0 && h->pathMode == 0 && h->U == 2;
  // ... bin 6 by k_sym_midpair (pairOk: the caller's guess that the bin is large enough, see spMinRows)
  h->spRan = h->mdLogged && h->symPair && pairOk;
  if (m <= 0) return SPGEMM_OK;
  clear_stale_hip_error();
  const int* bp = h->dsmall->binPtr;
  int* err = &h->dsmall->err;
  int* qc = h->dsmall->qctr;
  const int cu = h->numCU;
  fork_streams(h);
  { hipStream_t st = h->side[3]; KTimer t(h, SPGEMM_K_SYM_BIG, st);
    // (the grid never exceeds the CU count: rlLog has one region per CU)
    if (h->bdLogged)
      hipLaunchKernelGGL(k_sym_big<true>, dim3(clampi(m, 1, cu)), dim3(BIG_THREADS), sizeof(BigSymShared), st, bp, 8,
                         rowIds, dIA, sbl, dJB, n, dIC, h->bigBitmaps, h->bm_cap(), qc + 0 * 32,
                         h->rlMeta, h->rlLog ? h->rl_rows() : 0, h->rlLog, h->rl_region(), bd_cap(slots_of(BdGeos(), h->bdCfg)), h->bigFallback,
                         &h->dsmall->fbBin[1]);
    else
      hipLaunchKernelGGL(k_sym_big<false>, dim3(clampi(m, 1, cu)), dim3(BIG_THREADS), sizeof(BigSymShared), st, bp, 8,
                         rowIds, dIA, sbl, dJB, n, dIC, h->bigBitmaps, h->bm_cap(), qc + 0 * 32,
                         (int2*)nullptr, 0, (int*)nullptr, 0, 0, (int*)nullptr, (int*)nullptr); }
  // the logging variants of the two launches below: one log and one cursor for both, a fallback list each
  auto mid_log = [&](int which) {
    return MidLogArgs{h->mrMeta, h->mrLog, h->mrLog ? h->mr_cap() : 0ll, h->mdCap, &h->dsmall->mrCursor,
                      h->midFallback + (which ? h->cap_m : 0), &h->dsmall->fbMid[2 * which + 1], &h->dsmall->mrLogged[which]};
  };
  if (minBin <= 7) { hipStream_t st = h->side[2]; KTimer t(h, SPGEMM_K_SYM_HASH8, st);
    if (h->mdLogged)
      hipLaunchKernelGGL((k_sym_hash<8, 8192, 2, true>), dim3(clampi(m, 1, cu * 3)), dim3(512), 0, st, bp, 7, rowIds, dIA,
                         sbl, dJB, h->rowFlops, dIC, err, qc + 1 * 32, mid_log(1));
    else
    LAUNCH_U(k_sym_hash, 8, 8192, dim3(clampi(m, 1, cu * 3)), dim3(512), st, bp, 7, rowIds, dIA,
             sbl, dJB, h->rowFlops, dIC, err, qc + 1 * 32, MidLogArgs{}); }
  if (minBin <= 6) { hipStream_t st = h->side[2]; KTimer t(h, SPGEMM_K_SYM_HASH4, st);
    // (one launch for both layout slots of bin 6: split like the numeric side it measured 15 % slower)
    // k_sym_midpair: both slots in one launch too, statically scheduled (the bin's size is not known here: the grid is
    // what the CUs hold, a block without rows leaves at once)
    if (h->spRan) {
      const int perCU = h->spPerCU > 0 ? h->spPerCU : 6;
      if (h->spWaves == 4)
        hipLaunchKernelGGL(k_sym_midpair<4>, dim3(grid8(m, cu * perCU)), dim3(4 * WAVE), 0, st, h->dsmall->slotBase, SLOT_H4A,
                           SLOT_H4B, rowIds, dIA, sbl, dJB, (const int*)h->rowFlops, dIC, err, mid_log(0), &h->dsmall->spTook);
      else
        hipLaunchKernelGGL(k_sym_midpair<2>, dim3(grid8(m, cu * perCU)), dim3(2 * WAVE), 0, st, h->dsmall->slotBase, SLOT_H4A,
                           SLOT_H4B, rowIds, dIA, sbl, dJB, (const int*)h->rowFlops, dIC, err, mid_log(0), &h->dsmall->spTook);
    }
    else if (h->mdLogged)
      hipLaunchKernelGGL((k_sym_hash<4, 4096, 2, true>), dim3(clampi(m, 1, cu * 8)), dim3(256), 0, st, bp, 6, rowIds, dIA,
                         sbl, dJB, h->rowFlops, dIC, err, qc + 2 * 32, mid_log(0));
    else
    LAUNCH_U(k_sym_hash, 4, 4096, dim3(clampi(m, 1, cu * 8)), dim3(256), st, bp, 6, rowIds, dIA,
             sbl, dJB, h->rowFlops, dIC, err, qc + 2 * 32, MidLogArgs{}); }
  if (minBin <= 5) { hipStream_t st = h->side[1]; KTimer t(h, SPGEMM_K_SYM_HASH1, st);
    const int* sb = h->dsmall->slotBase;         // bin 5 = two layout slots: table 512 up to 256 products, 1024 above
    if (!skipH1A)
    LAUNCH_U(k_sym_hash, 1, 512, dim3(grid8(m, cu * h->h1sym)), dim3(64), st, sb, SLOT_H1A, rowIds, dIA,
             sbl, dJB, h->rowFlops, dIC, err, qc + 3 * 32, MidLogArgs{});
    LAUNCH_U(k_sym_hash, 1, 1024, dim3(grid8(m, cu * h->h1sym)), dim3(64), st, sb, SLOT_H1B, rowIds, dIA,
             sbl, dJB, h->rowFlops, dIC, err, qc + 3 * 32, MidLogArgs{}); }
  if (minBin <= 4) { hipStream_t st = h->side[0]; KTimer t(h, SPGEMM_K_SYM_G16, st);
    hipLaunchKernelGGL((k_sym_g16<128, 4>), dim3(grid8(cdiv(m, 16), cu * 16)), dim3(256), 0, st, bp, 4, 5,
                       rowIds, dIA, sbl, dJB, h->rowFlops, dIC, err); }
  if (minBin <= 3) { KTimer t(h, SPGEMM_K_SYM_SMALL4);           // 2..16 products: the same 16-lane flattened kernel, one round per row
    hipLaunchKernelGGL((k_sym_g16<32, 1>), dim3(grid8(cdiv(m, 16), cu * 16)), dim3(256), 0, h->stream, bp, 2, 4,
                       rowIds, dIA, sbl, dJB, h->rowFlops, dIC, err); }
  join_streams(h);
  HIPCHK(hipGetLastError());
  return SPGEMM_OK;
}

// exclusive scan of cnt[0..m) in place, cnt[m] = total; 64-bit total lands in *dTotal
static int launch_scan(spgemm_handle* h, int* cnt, int m, unsigned long long* dTotal, bool clampTotal = true) {
  clear_stale_hip_error();
  KTimer t(h, SPGEMM_K_SCAN);
  scan_launches(h->stream, cnt, m, h->tileSum, dTotal, clampTotal);
  HIPCHK(hipGetLastError());
  return SPGEMM_OK;
}

static int launch_numeric(spgemm_handle* h, const int* dIA, const float* dA,
                          const int* dJB, const float* dB, int n, const int* rowIds, const int* hostBinPtr,
                          const int* dIC, int* dJC, float* dC, int* pcnt = nullptr, int pmode = 1, int minBin = 0,
                          bool skipH1A = false) {
  // pcnt != nullptr: fused R-MCL prune -- every row leaves only its kept, normalised entries at the front of its range
  // of dJC/dC and their count in pcnt[row] (rows of bin 8 are written in full and fixed up in place right behind).
  // pmode 2: no symbolic pass ran below bin 8: dIC holds the prefix sums of the rows' product counts there, exact counts
  // for the rows of bin 8
  const int2* sbl = h->sbl;
  clear_stale_hip_error();
  const int* bp = h->dsmall->binPtr;
  int* err = &h->dsmall->err;
  int* qc = h->dsmall->qctr;
  const int cu = h->numCU;
  auto rows = [&](int lo, int hi) { return lo < minBin ? 0 : hostBinPtr[hi] - hostBinPtr[lo]; };   // (lo = the lowest bin of the launch)
  fork_streams(h);
  if (rows(8, 9) > 0) {
    hipStream_t st = h->side[3];
    if (n <= BIG_WC) { KTimer t(h, SPGEMM_K_NUM_BIG, st);
      hipLaunchKernelGGL(k_num_big, dim3(clampi(rows(8, 9), 1, cu)), dim3(BIG_THREADS), sizeof(BigNumShared), st,
                         bp, 8, rowIds, dIA, sbl, dA, dJB, dB, n, dIC, dJC, dC, err, h->bigBitmaps, h->bm_cap(),
                         qc + 4 * 32);
    } else { KTimer t(h, SPGEMM_K_NUM_BIGHASH, st);   // both launches of the direct path are timed under this id
      const int blocks = clampi(rows(8, 9), 1, cu);
      // rows whose re-hits the symbolic pass logged take k_num_bigdirect, the others are in the fallback list (its length is
      // on the device only: the launch is sized by the bin); the fused R-MCL step keeps k_num_bighash for all of them
      // (and so does a call with only a few such rows: bdMinRows)
      const bool direct = h->bdLogged && !pcnt && rows(8, 9) >= h->bdMinRows;
      h->bdRan = direct;
      // parking space of multi-pass rows: 1 MB per block, kept; without it those rows walk once per pass
      if (blocks > h->spill_blocks() && h->spill.reserve((size_t)blocks * BH_SPILL) != hipSuccess) (void)hipGetLastError();
      hipLaunchKernelGGL(k_num_bighash, dim3(blocks), dim3(BIG_THREADS), sizeof(BigHashShared), st,
                         direct ? h->dsmall->fbBin : bp, direct ? 0 : 8, direct ? h->bigFallback : rowIds, dIA, sbl, dA, dJB,
                         dB, dIC, dJC, dC, err, qc + 4 * 32, h->rowFlops,
                         h->spill_blocks() >= blocks ? h->spill.p : (int2*)nullptr, BH_SPILL, h->bhCap, h->bhMargin);
      if (direct && h->rlLog)                          // (no workspace yet: every row is in the fallback list)
        with_geometry(BdGeos(), h->bdCfg, [&](auto nw, auto slots) {
          const int lds = (int)sizeof(BigDirectShared<nw, slots>);
          const int perCU = blocks_per_cu(lds, nw);
          hipLaunchKernelGGL((k_num_bigdirect<nw, slots>), dim3(clampi(rows(8, 9), 1, cu * perCU)), dim3(WAVE * nw), lds, st,
                             bp, 8, rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, qc + 8 * 32,
                             (const int2*)h->rlMeta, h->rl_rows(), (const int*)h->rlLog);
          return 0; }); }
    if (pcnt) hipLaunchKernelGGL(k_rmcl_fix_rows<float>, dim3(clampi(rows(8, 9), 1, cu * 8)), dim3(256), 0, st,
                                 bp, 8, 9, rowIds, dIC, dJC, dC, pcnt, -1);   // lmin = -1: every row of the bin
  }
  // bins 6-7 of a product whose symbolic pass logged into a log that exists: k_num_middirect over the bin for the rows with
  // a log, k_num_hash (the larger table of the bin) over the bin's fallback list for the others -- its length is on the
  // device only, the launch is sized by the bin and a few blocks.  Both launches are timed under the bin's id.  (No log
  // yet, or a bin of fewer than mdMinRows rows: today's launches run over the bin itself.)
  const bool mid = h->mdLogged && h->mrLog && !pcnt && minBin <= 6;
  const bool mid6 = mid && rows(6, 7) >= h->mdMinRows, mid7 = mid && rows(7, 8) >= h->mdMinRows;
  h->mdRan[0] = mid6; h->mdRan[1] = mid7;
  // bin 6, rows up to waveCap re-hits: one wave per row (k_num_midwave), both layout slots in one launch, the heavy slot
  // first.  It puts the logged rows it leaves (midwave_takes is the one rule, read by both kernels) on a list, and
  // k_num_middirect runs over that list instead of the bin: skipping 56 000 rows of the headline matrix one dequeue of four at
  // a time cost it 0.185 ms (profiles/README.md, "Mid rows: one wave per row")
  const int waveCap = mid6 && h->mdWave && rows(6, 7) >= h->mwMinRows ? std::min(h->mdCap, bd_cap(MW_SLOTS)) : -1;
  h->mwRan = waveCap >= 0;
  auto launch_mid = [&](int bin, int nrows, int* qd, hipStream_t st, int wcap, unsigned long long* took,
                        const int* lbp, int lbin, const int* lrows) {       // (the rows: bin `lbin` of lbp over lrows)
    with_geometry(MdGeos(), h->mdCfg >= 0 ? h->mdCfg : bin == 7 ? 1 : 0, [&](auto nw, auto slots) {
      const int perCU = blocks_per_cu((int)sizeof(MidDirectShared<nw, slots>), nw);
      hipLaunchKernelGGL((k_num_middirect<nw, slots>), dim3(clampi(nrows, 1, cu * perCU)), dim3(WAVE * nw), 0, st,
                         lbp, lbin, lrows, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, qd, (const int*)h->rowFlops,
                         (const int2*)h->mrMeta, (const int*)h->mrLog, h->mr_cap(), h->mdCap, wcap, took);
      return 0; });
  };
  if (mid7) { hipStream_t st = h->side[2]; KTimer t(h, SPGEMM_K_NUM_HASH8, st);
    launch_mid(7, rows(7, 8), qc + 9 * 32, st, -1, (unsigned long long*)nullptr, bp, 7, rowIds);
    LAUNCH_U(k_num_hash, 8, 8192, dim3(clampi(rows(7, 8), 1, cu * 2)), dim3(512), st, h->dsmall->fbMid + 2, 0,
             (const int*)(h->midFallback + h->cap_m), dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, qc + 5 * 32, h->rowFlops, (int*)nullptr); }
  if (mid6) { hipStream_t st = h->side[2]; KTimer t(h, SPGEMM_K_NUM_HASH4, st);
    if (waveCap >= 0) {
      hipLaunchKernelGGL(k_num_midwave, dim3(grid8(rows(6, 7), cu * h->mwPerCU)), dim3(WAVE), 0, st, h->dsmall->slotBase,
                         SLOT_H4A, SLOT_H4B, rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, (const int*)h->rowFlops,
                         (const int2*)h->mrMeta, (const int*)h->mrLog, h->mr_cap(), waveCap, &h->dsmall->mdTook[0],
                         h->midFallback + 2 * (size_t)h->cap_m, &h->dsmall->mwRest[1]);
      launch_mid(6, rows(6, 7), qc + 6 * 32, st, waveCap, &h->dsmall->mdTook[1], h->dsmall->mwRest, 0,
                 (const int*)(h->midFallback + 2 * (size_t)h->cap_m));
    } else
    launch_mid(6, rows(6, 7), qc + 6 * 32, st, waveCap, &h->dsmall->mdTook[1], bp, 6, rowIds);
    LAUNCH_U(k_num_hash, 4, 4096, dim3(clampi(rows(6, 7), 1, cu * 4)), dim3(256), st, h->dsmall->fbMid, 0,
             (const int*)h->midFallback, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, qc + 7 * 32, h->rowFlops, (int*)nullptr); }
  if (!mid7 && rows(7, 8) > 0) { hipStream_t st = h->side[2]; KTimer t(h, SPGEMM_K_NUM_HASH8, st);
    LAUNCH_NUM(8, 8192, dim3(clampi(rows(7, 8), 1, cu * 2)), dim3(512), st, bp, 7,
             rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, qc + 5 * 32, h->rowFlops); }
  if (!mid6 && rows(6, 7) > 0) { hipStream_t st = h->side[2]; KTimer t(h, SPGEMM_K_NUM_HASH4, st);
    const int* sb = h->dsmall->slotBase;
    const int* hs_ = h->mirror.slotBase;
    const int na = hs_[SLOT_H4A + 1] - hs_[SLOT_H4A], nb = hs_[SLOT_H4B + 1] - hs_[SLOT_H4B];
    if (na > 0) LAUNCH_NUM(4, 2048, dim3(clampi(na, 1, cu * 7)), dim3(256), st, sb, SLOT_H4A,
                         rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, qc + 6 * 32, h->rowFlops);
    if (nb > 0) LAUNCH_NUM(4, 4096, dim3(clampi(nb, 1, cu * 4)), dim3(256), st, sb, SLOT_H4B,
                         rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, qc + 7 * 32, h->rowFlops); }
  if (rows(5, 6) > 0) { hipStream_t st = h->side[1]; KTimer t(h, SPGEMM_K_NUM_HASH1, st);
    const int* sb = h->dsmall->slotBase;
    const int* hs_ = h->mirror.slotBase;
    const int na = hs_[SLOT_H1A + 1] - hs_[SLOT_H1A], nb = hs_[SLOT_H1B + 1] - hs_[SLOT_H1B];
    if (na > 0 && !skipH1A) LAUNCH_NUM(1, 512, dim3(grid8(na, cu * h->h1num)), dim3(64), st, sb, SLOT_H1A,
                         rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, qc + 7 * 32, h->rowFlops);
    if (nb > 0) LAUNCH_NUM(1, 1024, dim3(grid8(nb, cu * 16)), dim3(64), st, sb, SLOT_H1B,
                         rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, qc + 7 * 32, h->rowFlops); }
  if (rows(4, 5) > 0) { hipStream_t st = h->side[0]; KTimer t(h, SPGEMM_K_NUM_G16, st);
    with_prune_arg(pcnt, pmode, [&](auto prune) {
      hipLaunchKernelGGL((k_num_g16<float, 128, 4, decltype(prune)::value>), dim3(grid8(cdiv(rows(4, 5), 16), cu * 16)), dim3(256), 0, st,
                         bp, 4, 5, rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, h->rowFlops, pcnt); }); }
  if (minBin <= 1 && rows(1, 4) > 0) { KTimer t(h, SPGEMM_K_NUM_SMALL4);   // 1..16 products: 16-lane flattened kernel, one round per row
    with_prune_arg(pcnt, pmode, [&](auto prune) {
      hipLaunchKernelGGL((k_num_g16<float, 32, 1, decltype(prune)::value>), dim3(grid8(cdiv(rows(1, 4), 16), cu * 16)), dim3(256), 0, h->stream,
                         bp, 1, 4, rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, h->rowFlops, pcnt); }); }
  join_streams(h);
  HIPCHK(hipGetLastError());
  return SPGEMM_OK;
}

// ---- rows up to smallMax products dealt across rows (chain_device.hpp): wave-per-batch kernels
// geometry: waves per block, table slots per wave, blocks per CU; rows up to smallMax products go through k_wbatch, the
// bins from minBin on keep their per-row kernels (skipH1A: of bin 5 only the 257-512 slot)
struct ChainCfg { int nw, tbl, bpc, smallMax, minBin; bool skipH1A; };
static const ChainCfg kChainCfgs[] = {
    {4, 1280, 3, 512, 6, false},
    {6, 1280, 2, 512, 6, false},
    {4, 1024, 3, 256, 5, true},
    {4, 2048, 2, 512, 6, false},
    {8, 1280, 1, 512, 6, false},
};
static const ChainCfg& chain_cfg(const spgemm_handle* h) {
  const int n = (int)(sizeof(kChainCfgs) / sizeof(kChainCfgs[0]));
  return kChainCfgs[h->chainCfg >= 0 && h->chainCfg < n ? h->chainCfg : 0];
}
#ifndef SMF_WB_MAXR
#define SMF_WB_MAXR 2          // rounds of 64 products gathered before the first insert (measured 8 / 4 / 2: 1.68 / 1.42 / 1.33 ms)
#endif

static int launch_cut(spgemm_handle* h, int m) {
  const ChainCfg& c = chain_cfg(h);
  const int ntiles = std::max(1, cdiv(m, SCAN_TILE));
  const CutParams p{c.smallMax, c.tbl - wb_slots(c.smallMax), WAVE};
  clear_stale_hip_error();
  KTimer t(h, SPGEMM_K_CUT);
  hipLaunchKernelGGL(k_cut_sums, dim3(ntiles), dim3(SCAN_THREADS), 0, h->stream, m, h->rowFlops, p, h->tileSum);
  hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, h->stream, ntiles, h->tileSum, &h->dsmall->cutTotal);
  hipLaunchKernelGGL(k_cut_apply, dim3(ntiles), dim3(SCAN_THREADS), 0, h->stream, m, h->rowFlops, p, h->tileSum,
                     h->batchStart, h->chainWords, &h->dsmall->nBatches, &h->dsmall->chainTicket);
  HIPCHK(hipGetLastError());
  return SPGEMM_OK;
}

template <int NW, int TBL, int MODE>
static void launch_wbatch_t(spgemm_handle* h, int blocks, int m, const int* dIA, const float* dA, const int* dJB, const float* dB,
                            int smallMax, int* dIC, int* dJC, float* dC, long long capC) {
  typedef WaveBatchShared<NW, TBL> Sh;
  static bool attr = false;                              // (more than 64 KB of dynamic LDS needs the attribute once)
  if (!attr) { (void)hipFuncSetAttribute((const void*)k_wbatch<NW, TBL, MODE, SMF_WB_MAXR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Sh)); attr = true; }
  hipLaunchKernelGGL((k_wbatch<NW, TBL, MODE, SMF_WB_MAXR>), dim3(blocks), dim3(WAVE * NW), sizeof(Sh), h->stream, m, dIA, h->sbl, dA, dJB, dB,
                     h->rowFlops, smallMax, h->batchStart, &h->dsmall->nBatches, h->chainWords, &h->dsmall->chainTicket, dIC, dJC, dC,
                     capC, &h->dsmall->nnzC64, &h->dsmall->err);
}

template <int MODE>
static int launch_wbatch(spgemm_handle* h, int m, const int* dIA, const float* dA, const int* dJB, const float* dB,
                         int* dIC, int* dJC, float* dC, long long capC) {
  const ChainCfg& c = chain_cfg(h);
  clear_stale_hip_error();
  KTimer t(h, MODE == WB_SYM ? SPGEMM_K_WB_SYM : MODE == WB_NUM ? SPGEMM_K_WB_NUM : SPGEMM_K_CHAIN);
  const int blocks = clampi((long long)h->numCU * c.bpc, 1, 1 << 20);
  switch (h->chainCfg) {
    case 1: launch_wbatch_t<6, 1280, MODE>(h, blocks, m, dIA, dA, dJB, dB, c.smallMax, dIC, dJC, dC, capC); break;
    case 2: launch_wbatch_t<4, 1024, MODE>(h, blocks, m, dIA, dA, dJB, dB, c.smallMax, dIC, dJC, dC, capC); break;
    case 3: launch_wbatch_t<4, 2048, MODE>(h, blocks, m, dIA, dA, dJB, dB, c.smallMax, dIC, dJC, dC, capC); break;
    case 4: launch_wbatch_t<8, 1280, MODE>(h, blocks, m, dIA, dA, dJB, dB, c.smallMax, dIC, dJC, dC, capC); break;
    default: launch_wbatch_t<4, 1280, MODE>(h, blocks, m, dIA, dA, dJB, dB, c.smallMax, dIC, dJC, dC, capC); break;
  }
  HIPCHK(hipGetLastError());
  return SPGEMM_OK;
}

static int check_common(const void* a, const void* b, const void* c, int nnz, const char* who) {
  if (nnz < 0) return fail(SPGEMM_ERR_ARG, "%s: negative nnz", who);
  if (!a) return fail(SPGEMM_ERR_ARG, "%s: rowPtr is null", who);
  if (nnz > 0 && (!b || !c)) return fail(SPGEMM_ERR_ARG, "%s: colInd/values null with nnz=%d", who, nnz);
  return SPGEMM_OK;
}

// `pre` (optional) supplies a classification made earlier by hip_gpuFlopsClassify:
// row ids grouped by bin + dflops + hv.
struct PreClass { const int* drowIds; const int* hv; const int* dflops; };
static int unpack_classification(spgemm_handle* h, int m, const PreClass& pre, int* dIC);

// C = A*B on device arrays as the routes below pass it around, and where the caller wants the result (arrays of the pool)
template <class V> struct Product { const int* IA; const int* JA; const V* A; int nnzA; const int* IB; const int* JB; const V* B; int m, k, n; };
template <class V> struct Result { int** IC; int** JC; V** C; int* nnz; };

// What a route publishes as spgemm_stats from the mirror it read (publish_stats).  Counts and bins always come from the mirror.
enum class StatsForm {
  OneShot,       // phases queued back to back: ms_scan_alloc = ev2->ev4 (scan + allocation of C), ms_total = elapsed ev0->ev5
  OneShotNoNnz,  // the same for the fused R-MCL step without a symbolic pass: nnz(C) is never computed, nnzC = -1
  Symbolic,      // end of a symbolic phase: ms_scan_alloc = ev2->ev3, ms_numeric = 0, ms_total = sum of the parts (numeric_phase adds its own)
  CountsOnly,    // R-MCL loop form: nnzC = -1 and no event is read, the host runs ahead of the stream
  Classified,    // hip_gpuFlopsClassify: no product is computed; nnzC and the phase times are left alone
};

static void publish_stats(spgemm_handle* h, const HostMirror& hm, StatsForm form) {
  spgemm_stats& st = h->stats;
  st.total_flops = (long long)hm.totalP;
  for (int b = 0; b < NBINS; ++b) st.bin_rows[b] = hm.binPtr[b + 1] - hm.binPtr[b];
  if (form == StatsForm::Classified) return collect_kernel_times(h, true);
  st.nnzC = (form == StatsForm::OneShot || form == StatsForm::Symbolic) ? (int)std::min<unsigned long long>(hm.nnzC64, 0x7fffffffULL) : -1;
  if (form == StatsForm::CountsOnly) return;
  const bool twoPhase = form == StatsForm::Symbolic;
  hipEventElapsedTime(&st.ms_classify, h->ev[0], h->ev[1]);
  hipEventElapsedTime(&st.ms_symbolic, h->ev[1], h->ev[2]);
  hipEventElapsedTime(&st.ms_scan_alloc, h->ev[2], h->ev[twoPhase ? 3 : 4]);
  if (twoPhase) {
    st.ms_numeric = 0.f;
    st.ms_total = st.ms_classify + st.ms_symbolic + st.ms_scan_alloc;
  } else {
    hipEventElapsedTime(&st.ms_numeric, h->ev[4], h->ev[5]);
    hipEventElapsedTime(&st.ms_total, h->ev[0], h->ev[5]);
  }
  collect_kernel_times(h, true);
}

// dsmall -> hsmall, then wait for the stream: the host round trip that ends a phase
static bool fetch_mirror(spgemm_handle* h) {
  return hipMemcpyAsync(h->hsmall, h->dsmall, sizeof(HostMirror), hipMemcpyDeviceToHost, h->stream) == hipSuccess &&
         hipStreamSynchronize(h->stream) == hipSuccess;
}

// ... kept as h->mirror, and what the device reported turned into a status; `phase` names the caller in the message.
// `deferred`: error flags the caller handles itself -- when one of them is set the error word is left to the caller.
static int read_mirror(spgemm_handle* h, const char* phase, int deferred = 0) {
  if (!fetch_mirror(h)) return fail(SPGEMM_ERR_HIP, "%s failed: %s", phase, hipGetErrorString(hipGetLastError()));
  h->mirror = *h->hsmall;
  const HostMirror& hm = h->mirror;
  if (hm.err && !(hm.err & deferred)) return fail(SPGEMM_ERR_INTERNAL, "device invariant broken in %s (flags=%d)", phase, hm.err);
  if (hm.nnzC64 > 0x7fffffffULL) return fail(SPGEMM_ERR_OVERFLOW, "nnz(C)=%llu does not fit int32 CSR", hm.nnzC64);
  return SPGEMM_OK;
}

// phase 1, finish: the one host sync (nnzC, bin sizes, error flags); leaves the phase pending for numeric_phase.
// Also ends a one-shot call whose symbolic kernels are queued but whose product is too large to size C by it.
static int finish_symbolic(spgemm_handle* h, int m, int* nnzCp) {
  CHK(read_mirror(h, "symbolic phase"));
  publish_stats(h, h->mirror, StatsForm::Symbolic);
  h->sym_m = m;
  *nnzCp = (int)h->mirror.nnzC64;
  return SPGEMM_OK;
}

// phase 1: classify + symbolic + scan are queued with ev[0..3] around them, then finish_symbolic
static int symbolic_phase(spgemm_handle* h, const int* dIA, const int* dJA, int nnzA, const int* dIB, const int* dJB,
                          int m, int k, int n, const PreClass* pre, int* dIC, int* nnzCp, bool logBig = true) {
  (void)k;
  if (h->failNext > 0) { --h->failNext; return fail(SPGEMM_ERR_INTERNAL, "forced failure (spgemm_hip_debug_fail_next)"); }
  hipStream_t s = h->stream;
  hipEventRecord(h->ev[0], s);
  h->cur_rowIds = h->rowIds;
  if (pre) {
    CHK(unpack_classification(h, m, *pre, dIC));
    h->cur_rowIds = pre->drowIds;
    CHK(ws_ensure_entries(h, nnzA));                 // the caller's classification carries no per-entry records
    if (nnzA > 0)
      hipLaunchKernelGGL(k_entry_lens, dim3(clampi(cdiv(nnzA, 256), 1, h->numCU * 32)), dim3(256), 0, s, nnzA, dJA, dIB, h->sbl);
  } else {
    CHK(launch_classify(h, dIA, dJA, dIB, m, nnzA, dIC));
  }
  hipEventRecord(h->ev[1], s);
  CHK(launch_symbolic(h, dIA, dJB, m, n, h->cur_rowIds, dIC, 0, false, logBig));
  hipEventRecord(h->ev[2], s);
  if (m > 0) CHK(launch_scan(h, dIC, m, &h->dsmall->nnzC64));
  else HIPCHK(hipMemsetAsync(dIC, 0, sizeof(int), s));
  hipEventRecord(h->ev[3], s);
  return finish_symbolic(h, m, nnzCp);
}

// room for the big rows' bitmaps next time (rank kernel only)
static void grow_bitmaps(spgemm_handle* h, int n) {
  const int nbig = h->mirror.binPtr[NBINS] - h->mirror.binPtr[NBINS - 1];
  if (n <= BIG_WC && nbig > h->bm_cap() && h->bigBitmaps.reserve((size_t)(nbig + nbig / 4 + 16) * BIG_WORDS) != hipSuccess)
    (void)hipGetLastError();
}

// room for the big rows' re-hit log next time (direct kernel only).  Size: one metadata slot per big row seen (+25 %), and
// RL_ROW_BUDGET = 2048 log ints per big row, dealt evenly to one region per CU: on the headline matrix a big row logs 930
// re-hits on average (median 816, p99 2285) and the dynamic queue hands a block rows in proportion to their work, so a
// region holds about twice what its block logs.  A row that finds its region full takes the fallback kernel: never wrong.
static void grow_rehit_log(spgemm_handle* h, int n) {
  const int nbig = h->mirror.binPtr[NBINS] - h->mirror.binPtr[NBINS - 1];
  if (!h->bigDirect || n <= BIG_WC || nbig <= h->rl_rows() || nbig < h->bdMinRows) return;   // (too few rows: the log would not be used)
  h->rlMeta.reserve(0); h->rlLog.reserve(0);             // both go before either comes back
  const int cap = nbig + nbig / 4 + 16;
  const long long perBlock = ((long long)cap + h->numCU - 1) / h->numCU * RL_ROW_BUDGET;
  long long region = h->rlRegionEnv > 0 ? h->rlRegionEnv : std::max<long long>(RL_MIN_REGION, perBlock);
  region = std::min<long long>(region, (1ll << 30) / h->numCU);           // entry indices stay ints
  if (h->rlMeta.reserve((size_t)cap) != hipSuccess || h->rlLog.reserve((size_t)region * (size_t)h->numCU) != hipSuccess) {
    (void)hipGetLastError();
    h->rlMeta.reserve(0); h->rlLog.reserve(0);           // one without the other is no log
  }
}

// room for the re-hit log of bins 6-7 next time: what this call's symbolic pass reserved from the cursor -- or would have,
// had the log been there -- plus a quarter, since the dynamic queue deals the rows to the blocks differently every time and
// every block leaves the tail of its last chunk unused.  (Headline matrix: 4.1 M re-hits in 68 K rows.)
static void grow_midrow_log(spgemm_handle* h) {
  const int* hb = h->mirror.binPtr;
  if (!h->mdLogged || std::max(hb[7] - hb[6], hb[8] - hb[7]) < h->mdMinRows) return;   // (too few rows: the log would not be used)
  const long long used = (long long)std::min<unsigned long long>(h->mirror.mrCursor, 1ull << 30);
  if (used == 0 || (h->mrLog && (h->mrLogEnv > 0 || used <= h->mr_cap()))) return;
  const long long want = h->mrLogEnv > 0 ? h->mrLogEnv : std::min<long long>(used + used / 4 + 16 * MD_CHUNK, 1ll << 30);
  if (h->mrLog.reserve((size_t)want) != hipSuccess) (void)hipGetLastError();
}

// ---- double values (spgemm_f64_device.hpp): the numeric phase only; classification, symbolic pass and scan are the
// float pipeline's.  One launch per bin, on the side streams launch_numeric uses, each timed into its bin's slot of
// spgemm_stats.ms_kernel.  Rows of bin 8 wider than the multi-pass LDS kernel takes get device-memory tables: their largest
// length sizes them (one small kernel and a host read, only when bin 8 has rows).
// The launch's own device blocks, owned by the caller until the kernels are done: the probe word pair of bin 8 and the
// device-memory tables (one block: keys, then values)
struct F64Scratch { DevBuf<int> probe; DevBuf<char> tables; };
static int launch_numeric_f64(spgemm_handle* h, const int* dIA, const double* dA, const int* dJB, const double* dB,
                              const int* rowIds, const int* hostBinPtr, const int* dIC, int* dJC, double* dC,
                              F64Scratch* scratch, int* pcnt = nullptr) {
  const int2* sbl = h->sbl;
  clear_stale_hip_error();
  const int* bp = h->dsmall->binPtr;
  int* err = &h->dsmall->err;
  const int cu = h->numCU;
  hipStream_t s = h->stream;
  auto rows = [&](int lo, int hi) { return hostBinPtr[hi] - hostBinPtr[lo]; };
  // pcnt: the fused R-MCL step (PRUNE of the numeric kernels) --the same launches with the row rule in their epilogues
  auto fused = [&](auto launch) { if (pcnt) launch(std::true_type()); else launch(std::false_type()); };
  int wide[2] = {0, 0};                                // largest L_i of the rows beyond F64_PASS_MAXL, their number
  int* gkeys = nullptr;
  double* gvals = nullptr;
  int gslots = 0, gblocks = 0;
  if (rows(8, 9) > 0) {
    HIPCHK(scratch->probe.alloc(2));
    int* const dw = scratch->probe;
    HIPCHK(hipMemsetAsync(dw, 0, sizeof(int) * 2, s));
    hipLaunchKernelGGL(k_num64_wide_rows, dim3(clampi(cdiv(rows(8, 9), 256), 1, cu)), dim3(256), 0, s, bp, 8, rowIds, dIC,
                       F64_PASS_MAXL, dw);
    if (hipMemcpyAsync(wide, dw, sizeof(wide), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(SPGEMM_ERR_HIP, "f64 wide-row probe failed: %s", hipGetErrorString(hipGetLastError()));
    if (wide[1] > 0) {
      gslots = 64;
      while (gslots < 2 * wide[0]) gslots <<= 1;
      const size_t perBlock = (size_t)gslots * (sizeof(int) + sizeof(double));
      gblocks = (int)std::max<size_t>(1, std::min<size_t>({(size_t)wide[1], (size_t)cu, (size_t(1) << 30) / perBlock}));
      // one allocation: keys, then values (8-byte aligned: gslots is a multiple of 64)
      HIPCHK(scratch->tables.alloc(perBlock * (size_t)gblocks));
      gkeys = reinterpret_cast<int*>(scratch->tables.p);
      gvals = reinterpret_cast<double*>(gkeys + (size_t)gslots * gblocks);
    }
  }
  fork_streams(h);
  if (rows(8, 9) > 0) {
    hipStream_t st = h->side[3];
    { KTimer t(h, SPGEMM_K_NUM_BIG, st);
      fused([&](auto P) {
        hipLaunchKernelGGL((k_num64_rows<F64_BIG_THREADS, F64_LDS_TBL, false, decltype(P)::value>), dim3(clampi(rows(8, 9), 1, cu)),
                           dim3(F64_BIG_THREADS), 0, st, bp, 8, rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, 0,
                           F64_PASS_MAXL, (int*)nullptr, (double*)nullptr, 0, pcnt); }); }
    // (device-memory rows are written in full either way: no fused form)
    if (gblocks > 0 || pcnt) { KTimer t(h, SPGEMM_K_NUM_BIGHASH, st);
      if (gblocks > 0)
      hipLaunchKernelGGL((k_num64_rows<F64_BIG_THREADS, 1, true>), dim3(gblocks), dim3(F64_BIG_THREADS), 0, st, bp, 8,
                         rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, F64_PASS_MAXL + 1, 0x7fffffff, gkeys, gvals, gslots,
                         (int*)nullptr);
      // fused step: the rows that pass through LDS in pieces or through a device-memory table were written in full --
      // the row rule in place, behind both kernels on their stream (timed with the device-memory kernel's slot)
      if (pcnt)
        hipLaunchKernelGGL(k_rmcl_fix_rows<double>, dim3(clampi(rows(8, 9), 1, cu * 4)), dim3(256), 0, st, bp, 8, 9, rowIds, dIC, dJC,
                           dC, pcnt, F64_LDS_MAXL); }
  }
  if (rows(7, 8) > 0) { hipStream_t st = h->side[2]; KTimer t(h, SPGEMM_K_NUM_HASH8, st);
    fused([&](auto P) {
      hipLaunchKernelGGL((k_num64_rows<512, 8192, false, decltype(P)::value>), dim3(clampi(rows(7, 8), 1, cu)), dim3(512), 0, st, bp, 7,
                         rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, 0, 0x7fffffff, (int*)nullptr, (double*)nullptr, 0, pcnt); }); }
  if (rows(6, 7) > 0) { hipStream_t st = h->side[2]; KTimer t(h, SPGEMM_K_NUM_HASH4, st);
    fused([&](auto P) {
      hipLaunchKernelGGL((k_num64_rows<256, 4096, false, decltype(P)::value>), dim3(clampi(rows(6, 7), 1, cu * 3)), dim3(256), 0, st, bp, 6,
                         rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, 0, 0x7fffffff, (int*)nullptr, (double*)nullptr, 0, pcnt); }); }
  if (rows(5, 6) > 0) { hipStream_t st = h->side[1]; KTimer t(h, SPGEMM_K_NUM_HASH1, st);
    fused([&](auto P) {
      hipLaunchKernelGGL((k_num64_rows<64, 1024, false, decltype(P)::value>), dim3(clampi(rows(5, 6), 1, cu * 12)), dim3(64), 0, st, bp, 5,
                         rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, 0, 0x7fffffff, (int*)nullptr, (double*)nullptr, 0, pcnt); }); }
  if (rows(4, 5) > 0) { hipStream_t st = h->side[0]; KTimer t(h, SPGEMM_K_NUM_G16, st);
    fused([&](auto P) {
      hipLaunchKernelGGL((k_num_g16<double, 128, 4, decltype(P)::value>), dim3(grid8(cdiv(rows(4, 5), 16), cu * 16)), dim3(256), 0, st, bp, 4, 5,
                         rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, h->rowFlops, pcnt); }); }
  if (rows(1, 4) > 0) { KTimer t(h, SPGEMM_K_NUM_SMALL4);
    fused([&](auto P) {
      hipLaunchKernelGGL((k_num_g16<double, 32, 1, decltype(P)::value>), dim3(grid8(cdiv(rows(1, 4), 16), cu * 16)), dim3(256), 0, s, bp, 1, 4,
                         rowIds, dIA, sbl, dA, dJB, dB, dIC, dJC, dC, err, h->rowFlops, pcnt); }); }
  join_streams(h);
  HIPCHK(hipGetLastError());
  return SPGEMM_OK;
}

// the numeric launch of either value type behind one name (`scratch`: double only)
static int launch_numeric_of(spgemm_handle* h, const int* dIA, const float* dA, const int* dJB, const float* dB, int n,
                             const int* dIC, int* dJC, float* dC, F64Scratch*) {
  return launch_numeric(h, dIA, dA, dJB, dB, n, h->cur_rowIds, h->mirror.binPtr, dIC, dJC, dC);
}
static int launch_numeric_of(spgemm_handle* h, const int* dIA, const double* dA, const int* dJB, const double* dB, int,
                             const int* dIC, int* dJC, double* dC, F64Scratch* scratch) {
  return launch_numeric_f64(h, dIA, dA, dJB, dB, h->cur_rowIds, h->mirror.binPtr, dIC, dJC, dC, scratch);
}

// phase 2: numeric into dJC/dC, which it borrows like dIC (the caller's own, or the product routes' C); one host sync at
// the end (error flags)
template <class V>
static int numeric_phase(spgemm_handle* h, const int* dIA, const int* dJA, const V* dA, const int* dIB, const int* dJB,
                         const V* dB, int m, int n, const int* dIC, int* dJC, V* dC) {
  (void)dJA; (void)dIB;
  constexpr bool isFloat = std::is_same<V, float>::value;
  if (h->sym_m != m) return fail(SPGEMM_ERR_ARG, "numeric phase without a matching symbolic phase on this handle");
  hipStream_t s = h->stream;
  const int nnzC = (int)h->mirror.nnzC64;
  F64Scratch scratch;
  hipEventRecord(h->ev[4], s);
  if (m > 0 && nnzC > 0) {
    if (!dJC || !dC) return fail(SPGEMM_ERR_ARG, "output buffers are null");
    if (int rc = launch_numeric_of(h, dIA, dA, dJB, dB, n, dIC, dJC, dC, &scratch)) return drained(s, rc);
  }
  hipEventRecord(h->ev[5], s);
  // (only the error word: the rest of the mirror was read at the end of the symbolic phase)
  if (hipMemcpyAsync(&h->hsmall->err, &h->dsmall->err, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return drained(s, fail(SPGEMM_ERR_HIP, "numeric phase failed: %s", hipGetErrorString(hipGetLastError())));
  h->sym_m = -1;                                       // (the stream is idle from here on)
  if (!(kAblate && isFloat) && h->hsmall->err)
    return fail(SPGEMM_ERR_INTERNAL, "device invariant broken in numeric phase (flags=%d)", h->hsmall->err);
  spgemm_stats& st = h->stats;
  hipEventElapsedTime(&st.ms_numeric, h->ev[4], h->ev[5]);
  st.ms_total += st.ms_numeric;
  collect_kernel_times(h, false);
  if (isFloat) { grow_bitmaps(h, n); grow_rehit_log(h, n); grow_midrow_log(h); }
  return SPGEMM_OK;
}

// The C of a product lives in ONE DevCSRT<V> in the frame of the entry point's route (spgemm_device, hip_gpuSpMM_f64):
// begin_product allocates its rowPtr, finish_exact or one_shot_back its colInd/values, and success ends in give() into the
// caller's Result<V>.  The functions in between fill it and return a status; on an error the frame drains the stream (rule A)
// and the blocks go back with the object.
//
// The end of every route that has nnz(C) on the host: allocate colInd/values exactly and run the numeric phase.
template <class V>
static int finish_exact(spgemm_handle* h, const Product<V>& p, int nnzC, DevCSRT<V>* C) {
  if (C->alloc_entries(nnzC) != hipSuccess) return fail(SPGEMM_ERR_HIP, "device allocation of C (%d entries) failed", nnzC);
  C->nnz = nnzC;
  return numeric_phase(h, p.IA, p.JA, p.A, p.IB, p.JB, p.B, p.m, p.n, C->I, C->J, C->V.p);
}

// the two-phase pipeline from its start: symbolic phase, exact allocation, numeric phase
template <class V>
static int two_phase(spgemm_handle* h, const Product<V>& p, const PreClass* pre, DevCSRT<V>* C) {
  int nnzC = 0;
  // (a double product's numeric kernels have no use for the big rows' re-hit log)
  CHK(symbolic_phase(h, p.IA, p.JA, p.nnzA, p.IB, p.JB, p.m, p.k, p.n, pre, C->I, &nnzC, std::is_same<V, float>::value));
  return finish_exact(h, p, nnzC, C);
}

// what the C-producing entry points do first: outputs cleared, arguments checked, handle, device, workspace, C.rowPtr
template <class V>
static int begin_product(spgemm_handle** hp, const Product<V>& p, int nnzB, const Result<V>& out, DevCSRT<V>* C) {
  if (!out.IC || !out.JC || !out.C || !out.nnz) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *out.IC = nullptr; *out.JC = nullptr; *out.C = nullptr; *out.nnz = 0;
  if (p.m < 0 || p.k < 0 || p.n < 0) return fail(SPGEMM_ERR_ARG, "negative dimension m=%d k=%d n=%d", p.m, p.k, p.n);
  CHK(check_common(p.IA, p.JA, p.A, p.nnzA, "A"));
  CHK(check_common(p.IB, p.JB, p.B, nnzB, "B"));
  if (!*hp) CHK(default_handle(hp));
  HIPCHK(hipSetDevice((*hp)->device));
  CHK(ws_ensure(*hp, p.m));
  HIPCHK(C->I.alloc((size_t)p.m + 1));
  return SPGEMM_OK;
}

// ---- hip_gpuSpMM without a caller's classification.  SPGEMM_PATH (opt-in): rows up to ChainCfg::smallMax products are dealt
// across rows by the wave-per-batch kernels (chain_device.hpp, round 4) -- pathMode 1 in two passes (counts, scan, entries),
// pathMode 2 in ONE pass (no symbolic pass, no scan: a chained prefix places them); the bins above keep their per-row kernels.
struct OptInPath { bool chain, wb2; int minBin; bool skipH1A; };
static OptInPath opt_in_path(const spgemm_handle* h) {
  const bool chain = h->pathMode == 2, wb2 = h->pathMode == 1;
  return {chain, wb2, (chain || wb2) ? chain_cfg(h).minBin : 0, (chain || wb2) && chain_cfg(h).skipH1A};
}

// Front half: classification, symbolic kernels and scan are queued with no host round trip; the classification (bin sizes,
// P) is copied to the host while the symbolic kernels run and lands in *mid.
static int one_shot_front(spgemm_handle* h, const Product<float>& p, const OptInPath& o, int* dIC, HostMirror* mid) {
  hipStream_t s = h->stream;
  hipEventRecord(h->ev[0], s);
  h->cur_rowIds = h->rowIds;
  CHK(launch_classify(h, p.IA, p.JA, p.IB, p.m, p.nnzA, dIC));
  if (o.chain || o.wb2) CHK(launch_cut(h, p.m));
  hipEventRecord(h->ev[1], s);
  if (hipMemcpyAsync(h->hmid, h->dsmall, sizeof(HostMirror), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipEventRecord(h->evMid, s) != hipSuccess)
    return fail(SPGEMM_ERR_HIP, "classification copy failed: %s", hipGetErrorString(hipGetLastError()));
  if (o.wb2) CHK(launch_wbatch<WB_SYM>(h, p.m, p.IA, nullptr, p.JB, nullptr, dIC, nullptr, nullptr, 0));
  // k_sym_midpair for bin 6: the handle's previous product looked the same and had enough such rows (spMinRows)
  const bool pairOk = h->spMinRows <= 0 || (h->spPrevM == p.m && h->spPrevN == p.n && h->spPrevNnzA == (long long)p.nnzA &&
                                            h->spPrevRows6 >= h->spMinRows);
  CHK(launch_symbolic(h, p.IA, p.JB, p.m, p.n, h->cur_rowIds, dIC, o.minBin, o.skipH1A, true, pairOk));
  hipEventRecord(h->ev[2], s);
  if (!o.chain) CHK(launch_scan(h, dIC, p.m, &h->dsmall->nnzC64));
  hipEventRecord(h->ev[3], s);
  if (hipEventSynchronize(h->evMid) != hipSuccess)
    return fail(SPGEMM_ERR_HIP, "classification failed: %s", hipGetErrorString(hipGetLastError()));
  *mid = *h->hmid;
  h->spPrevM = p.m; h->spPrevN = p.n; h->spPrevNnzA = (long long)p.nnzA;
  h->spPrevRows6 = mid->binPtr[7] - mid->binPtr[6];
  return SPGEMM_OK;
}

// Back half: colInd/values are allocated with capC entries -- P, an upper bound of nnz(C) (8*P bytes: HBM is 288 GB), or on
// the one-pass path what the previous, identical-looking call produced (the kernels never write past that and say so if it
// was not enough) -- so that the numeric kernels can be queued right behind the scan; nnz(C) and the error flags are read
// once, at the end.
static int one_shot_back(spgemm_handle* h, const Product<float>& p, const OptInPath& o, const HostMirror& mid, size_t capC, DevCSR* C) {
  const unsigned long long P = mid.totalP;
  hipStream_t s = h->stream;
  if (C->J.alloc(capC) != hipSuccess || C->V.alloc(capC) != hipSuccess)
    return fail(SPGEMM_ERR_HIP, "device allocation of C (%llu entries) failed", P);
  hipEventRecord(h->ev[4], s);
  h->mirror = mid;                                     // bin sizes for the numeric launch grids
  if (o.chain) CHK(launch_wbatch<WB_CHAIN>(h, p.m, p.IA, p.A, p.JB, p.B, C->I, C->J, C->V, (long long)capC));
  if (o.wb2 && P > 0) CHK(launch_wbatch<WB_NUM>(h, p.m, p.IA, p.A, p.JB, p.B, C->I, C->J, C->V, (long long)capC));
  if (P > 0) CHK(launch_numeric(h, p.IA, p.A, p.JB, p.B, p.n, h->cur_rowIds, mid.binPtr, C->I, C->J, C->V, nullptr, 1, o.minBin, o.skipH1A));
  hipEventRecord(h->ev[5], s);
  const int rc = read_mirror(h, "SpGEMM", kAblate ? ~0 : o.chain ? ERRF_CHAIN_CAP : 0);
  if (rc != SPGEMM_ERR_HIP) h->sym_m = -1;             // the mirror of a pending symbolic phase is gone
  if (rc) return rc;
  const HostMirror& hm = h->mirror;
  if (o.chain && (hm.err & ERRF_CHAIN_CAP)) {          // (this condition misses overflows in rows above smallMax: ADVICE.md)
    // C sized from the previous call was too small for this product (same shape and product count, more distinct
    // columns): nothing was written out of bounds; forget the guess and compute the product the two-phase way
    C->J.reset(); C->V.reset();
    h->prev_m = -1; h->prev_nnzC = -1;
    return two_phase(h, p, nullptr, C);
  }
  publish_stats(h, hm, StatsForm::OneShot);
  grow_bitmaps(h, p.n);
  grow_rehit_log(h, p.n);
  grow_midrow_log(h);
  h->prev_m = p.m; h->prev_P = P; h->prev_nnzC = (long long)hm.nnzC64;
  C->nnz = (int)hm.nnzC64;
  return SPGEMM_OK;
}

// C = A*B in float, five routes:
//   1 one-shot            C sized by P, one host sync at the end (the default)
//   2 capacity redo       one-pass path only: C sized by the previous call was too small, two-phase pipeline from its start
//   3 chain, P too large  the one-pass path queued only part of the symbolic kernels: two-phase pipeline from its start
//   4 P too large         P > 2^30, or a product known to compress: the queued symbolic phase is finished, C sized exactly
//   5 pre-classified      a caller's classification, or no rows: two-phase pipeline
// prev_m/prev_P/prev_nnzC (allocation policy of the next call): set by routes 1, 3 and 4, reset by 2, left alone by 5.
static int product_routes(spgemm_handle* h, const Product<float>& p, const PreClass* pre, DevCSR* C) {
  if (pre || p.m == 0) return two_phase(h, p, pre, C);                                         // route 5
  const OptInPath o = opt_in_path(h);
  HostMirror mid;
  CHK(one_shot_front(h, p, o, C->I, &mid));
  const unsigned long long P = mid.totalP;
  // A product that compresses (real web graphs: nnz(C)/P ~ 0.5) would hold twice the memory it needs when sized by P.
  // The handle remembers the previous call: the same shape and product count with nnz(C) < 3/4 P sends this call down
  // the two-phase path (exact allocation, one more host round trip -- cheap next to the halved footprint).
  const bool compressive = h->prev_m == p.m && h->prev_P == P && h->prev_nnzC >= 0 && (double)h->prev_nnzC < 0.75 * (double)P;
  if (P <= (1ull << 30) && (!compressive || o.chain)) {
    const size_t capC = compressive ? (size_t)std::max<long long>(h->prev_nnzC, 1ll) : (size_t)std::max<unsigned long long>(P, 1ull);
    return one_shot_back(h, p, o, mid, capC, C);                                                // routes 1 and 2
  }
  int nnzC = 0;
  CHK(o.chain ? symbolic_phase(h, p.IA, p.JA, p.nnzA, p.IB, p.JB, p.m, p.k, p.n, nullptr, C->I, &nnzC)   // route 3
              : finish_symbolic(h, p.m, &nnzC));                                                      // route 4
  h->prev_m = p.m; h->prev_P = P; h->prev_nnzC = nnzC;
  return finish_exact(h, p, nnzC, C);
}

static int spgemm_device(spgemm_handle* h, const Product<float>& p, int nnzB, const PreClass* pre, const Result<float>& out) {
  DevCSR C;
  CHK(begin_product(&h, p, nnzB, out, &C));
  if (int rc = product_routes(h, p, pre, &C)) return drained(h->stream, rc);
  C.give(out.IC, out.JC, out.C, out.nnz);
  return SPGEMM_OK;
}

extern "C" int hip_gpuSpMM(spgemm_handle* h, const int* dIA, const int* dJA, const float* dA, int nnzA,
                           const int* dIB, const int* dJB, const float* dB, int nnzB, int m, int k, int n,
                           int** dIC, int** dJC, float** dC, int* nnzC) {
  return spgemm_device(h, {dIA, dJA, dA, nnzA, dIB, dJB, dB, m, k, n}, nnzB, nullptr, {dIC, dJC, dC, nnzC});
}

extern "C" int hip_spgemm_symbolic(spgemm_handle* h, const int* dIA, const int* dJA, int nnzA, const int* dIB,
                                   const int* dJB, int nnzB, int m, int k, int n, int* dIC, int* nnzC) {
  if (!h) return fail(SPGEMM_ERR_ARG, "hip_spgemm_symbolic needs a handle");
  if (!dIC || !nnzC) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  if (m < 0 || k < 0 || n < 0) return fail(SPGEMM_ERR_ARG, "negative dimension");
  CHK(check_common(dIA, dJA, dJA, nnzA, "A"));
  CHK(check_common(dIB, dJB, dJB, nnzB, "B"));
  HIPCHK(hipSetDevice(h->device));
  CHK(ws_ensure(h, m));
  return symbolic_phase(h, dIA, dJA, nnzA, dIB, dJB, m, k, n, nullptr, dIC, nnzC);
}

extern "C" int hip_spgemm_numeric(spgemm_handle* h, const int* dIA, const int* dJA, const float* dA, int nnzA,
                                  const int* dIB, const int* dJB, const float* dB, int nnzB, int m, int k, int n,
                                  const int* dIC, int* dJC, float* dC) {
  (void)k;
  if (!h) return fail(SPGEMM_ERR_ARG, "hip_spgemm_numeric needs a handle");
  if (!dIC) return fail(SPGEMM_ERR_ARG, "dIC is null");
  CHK(check_common(dIA, dJA, dA, nnzA, "A"));
  CHK(check_common(dIB, dJB, dB, nnzB, "B"));
  HIPCHK(hipSetDevice(h->device));
  return numeric_phase(h, dIA, dJA, dA, dIB, dJB, dB, m, n, dIC, dJC, dC);
}

// double values: the two-phase pipeline with the f64 numeric launch (never the opt-in SPGEMM_PATH kernels)
extern "C" int hip_gpuSpMM_f64(spgemm_handle* h, const int* dIA, const int* dJA, const double* dA, int nnzA,
                               const int* dIB, const int* dJB, const double* dB, int nnzB, int m, int k, int n,
                               int** dICp, int** dJCp, double** dCp, int* nnzCp) {
  const Product<double> p{dIA, dJA, dA, nnzA, dIB, dJB, dB, m, k, n};
  const Result<double> out{dICp, dJCp, dCp, nnzCp};
  DevCSRT<double> C;
  CHK(begin_product(&h, p, nnzB, out, &C));
  if (int rc = two_phase(h, p, nullptr, &C)) return drained(h->stream, rc);
  C.give(out.IC, out.JC, out.C, out.nnz);
  return SPGEMM_OK;
}

extern "C" int hip_spgemm_numeric_f64(spgemm_handle* h, const int* dIA, const int* dJA, const double* dA, int nnzA,
                                      const int* dIB, const int* dJB, const double* dB, int nnzB, int m, int k, int n,
                                      const int* dIC, int* dJC, double* dC) {
  (void)k;
  if (!h) return fail(SPGEMM_ERR_ARG, "hip_spgemm_numeric_f64 needs a handle");
  if (!dIC) return fail(SPGEMM_ERR_ARG, "dIC is null");
  CHK(check_common(dIA, dJA, dA, nnzA, "A"));
  CHK(check_common(dIB, dJB, dB, nnzB, "B"));
  HIPCHK(hipSetDevice(h->device));
  return numeric_phase(h, dIA, dJA, dA, dIB, dJB, dB, m, n, dIC, dJC, dC);
}

extern "C" int hip_csr_row_flops(spgemm_handle* h, const int* dIA, const int* dJA, const int* dIB, int m,
                                 int* dRowFlops, long long* total_flops) {
  if (!h) CHK(default_handle(&h));
  if (m < 0 || !dIA || (m > 0 && !dRowFlops)) return fail(SPGEMM_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(h->device));
  h->sym_m = -1;                                   // the classification workspace is about to be overwritten
  CHK(ws_ensure(h, m));
  hipStream_t s = h->stream;
  DevBuf<int> tmpIC;
  HIPCHK(tmpIC.alloc((size_t)m + 1));
  if (int rc = launch_classify(h, dIA, dJA, dIB, m, -1, tmpIC)) return drained(s, rc);
  if (m > 0 && hipMemcpyAsync(dRowFlops, h->rowFlops, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return drained(s, fail(SPGEMM_ERR_HIP, "copy of row flops failed"));
  if (!fetch_mirror(h)) return drained(s, fail(SPGEMM_ERR_HIP, "row flops failed: %s", hipGetErrorString(hipGetLastError())));
  collect_kernel_times(h, true);
  if (total_flops) *total_flops = (long long)h->hsmall->totalP;
  return SPGEMM_OK;
}

// ------------------------------------------------------------------------------------------------
// classification API (reference-shaped outputs)
// ------------------------------------------------------------------------------------------------
static void hv_from_binptr(const int* binPtr, int hv[SPGEMM_HV_LEN], int* hv_len) {
  // reference bins (dqueueId): 1:{0} 2:{1} 3:{2..4} 4:{5..16} 5:{17..64} 6:{65..512} 7:{>512}; element 0 of the
  // (m+1)-long bin array is a dummy with 0 flops (bin 1).  Internal bins 6,7,8 together are reference bin 7.
  int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  cnt[1] = 1 + (binPtr[1] - binPtr[0]);
  cnt[2] = binPtr[2] - binPtr[1];
  cnt[3] = binPtr[3] - binPtr[2];
  cnt[4] = binPtr[4] - binPtr[3];
  cnt[5] = binPtr[5] - binPtr[4];
  cnt[6] = binPtr[6] - binPtr[5];
  cnt[7] = binPtr[NBINS] - binPtr[6];
  hv[0] = 0;
  int maxbin = 1;
  for (int b = 0; b < 8; ++b) { hv[b + 1] = hv[b] + cnt[b]; if (cnt[b] > 0) maxbin = b; }
  *hv_len = maxbin + 2;
}

extern "C" int hip_gpuFlopsClassify(spgemm_handle* h, const int* dIA, const int* dJA, const int* dIB, int m, int k,
                                    int** drowIds, int** dflops, int hv[SPGEMM_HV_LEN], int* hv_len,
                                    long long* total_flops) {
  (void)k;
  if (!drowIds || !dflops || !hv || !hv_len) return fail(SPGEMM_ERR_ARG, "null output pointer");
  *drowIds = nullptr; *dflops = nullptr;
  if (m < 0) return fail(SPGEMM_ERR_ARG, "negative m");
  if (!dIA) return fail(SPGEMM_ERR_ARG, "A.rowPtr is null");
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  h->sym_m = -1;
  CHK(ws_ensure(h, m));
  DevBuf<int> ids, fl, tmpIC;
  HIPCHK(ids.alloc((size_t)std::max(m, 1)));
  if (fl.alloc((size_t)m + 1) != hipSuccess || tmpIC.alloc((size_t)m + 1) != hipSuccess)
    return fail(SPGEMM_ERR_HIP, "device allocation failed");
  hipStream_t s = h->stream;
  if (int rc = launch_classify(h, dIA, dJA, dIB, m, -1, tmpIC)) return drained(s, rc);
  if (m > 0) {
    hipMemcpyAsync(ids, h->rowIds, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, s);
    hipLaunchKernelGGL(k_gather_flops, dim3(cdiv(m, 256)), dim3(256), 0, s, m, h->rowIds, h->rowFlops, fl.p);
    if (int rc = launch_scan(h, fl, m, &h->dsmall->nnzC64, false)) return drained(s, rc);   // wraps: differences stay exact
  } else {
    hipMemsetAsync(fl, 0, sizeof(int), s);
  }
  if (!fetch_mirror(h)) return drained(s, fail(SPGEMM_ERR_HIP, "classify failed: %s", hipGetErrorString(hipGetLastError())));
  hv_from_binptr(h->hsmall->binPtr, hv, hv_len);
  if (total_flops) *total_flops = (long long)h->hsmall->totalP;
  publish_stats(h, *h->hsmall, StatsForm::Classified);
  *drowIds = ids.release();                            // the caller's now (spgemm_hip_free); tmpIC goes back here
  *dflops = fl.release();
  return SPGEMM_OK;
}

// rebuild the internal view (rowFlops by row, 9-bin binPtr, IC presets) from a caller-held classification
__global__ void k_unpack_classify(int m, const int* __restrict__ rowIds, const int* __restrict__ dflops,
                                  int* __restrict__ rowFlops, int* __restrict__ IC, int lo6, int* __restrict__ n67) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  int is6 = 0, is7 = 0, is5a = 0, is6a = 0;
  if (q < m) {
    const int r = rowIds[q];
    // dflops is an int scan (like the reference's): differences stay exact modulo 2^32
    const unsigned f = (unsigned)dflops[q + 1] - (unsigned)dflops[q];
    rowFlops[r] = f > 0x7fffffffu ? 0x7fffffff : (int)f;
    if (f <= 1u) IC[r] = (int)f;
    is6 = (q >= lo6 && f <= 2048u) ? 1 : 0;
    is7 = (q >= lo6 && f > 2048u && f <= 4096u) ? 1 : 0;
    is5a = (f > 64u && f <= (unsigned)smf::H1A_MAX) ? 1 : 0;
    is6a = (q >= lo6 && f <= (unsigned)smf::H4A_MAX) ? 1 : 0;
  }
  const unsigned long long m6 = __ballot(is6), m7 = __ballot(is7), m5 = __ballot(is5a), m6a = __ballot(is6a);
  if (smf::lane_id() == 0) {
    if (m6a) atomicAdd(&n67[3], __popcll(m6a));
    if (m6) atomicAdd(&n67[0], __popcll(m6));
    if (m7) atomicAdd(&n67[1], __popcll(m7));
    if (m5) atomicAdd(&n67[2], __popcll(m5));
  }
}

__global__ void k_binptr_from_hv(int* binPtr, int* slotBase, int h2, int h3, int h4, int h5, int h6, int h7, int m,
                                 const int* n67) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    binPtr[0] = 0; binPtr[1] = h2 - 1; binPtr[2] = h3 - 1; binPtr[3] = h4 - 1; binPtr[4] = h5 - 1;
    binPtr[5] = h6 - 1; binPtr[6] = h7 - 1; binPtr[7] = h7 - 1 + n67[0]; binPtr[8] = binPtr[7] + n67[1]; binPtr[9] = m;
    // the two layout slots of bin 5 (the classification came from hip_gpuFlopsClassify: <=256 products first)
    slotBase[smf::SLOT_H1A] = binPtr[5]; slotBase[smf::SLOT_H1B] = binPtr[5] + n67[2]; slotBase[smf::SLOT_H4A] = binPtr[6];
    slotBase[smf::SLOT_H4B] = binPtr[6] + n67[3]; slotBase[smf::SLOT_H8] = binPtr[7];
  }
}

static int unpack_classification(spgemm_handle* h, int m, const PreClass& pre, int* dIC) {
  if (!pre.drowIds || !pre.hv || !pre.dflops) return fail(SPGEMM_ERR_ARG, "classification pointers are null");
  const int* hv = pre.hv;
  for (int b = 0; b < 8; ++b)
    if (hv[b] > hv[b + 1]) return fail(SPGEMM_ERR_ARG, "hv is not monotone");
  if (hv[8] != m + 1 || hv[1] != 0 || hv[2] < 1) return fail(SPGEMM_ERR_ARG, "hv does not describe %d rows", m);
  clear_stale_hip_error();
  HIPCHK(hipMemsetAsync(h->dsmall, 0, sizeof(HostMirror), h->stream));
  if (m > 0) {
    int* n67 = h->dsmall->scratch2;
    hipLaunchKernelGGL(k_unpack_classify, dim3(cdiv(m, 256)), dim3(256), 0, h->stream, m, pre.drowIds, pre.dflops,
                       h->rowFlops, dIC, hv[7] - 1, n67);
    hipLaunchKernelGGL(k_binptr_from_hv, dim3(1), dim3(64), 0, h->stream, h->dsmall->binPtr, h->dsmall->slotBase, hv[2], hv[3], hv[4], hv[5],
                       hv[6], hv[7], m, n67);
  }
  HIPCHK(hipGetLastError());
  return SPGEMM_OK;
}

extern "C" int hip_sgpuSpMM(spgemm_handle* h, const int* dIA, const int* dJA, const float* dA, int nnzA,
                            const int* dIB, const int* dJB, const float* dB, int nnzB, int m, int k, int n,
                            const int* drowIds, const int hv[SPGEMM_HV_LEN], const int* dflops, int** dIC, int** dJC,
                            float** dC, int* nnzC) {
  PreClass pre{drowIds, hv, dflops};
  return spgemm_device(h, {dIA, dJA, dA, nnzA, dIB, dJB, dB, m, k, n}, nnzB, &pre, {dIC, dJC, dC, nnzC});
}

// ------------------------------------------------------------------------------------------------
// host arrays in / host arrays out
// ------------------------------------------------------------------------------------------------
static int validate_host_csr(const int* I, const int* J, int rows, int cols, int nnz, const char* who) {
  if (I[0] != 0) return fail(SPGEMM_ERR_INPUT, "%s: rowPtr[0]=%d, expected 0", who, I[0]);
  for (int i = 0; i < rows; ++i)
    if (I[i + 1] < I[i]) return fail(SPGEMM_ERR_INPUT, "%s: rowPtr decreases at row %d", who, i);
  if (I[rows] != nnz) return fail(SPGEMM_ERR_INPUT, "%s: rowPtr[rows]=%d but nnz=%d", who, I[rows], nnz);
  for (int p = 0; p < nnz; ++p)
    if ((unsigned)J[p] >= (unsigned)cols) return fail(SPGEMM_ERR_INPUT, "%s: colInd[%d]=%d outside [0,%d)", who, p, J[p], cols);
  return SPGEMM_OK;
}

// Pageable host memory <-> device at PCIe speed.  The caller's arrays are plain malloc memory (the reference's
// CSR::dispose() is free(), nlibs/CSR.h:323-327), and for the outputs they are fresh: a blocking hipMemcpy moves them
// through the runtime's single staging thread (page faults of 1.8 GB of untouched memory included) at a fraction of the
// link rate.  Here T threads each own a contiguous slice, a private stream and two pinned 4 MB slots: while one slot is
// on the link the thread moves the other between slot and destination, so the faults and the memcpy of the slices run
// in parallel and the link stays busy.  Slots are allocated once per process.
namespace {
struct CopyLanes {
  static constexpr int T = 8;
  static constexpr size_t SLOT = size_t(4) << 20;
  PinBlock<char> slot[T][2];
  hipEvent_t done[T][2] = {};                         // "the copy out of this slot has finished" (host -> device direction)
  hipStream_t st[T] = {};
  int device = -1;
  std::mutex mu;
  int ensure(int dev) {
    if (device == dev && slot[0][0]) return SPGEMM_OK;
    release();
    for (int t = 0; t < T; ++t) {
      HIPCHK(hipStreamCreateWithFlags(&st[t], hipStreamNonBlocking));
      for (int b = 0; b < 2; ++b) {
        HIPCHK(slot[t][b].reserve(SLOT));
        HIPCHK(hipEventCreateWithFlags(&done[t][b], hipEventDisableTiming));
      }
    }
    device = dev;
    return SPGEMM_OK;
  }
  void release() {
    for (int t = 0; t < T; ++t) {
      for (int b = 0; b < 2; ++b) {
        slot[t][b].reserve(0);
        if (done[t][b]) hipEventDestroy(done[t][b]);
        done[t][b] = nullptr;
      }
      if (st[t]) hipStreamDestroy(st[t]);
      st[t] = nullptr;
    }
    device = -1;
  }
};
CopyLanes& lanes() { static CopyLanes* l = new CopyLanes(); return *l; }

// one thread's slice; toDevice: host -> device, else device -> host
hipError_t lane_copy(int dev, hipStream_t st, char* const slots[2], hipEvent_t const done[2], char* host, char* devp, size_t bytes,
                     bool toDevice) {
  hipError_t e = hipSetDevice(dev);
  if (e != hipSuccess) return e;
  const size_t S = CopyLanes::SLOT;
  const size_t n = (bytes + S - 1) / S;
  if (toDevice) {
    for (size_t c = 0; c < n; ++c) {
      const size_t off = c * S, len = std::min(S, bytes - off);
      char* sl = slots[c & 1];
      // wait only for THIS slot's previous transfer (chunk c-2): chunk c-1 stays on the link while this one is staged
      // (round 3 synchronised the stream here, which also waited for chunk c-1: the two slots gave no double buffering)
      if (c >= 2 && (e = hipEventSynchronize(done[c & 1])) != hipSuccess) return e;
      memcpy(sl, host + off, len);
      if ((e = hipMemcpyAsync(devp + off, sl, len, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
      if ((e = hipEventRecord(done[c & 1], st)) != hipSuccess) return e;
    }
    return hipStreamSynchronize(st);
  }
  // The destination is fresh malloc memory: without help every 4 KB page of it costs a fault inside the memcpy below (and
  // the faults of the threads contend for the process's address-space lock: measured 11 GB/s for 1.8 GB over 8 threads).
  // Ask for huge pages once and populate every chunk in one call right before it is filled -- while the next chunk is on
  // the link.  Both are hints (errors ignored: older kernels).
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
  auto page_in = [](char* p, size_t len, int advice) {
    const uintptr_t a = ((uintptr_t)p + 4095) & ~uintptr_t(4095), b = ((uintptr_t)p + len) & ~uintptr_t(4095);
    if (b > a) (void)madvise((void*)a, b - a, advice);
  };
#ifdef MADV_HUGEPAGE
  page_in(host, bytes, MADV_HUGEPAGE);
#endif
  size_t pendOff = 0, pendLen = 0;
  int pendSlot = -1;
  for (size_t c = 0; c < n; ++c) {
    const size_t off = c * S, len = std::min(S, bytes - off);
    if ((e = hipMemcpyAsync(slots[c & 1], devp + off, len, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if (pendSlot >= 0) {                                                      // the previous chunk, already landed
      page_in(host + pendOff, pendLen, MADV_POPULATE_WRITE);
      memcpy(host + pendOff, slots[pendSlot], pendLen);
    } else {
      page_in(host, std::min(bytes, S), MADV_POPULATE_WRITE);         // nothing to move yet: prepare the first chunk
    }
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    pendOff = off; pendLen = len; pendSlot = (int)(c & 1);
  }
  if (pendSlot >= 0) { page_in(host + pendOff, pendLen, MADV_POPULATE_WRITE); memcpy(host + pendOff, slots[pendSlot], pendLen); }
  return hipSuccess;
}
}  // namespace

// several (host, device, bytes) pairs in one go: the bytes of all of them are dealt to the lanes in 4 MB chunks
static int copy_pageable(int dev, const CopyJob* jobs, int njobs, bool toDevice) {
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) total += jobs[i].bytes;
  if (!total) return SPGEMM_OK;
  if (total < (size_t(1) << 20)) {                       // small: not worth the threads
    for (int i = 0; i < njobs; ++i)
      if (jobs[i].bytes) HIPCHK(toDevice ? hipMemcpy(jobs[i].dev, jobs[i].host, jobs[i].bytes, hipMemcpyHostToDevice)
                                        : hipMemcpy(jobs[i].host, jobs[i].dev, jobs[i].bytes, hipMemcpyDeviceToHost));
    return SPGEMM_OK;
  }
  CopyLanes& L = lanes();
  std::lock_guard<std::mutex> lk(L.mu);
  {
    int cur = dev;                                       // the lanes' streams belong to `dev`: make them there
    (void)hipGetDevice(&cur);
    HIPCHK(hipSetDevice(dev));
    const int rc = L.ensure(dev);
    if (cur != dev) (void)hipSetDevice(cur);
    CHK(rc);
  }
  // cut every job into T slices (all lanes work on the same job at the same time: neighbouring pages, one job after the other)
  hipError_t errs[CopyLanes::T];
  std::vector<std::thread> th;
  for (int t = 0; t < CopyLanes::T; ++t) {
    errs[t] = hipSuccess;
    th.emplace_back([&, t] {
      for (int i = 0; i < njobs && errs[t] == hipSuccess; ++i) {
        const size_t b = jobs[i].bytes;
        const size_t per = ((b + CopyLanes::T - 1) / CopyLanes::T + 4095) & ~size_t(4095);
        const size_t lo = std::min(b, per * (size_t)t), hi = std::min(b, lo + per);
        char* const slots[2] = {L.slot[t][0], L.slot[t][1]};
        if (hi > lo) errs[t] = lane_copy(dev, L.st[t], slots, L.done[t], (char*)jobs[i].host + lo, (char*)jobs[i].dev + lo, hi - lo, toDevice);
      }
    });
  }
  for (auto& x : th) x.join();
  for (int t = 0; t < CopyLanes::T; ++t)
    if (errs[t] != hipSuccess) {
      for (hipStream_t st : L.st) (void)hipStreamSynchronize(st);   // rule A: the callers' blocks go back behind idle lanes
      return fail(SPGEMM_ERR_HIP, "pipelined %s copy failed: %s", toDevice ? "h2d" : "d2h", hipGetErrorString(errs[t]));
    }
  return SPGEMM_OK;
}

// a malloc()ed host array on its way to a caller who free()s it
struct FreeHost { void operator()(void* p) const { free(p); } };
template <class T> using HostArray = std::unique_ptr<T, FreeHost>;

// the device product hip_CSR_SpMM{,_f64} runs between the copies
template <class V>
using DeviceSpMM = int (*)(spgemm_handle*, const int*, const int*, const V*, int, const int*, const int*, const V*, int, int,
                           int, int, int**, int**, V**, int*);

template <class V>
static int csr_spmm_host(DeviceSpMM<V> device_spmm, const int* IA, const int* JA, const V* A, int nnzA, const int* IB,
                         const int* JB, const V* B, int nnzB, int** IC, int** JC, V** C, int* nnzC, int m, int k, int n) {
  if (!IC || !JC || !C || !nnzC) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *IC = nullptr; *JC = nullptr; *C = nullptr; *nnzC = 0;
  if (m < 0 || k < 0 || n < 0) return fail(SPGEMM_ERR_ARG, "negative dimension");
  CHK(check_common(IA, JA, A, nnzA, "A"));
  CHK(check_common(IB, JB, B, nnzB, "B"));
  CHK(validate_host_csr(IA, JA, m, k, nnzA, "A"));
  CHK(validate_host_csr(IB, JB, k, n, nnzB, "B"));
  spgemm_handle* h = nullptr;
  CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  DevCSRT<V> dA, dB, dC;                               // the operands' copies and the product: all of them go back on return
  const bool same = (IA == IB && JA == JB && A == B && nnzA == nnzB && m == k);  // C = A*A: upload once
  const auto t0 = std::chrono::steady_clock::now();
  auto ms_since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count(); };
  std::vector<CopyJob> up;
  auto stage = [&up](auto& buf, const auto* src, size_t n) {        // a block for n elements and its place in the one copy
    CHK(spgemm_hip_malloc((void**)&buf.p, sizeof(*src) * n));
    up.push_back(CopyJob{(void*)src, (void*)buf.p, sizeof(*src) * n});
    return SPGEMM_OK;
  };
  CHK(stage(dA.I, IA, (size_t)m + 1));
  CHK(stage(dA.J, JA, (size_t)nnzA));
  CHK(stage(dA.V, A, (size_t)nnzA));
  if (!same) {
    CHK(stage(dB.I, IB, (size_t)k + 1));
    CHK(stage(dB.J, JB, (size_t)nnzB));
    CHK(stage(dB.V, B, (size_t)nnzB));
  }
  const DevCSRT<V>& dBx = same ? dA : dB;
  CHK(copy_pageable(h->device, up.data(), (int)up.size(), true));
  h->host_api.ms_h2d = ms_since(t0);
  const auto t1 = std::chrono::steady_clock::now();
  int nz = 0;
  CHK(device_spmm(h, dA.I, dA.J, dA.V, nnzA, dBx.I, dBx.J, dBx.V, nnzB, m, k, n, &dC.I.p, &dC.J.p, &dC.V.p, &nz));
  h->host_api.ms_device = ms_since(t1);
  const auto t2 = std::chrono::steady_clock::now();
  // outputs must be malloc()ed: the caller's CSR::dispose() is free() (nlibs/CSR.h:323-327)
  HostArray<int> hIC((int*)malloc(sizeof(int) * ((size_t)m + 1))), hJC((int*)malloc(sizeof(int) * (size_t)std::max(nz, 1)));
  HostArray<V> hC((V*)malloc(sizeof(V) * (size_t)std::max(nz, 1)));
  if (!hIC || !hJC || !hC) return fail(SPGEMM_ERR_NOMEM, "host malloc of C failed");
  const CopyJob down[3] = {{hIC.get(), dC.I, sizeof(int) * ((size_t)m + 1)}, {hJC.get(), dC.J, sizeof(int) * (size_t)nz},
                           {hC.get(), dC.V, sizeof(V) * (size_t)nz}};
  CHK(copy_pageable(h->device, down, 3, false));
  h->host_api.ms_d2h = ms_since(t2);
  h->host_api.ms_total = ms_since(t0);
  h->host_api.bytes_h2d = 0;
  for (auto& j : up) h->host_api.bytes_h2d += (long long)j.bytes;
  h->host_api.bytes_d2h = (long long)(down[0].bytes + down[1].bytes + down[2].bytes);
  *IC = hIC.release(); *JC = hJC.release(); *C = hC.release(); *nnzC = nz;
  return SPGEMM_OK;
}

extern "C" int hip_CSR_SpMM(const int* IA, const int* JA, const float* A, int nnzA, const int* IB, const int* JB,
                            const float* B, int nnzB, int** IC, int** JC, float** C, int* nnzC, int m, int k, int n) {
  return csr_spmm_host<float>(hip_gpuSpMM, IA, JA, A, nnzA, IB, JB, B, nnzB, IC, JC, C, nnzC, m, k, n);
}

extern "C" int hip_CSR_SpMM_f64(const int* IA, const int* JA, const double* A, int nnzA, const int* IB, const int* JB,
                                const double* B, int nnzB, int** IC, int** JC, double** C, int* nnzC, int m, int k, int n) {
  return csr_spmm_host<double>(hip_gpuSpMM_f64, IA, JA, A, nnzA, IB, JB, B, nnzB, IC, JC, C, nnzC, m, k, n);
}

// phases of the latest hip_CSR_SpMM (host arrays in, host arrays out) on the default handle
extern "C" int spgemm_hip_host_api_stats(spgemm_host_api_stats* out) {
  if (!out) return fail(SPGEMM_ERR_ARG, "null argument");
  spgemm_handle* h = nullptr;
  CHK(default_handle(&h));
  *out = h->host_api;
  return SPGEMM_OK;
}

// ------------------------------------------------------------------------------------------------
// R-MCL
// ------------------------------------------------------------------------------------------------
// Lanes per row of the row-wise kernels (k_rmcl_stats / _compact / _move): 16 for short rows; a whole wave once rows
// average ~100 entries.  nnz = 0 asks for the 16-lane form.
struct RowLanes { bool wide; int grid; };
static RowLanes row_lanes(const spgemm_handle* h, int m, long long nnz) {
  const bool wide = m > 0 && nnz >= 96ll * m;
  return {wide, wide ? clampi(cdiv(m, 4), 1, h->numCU * 32) : clampi(cdiv(m, 16), 1, h->numCU * 16)};
}
// kern<16 or 64, V>; V is the value type of the arrays among the arguments
#define RMCL_ROWS(kern, V, rl, stream, ...)                                                              \
  do {                                                                                                   \
    if ((rl).wide) hipLaunchKernelGGL((kern<64, V>), dim3((rl).grid), dim3(256), 0, stream, __VA_ARGS__);  \
    else hipLaunchKernelGGL((kern<16, V>), dim3((rl).grid), dim3(256), 0, stream, __VA_ARGS__);            \
  } while (0)

// nnzIn >= 0: the caller knows nnz(C) (it is on the host after every SpGEMM of this library) and the choice of lanes per
// row needs no device read; nnzIn < 0: one 4-byte copy fetches it.
template <class V>
static int rmcl_prune_impl(spgemm_handle* h, int m, long long nnzIn, const int* dIC, const int* dJC, const V* dC, DevCSRT<V>* out) {
  out->reset();
  if (m < 0 || !dIC) return fail(SPGEMM_ERR_ARG, "bad argument");
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  h->sym_m = -1;                                   // scan scratch and the small device block are shared with a pending phase
  clear_stale_hip_error();
  CHK(ws_ensure(h, m));
  DevCSRT<V> N;
  DevBuf<V> th, ks;
  auto hipfail = [&](const char* what) {
    return fail(SPGEMM_ERR_HIP, "rmcl prune%s: %s: %s", std::is_same<V, double>::value ? " (f64)" : "", what, hipGetErrorString(hipGetLastError()));
  };
  if (N.I.alloc((size_t)m + 1) || th.alloc((size_t)std::max(m, 1)) || ks.alloc((size_t)std::max(m, 1))) return hipfail("device allocation failed");
  hipStream_t s = h->stream;
  if (hipMemsetAsync(&h->dsmall->nnzC64, 0, sizeof(unsigned long long), s) != hipSuccess) return hipfail("memset");
  if (m > 0 && nnzIn < 0) {
    int tmp = 0;
    if (hipMemcpyAsync(&tmp, dIC + m, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return hipfail("reading nnz");
    nnzIn = tmp;
  }
  const RowLanes rl = row_lanes(h, m, nnzIn);
  if (m > 0) {
    RMCL_ROWS(k_rmcl_stats, V, rl, s, m, dIC, dC, N.I.p, th.p, ks.p);
    if (int rc = launch_scan(h, N.I, m, &h->dsmall->nnzC64)) return drained(s, rc);
  } else {
    hipMemsetAsync(N.I, 0, sizeof(int), s);
  }
  if (hipMemcpyAsync(&h->hsmall->nnzC64, &h->dsmall->nnzC64, sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return drained(s, hipfail("kept-entry count"));
  N.nnz = (int)h->hsmall->nnzC64;
  if (N.alloc_entries(N.nnz)) return hipfail("device allocation failed");
  if (m > 0 && N.nnz > 0) {
    RMCL_ROWS(k_rmcl_compact, V, rl, s, m, dIC, dJC, dC, N.I.p, th.p, ks.p, N.J.p, N.V.p);
    if (hipGetLastError() != hipSuccess) return drained(s, hipfail("compaction launch"));
  }
  if (hipStreamSynchronize(s) != hipSuccess) return drained(s, hipfail("compaction"));
  *out = std::move(N);
  return SPGEMM_OK;
}

// ---- the argument checks of the R-MCL entry points, one of each for both precisions ----
// the four output pointers, set to "nothing" until the call succeeds
template <class V>
static int clear_outputs(int** oI, int** oJ, V** oV, int* onnz) {
  if (!oI || !oJ || !oV || !onnz) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *oI = nullptr; *oJ = nullptr; *oV = nullptr; *onnz = 0;
  return SPGEMM_OK;
}
// the fused step's: outputs, dimensions, both operands
template <class V>
static int rmcl_step_args(const int* dIA, const int* dJA, const V* dA, int nnzA, const int* dIB, const int* dJB, const V* dB,
                          int nnzB, int m, int k, int n, int** dIN, int** dJN, V** dCN, int* nnzN) {
  CHK(clear_outputs(dIN, dJN, dCN, nnzN));
  if (m < 0 || k < 0 || n < 0) return fail(SPGEMM_ERR_ARG, "negative dimension m=%d k=%d n=%d", m, k, n);
  CHK(check_common(dIA, dJA, dA, nnzA, "A"));
  return check_common(dIB, dJB, dB, nnzB, "B");
}
// the loop's: outputs, a square matrix, both operands
template <class V>
static int rmcl_loop_args(int maxIter, int rows, int cols, const int* gI, const int* gJ, const V* gA, int gnnz, const int* tI,
                          const int* tJ, const V* tA, int tnnz, int** oI, int** oJ, V** oA, int* onnz) {
  CHK(clear_outputs(oI, oJ, oA, onnz));
  if (rows < 0 || cols != rows || maxIter < 0) return fail(SPGEMM_ERR_ARG, "R-MCL needs a square matrix and maxIter >= 0");
  CHK(check_common(gI, gJ, gA, gnnz, "Mgt"));
  return check_common(tI, tJ, tA, tnnz, "Mt");
}

template <class V>
static int rmcl_prune_abi(spgemm_handle* h, int m, long long nnz, const int* dIC, const int* dJC, const V* dC, int** dIN,
                          int** dJN, V** dCN, int* nnzN) {
  CHK(clear_outputs(dIN, dJN, dCN, nnzN));
  DevCSRT<V> N;
  CHK(rmcl_prune_impl(h, m, nnz, dIC, dJC, dC, &N));
  N.give(dIN, dJN, dCN, nnzN);
  return SPGEMM_OK;
}

extern "C" int hip_rmcl_prune(spgemm_handle* h, int m, const int* dIC, const int* dJC, float* dC, int** dIN, int** dJN,
                              float** dCN, int* nnzN) {
  return rmcl_prune_abi<float>(h, m, -1, dIC, dJC, dC, dIN, dJN, dCN, nnzN);
}
extern "C" int hip_rmcl_prune_n(spgemm_handle* h, int m, int nnz, const int* dIC, const int* dJC, const float* dC,
                                int** dIN, int** dJN, float** dCN, int* nnzN) {
  return nnz < 0 ? fail(SPGEMM_ERR_ARG, "negative nnz") : rmcl_prune_abi<float>(h, m, nnz, dIC, dJC, dC, dIN, dJN, dCN, nnzN);
}
extern "C" int hip_rmcl_prune_f64(spgemm_handle* h, int m, const int* dIC, const int* dJC, const double* dC, int** dIN,
                                  int** dJN, double** dCN, int* nnzN) {
  return rmcl_prune_abi<double>(h, m, -1, dIC, dJC, dC, dIN, dJN, dCN, nnzN);
}
extern "C" int hip_rmcl_prune_n_f64(spgemm_handle* h, int m, int nnz, const int* dIC, const int* dJC, const double* dC,
                                    int** dIN, int** dJN, double** dCN, int* nnzN) {
  return nnz < 0 ? fail(SPGEMM_ERR_ARG, "negative nnz") : rmcl_prune_abi<double>(h, m, nnz, dIC, dJC, dC, dIN, dJN, dCN, nnzN);
}

// Expansion and prune of one R-MCL iteration as ONE operator: C = A*B is never materialised.  Every numeric kernel
// applies the row rule to the finished row while it still sits in LDS and writes only the kept, normalised entries
// (about a quarter of the product) to the front of the row's range of a scratch C; k_rmcl_move packs them.
// What the reference's loop does in three steps (gpu SpGEMM, inflate+threshold kernels of dutil.cuh, thrust::remove;
// gpu_csr_kernel.cu:218-270) and hip_gpuSpMM + hip_rmcl_prune do in two.
// The m rows of an unpacked R, packed into a CSR of their own: the scan of the lengths is the row pointer, k_rmcl_move
// copies the rows.
static int rmcl_pack_rows(spgemm_handle* h, int m, const CsrView& R, DevCSR* out) {
  out->reset();
  hipStream_t s = h->stream;
  DevCSR N;
  if (N.I.alloc((size_t)m + 1)) return fail(SPGEMM_ERR_NOMEM, "device allocation failed");
  if (hipMemsetAsync(N.I, 0, sizeof(int) * ((size_t)m + 1), s) != hipSuccess ||
      hipMemcpyAsync(N.I, R.len, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return fail(SPGEMM_ERR_HIP, "pack: copy of the row lengths");
  CHK(launch_scan(h, N.I, m, &h->dsmall->kept64));
  if (hipMemcpyAsync(&h->hsmall->kept64, &h->dsmall->kept64, sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(SPGEMM_ERR_HIP, "pack: scan of the row lengths");
  const unsigned long long total = h->hsmall->kept64;
  if (total > 0x7fffffffULL) return fail(SPGEMM_ERR_OVERFLOW, "pack: %llu entries", total);
  N.nnz = (int)total;
  if (N.alloc_entries(N.nnz)) return fail(SPGEMM_ERR_NOMEM, "device allocation failed");
  if (N.nnz > 0 && m > 0) {
    const RowLanes rl = row_lanes(h, m, 0);          // always the 16-lane form
    RMCL_ROWS(k_rmcl_move, float, rl, s, m, R.I, N.I.p, R.J, R.V, N.J.p, N.V.p);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail(SPGEMM_ERR_HIP, "pack: move");
  }
  *out = std::move(N);
  return SPGEMM_OK;
}

// ---- one fused R-MCL step (rmcl_expand_prune_core) and its phases ----
// The form the step leaves its result in (DevCSR): extents for the next iteration of the loop, packed for a caller,
// block for the sharded loop.  The give-up route returns a packed result whatever was asked for.
enum { RMCL_EXTENTS = 0, RMCL_PACK = 1, RMCL_BLOCK = 2 };

static int rmcl_hipfail(const char* what) { return fail(SPGEMM_ERR_HIP, "rmcl expand+prune: %s: %s", what, hipGetErrorString(hipGetLastError())); }

// Products beyond which the scratch C is not made and the step runs as SpGEMM + prune.  SPGEMM_RMCL_MAXP lowers the bound
// (test hook: the give-up path, in the float loop behind an unpacked Mt, on small inputs).
static unsigned long long rmcl_max_products() {
  unsigned long long maxP = 1ull << 30;
  if (const char* e = getenv("SPGEMM_RMCL_MAXP")) maxP = std::min<unsigned long long>(maxP, strtoull(e, nullptr, 10));
  return maxP;
}

// Give-up route (no rows, no products, or a product too large for the scratch C): SpGEMM + prune, an unpacked B packed first.
static int rmcl_two_steps(spgemm_handle* h, const CsrView& A, CsrView B, int m, int k, int n, DevCSR* out) {
  DevCSR Bp, C;
  if (B.len) { CHK(rmcl_pack_rows(h, k, B, &Bp)); B = Bp.view(); }
  CHK(spgemm_device(h, {A.I, A.J, A.V, A.nnz, B.I, B.J, B.V, m, k, n}, B.nnz, nullptr, {&C.I.p, &C.J.p, &C.V.p, &C.nnz}));
  return rmcl_prune_impl<float>(h, m, C.nnz, C.I, C.J, C.V, out);
}

// Classification of the rows by their products into `mid`; C gets its row-start and kept-count arrays (m + 1 each).
static int rmcl_classify(spgemm_handle* h, const CsrView& A, const CsrView& B, int m, DevCSR* C, HostMirror* mid, bool* errPending) {
  if (C->I.alloc((size_t)m + 1) || C->len.alloc((size_t)m + 1)) return rmcl_hipfail("device allocation failed");
  hipStream_t s = h->stream;
  h->sym_m = -1;
  hipEventRecord(h->ev[0], s);
  h->cur_rowIds = h->rowIds;
  CHK(launch_classify(h, A.I, A.J, B.I, m, A.nnz, C->I, B.se));
  hipEventRecord(h->ev[1], s);
  if (hipMemcpyAsync(h->hmid, h->dsmall, sizeof(HostMirror), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipEventRecord(h->evMid, s) != hipSuccess)
    return rmcl_hipfail("classification copy");
  if (hipMemsetAsync(C->len, 0, sizeof(int) * ((size_t)m + 1), s) != hipSuccess) return rmcl_hipfail("memset");
  if (hipEventSynchronize(h->evMid) != hipSuccess) return rmcl_hipfail("classification");
  if (errPending && *errPending) {                   // the previous iteration of the loop returned without waiting for its
    *errPending = false;                             // numeric kernels: their flags reached the host before this event
    if (h->hsmall->err) return fail(SPGEMM_ERR_INTERNAL, "device invariant broken in the previous iteration (flags=%d)", h->hsmall->err);
  }
  *mid = *h->hmid;
  return SPGEMM_OK;
}

// Row sizing WITHOUT the symbolic pass, for every row of at most 4096 products (all rows of an R-MCL iteration on a
// sparse graph without hubs).  The pass's only product is the exact size of every row of C, and C is not kept: the
// scratch rows are laid out by the rows' product counts (known from the classification), every such row is hashed in a
// table sized by its products and the epilogue counts the distinct columns itself.  Rows of bin 8 pass through LDS in
// pieces and need their exact counts: only they get a symbolic kernel (k_sym_big overwrites their entries of dIC).
static int rmcl_size_rows_by_products(spgemm_handle* h, const CsrView& A, const CsrView& B, int m, int n, const HostMirror& mid, int* dIC) {
  hipStream_t s = h->stream;
  if (hipMemcpyAsync(dIC, h->rowFlops, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, s) != hipSuccess) return rmcl_hipfail("copy");
  const int nbig = mid.binPtr[NBINS] - mid.binPtr[NBINS - 1];
  if (nbig > 0) {
    KTimer t(h, SPGEMM_K_SYM_BIG, s);
    h->bdLogged = false;
    h->mdLogged = false;
    hipLaunchKernelGGL(k_sym_big<false>, dim3(clampi(nbig, 1, h->numCU)), dim3(BIG_THREADS), sizeof(BigSymShared), s,
                       h->dsmall->binPtr, 8, h->cur_rowIds, A.I, h->sbl, B.J, n, dIC, h->bigBitmaps, h->bm_cap(),
                       h->dsmall->qctr + 0 * 32, (int2*)nullptr, 0, (int*)nullptr, 0, 0, (int*)nullptr, (int*)nullptr);
    if (hipGetLastError() != hipSuccess) return rmcl_hipfail("symbolic launch");
  }
  return SPGEMM_OK;
}

// Scan of the row sizes, the scratch arrays (one slot per product) and the numeric kernels with the row rule in their
// epilogues (pmode 2: rows laid out by products); scanKept: the kept counts are scanned behind them.
static int rmcl_numeric(spgemm_handle* h, const CsrView& A, const CsrView& B, int m, int n, const HostMirror& mid, bool nosym,
                        bool scanKept, DevCSR* C) {
  hipStream_t s = h->stream;
  hipEventRecord(h->ev[2], s);
  CHK(launch_scan(h, C->I, m, &h->dsmall->nnzC64));
  hipEventRecord(h->ev[3], s);
  if (C->alloc_entries((long long)mid.totalP)) return rmcl_hipfail("device allocation of the scratch product failed");
  hipEventRecord(h->ev[4], s);
  h->mirror = mid;
  CHK(launch_numeric(h, A.I, A.V, B.J, B.V, n, h->cur_rowIds, mid.binPtr, C->I, C->J, C->V, C->len, nosym ? 2 : 1));
  hipEventRecord(h->ev[5], s);
  return scanKept ? launch_scan(h, C->len, m, &h->dsmall->kept64) : SPGEMM_OK;
}

// Finish 1: the rows stay where the epilogues wrote them, as {start, end} pairs for the next classification (queued behind this).
static int rmcl_leave_extents(spgemm_handle* h, int m, const HostMirror& mid, DevCSR* C) {
  if (C->se.alloc((size_t)m)) return rmcl_hipfail("device allocation failed");
  hipLaunchKernelGGL(k_zip_extents, dim3(cdiv(m, 256)), dim3(256), 0, h->stream, m, C->I.p, C->len.p, C->se.p);
  if (hipGetLastError() != hipSuccess) return rmcl_hipfail("extent launch");
  C->nnz = (int)mid.totalP;
  return SPGEMM_OK;
}

// Finish 3 (finish 2, the block form, is the scratch C as it stands): the kept entries move into packed arrays, the
// scanned counts become the row pointer and the scratch C goes back to the pool.
template <class V>
static int rmcl_pack_result(spgemm_handle* h, int m, int nz, DevCSRT<V>* C) {
  DevCSRT<V> N;
  if (N.alloc_entries(nz)) return rmcl_hipfail("device allocation failed");
  if (nz > 0) {
    const RowLanes rl = row_lanes(h, m, nz);
    RMCL_ROWS(k_rmcl_move, V, rl, h->stream, m, C->I.p, C->len.p, C->J.p, C->V.p, N.J.p, N.V.p);
    if (hipGetLastError() != hipSuccess) return drained(h->stream, rmcl_hipfail("move launch"));   // N goes before the caller drains
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) return drained(h->stream, rmcl_hipfail("move"));
  N.I = std::move(C->len);
  N.nnz = nz;
  *C = std::move(N);
  return SPGEMM_OK;
}

// One R-MCL iteration (expansion with the row rule fused into the numeric epilogues): *out = prune(A * B) in the form
// `mode` names.  errPending != nullptr: the loop form, whose extents exit does not wait (below).
static int rmcl_expand_prune_core(spgemm_handle* h, const CsrView& A, const CsrView& B, int m, int k, int n, int mode,
                                  DevCSR* out, bool* errPending = nullptr) {
  out->reset();
  if (h->failNext > 0) { --h->failNext; return fail(SPGEMM_ERR_INTERNAL, "forced failure (spgemm_hip_debug_fail_next)"); }
  HIPCHK(hipSetDevice(h->device));
  if (m == 0) return rmcl_two_steps(h, A, B, m, k, n, out);
  CHK(ws_ensure(h, m));
  hipStream_t s = h->stream;
  DevCSR C;                                          // the scratch product: row starts, kept counts, one slot per product
  HostMirror mid;
  int rc = rmcl_classify(h, A, B, m, &C, &mid, errPending);
  if (rc) return drained(s, rc);
  if (mid.totalP == 0 || mid.totalP > rmcl_max_products()) {   // (the scratch C takes 8 bytes per product)
    if (hipStreamSynchronize(s) != hipSuccess) return drained(s, rmcl_hipfail("classification"));
    C.reset();
    return rmcl_two_steps(h, A, B, m, k, n, out);
  }
  const bool nosym = !getenv("SPGEMM_RMCL_SYMBOLIC");
  rc = nosym ? rmcl_size_rows_by_products(h, A, B, m, n, mid, C.I) : launch_symbolic(h, A.I, B.J, m, n, h->cur_rowIds, C.I);
  if (!rc) rc = rmcl_numeric(h, A, B, m, n, mid, nosym, mode != RMCL_EXTENTS, &C);
  if (rc) return drained(s, rc);
  if (mode == RMCL_EXTENTS && errPending && h->ktiming == 0) {
    // Loop form: nothing of this iteration is needed on the host before the next one starts -- its classification is
    // queued behind the numeric kernels, and the error flags are looked at after that classification's event.
    // The host runs ahead and the GPU does not idle between iterations.  (With per-kernel timing on, the events have to
    // be read now: the call waits as before.)
    if (hipMemcpyAsync(h->hsmall, h->dsmall, sizeof(HostMirror), hipMemcpyDeviceToHost, s) != hipSuccess)
      return drained(s, rmcl_hipfail("numeric phase"));   // (read_mirror's copy without its wait)
    if ((rc = rmcl_leave_extents(h, m, mid, &C))) return drained(s, rc);
    publish_stats(h, mid, StatsForm::CountsOnly);
    *errPending = true;
    *out = std::move(C);
    return SPGEMM_OK;
  }
  if ((rc = read_mirror(h, "rmcl expand+prune"))) return drained(s, rc);
  publish_stats(h, h->mirror, nosym ? StatsForm::OneShotNoNnz : StatsForm::OneShot);
  grow_bitmaps(h, n);
  const int kept = (int)h->mirror.kept64;            // <= nnz(C) <= P <= 2^30
  if (mode == RMCL_BLOCK) C.nnz = kept;              // scratch rows + the row pointer of the packed block
  else if ((rc = mode == RMCL_PACK ? rmcl_pack_result(h, m, kept, &C) : rmcl_leave_extents(h, m, mid, &C))) return drained(s, rc);
  *out = std::move(C);
  return SPGEMM_OK;
}

extern "C" int hip_rmcl_expand_prune(spgemm_handle* h, const int* dIA, const int* dJA, const float* dA, int nnzA,
                                     const int* dIB, const int* dJB, const float* dB, int nnzB, int m, int k, int n,
                                     int** dIN, int** dJN, float** dCN, int* nnzN) {
  CHK(rmcl_step_args(dIA, dJA, dA, nnzA, dIB, dJB, dB, nnzB, m, k, n, dIN, dJN, dCN, nnzN));
  if (!h) CHK(default_handle(&h));
  DevCSR N;
  CHK(rmcl_expand_prune_core(h, {dIA, dJA, dA, nnzA}, {dIB, dJB, dB, nnzB}, m, k, n, RMCL_PACK, &N));
  N.give(dIN, dJN, dCN, nnzN);
  return SPGEMM_OK;
}

// maxIter == 0: the loop's result is a copy of Mt
template <class V>
static int rmcl_copy_of_mt(hipStream_t s, int rows, const int* dtI, const int* dtJ, const V* dtA, int tnnz, DevCSRT<V>* out) {
  DevCSRT<V> N;
  if (N.I.alloc((size_t)rows + 1) || N.alloc_entries(tnnz)) return fail(SPGEMM_ERR_NOMEM, "device allocation failed");
  if (hipMemcpyAsync(N.I, dtI, sizeof(int) * ((size_t)rows + 1), hipMemcpyDeviceToDevice, s) != hipSuccess ||
      (tnnz > 0 && (hipMemcpyAsync(N.J, dtJ, sizeof(int) * (size_t)tnnz, hipMemcpyDeviceToDevice, s) != hipSuccess ||
                    hipMemcpyAsync(N.V, dtA, sizeof(V) * (size_t)tnnz, hipMemcpyDeviceToDevice, s) != hipSuccess)) ||
      hipStreamSynchronize(s) != hipSuccess)
    return drained(s, fail(SPGEMM_ERR_HIP, "copy of Mt"));
  N.nnz = tnnz;
  *out = std::move(N);
  return SPGEMM_OK;
}

// The R-MCL loop on device arrays (gpuRmclIter, gpus/gpu_csr_kernel.cu:15-40, without its two copies): maxIter iterations
// Mt <- prune(Mgt * Mt) from (tI, tJ, tA), which are left alone; the result is a packed device CSR of the library's
// pool.  Between iterations Mt is NOT packed: every epilogue leaves its kept entries at the front of the row's scratch
// range and the next classification reads {start, kept} per row (k_row_flops' IBlen), so that only the last iteration
// pays for the scan of the counts, the packed arrays and the copy into them.
extern "C" int hip_gpuRmclIter_device(spgemm_handle* h, int maxIter, int rows, int cols, const int* dgI, const int* dgJ,
                                      const float* dgA, int gnnz, const int* dtI, const int* dtJ, const float* dtA,
                                      int tnnz, int** oI, int** oJ, float** oA, int* onnz) {
  CHK(rmcl_loop_args(maxIter, rows, cols, dgI, dgJ, dgA, gnnz, dtI, dtJ, dtA, tnnz, oI, oJ, oA, onnz));
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  const bool keep_packed = getenv("SPGEMM_RMCL_PACK") != nullptr;       // A/B switch: pack after every iteration
  hipStream_t s = h->stream;
  DevCSR cur;                                        // the current Mt once the loop owns one; until then the caller's
  Retired old;                                       // rule B: the Mt the latest step read
  bool errPending = false;
  for (int it = 0; it < maxIter; ++it) {
    DevCSR next;
    const bool pack = keep_packed || it == maxIter - 1;
    const CsrView Mt = it ? cur.view() : CsrView{dtI, dtJ, dtA, tnnz};
    if (int rc = rmcl_expand_prune_core(h, {dgI, dgJ, dgA, gnnz}, Mt, rows, cols, cols, pack ? RMCL_PACK : RMCL_EXTENTS, &next, &errPending))
      return drained(s, rc);
    old.park(std::move(cur));                        // that call waited behind the readers of the Mt parked before
    cur = std::move(next);
  }                                                  // (the last iteration packs and waits for everything)
  if (maxIter == 0) {
    CHK(rmcl_copy_of_mt(s, rows, dtI, dtJ, dtA, tnnz, &cur));
  } else if (!cur.packed()) {                        // the last iteration gave up on the fused step?  it returns packed: not reached
    return drained(s, fail(SPGEMM_ERR_INTERNAL, "the last iteration returned an unpacked matrix"));
  }
  cur.give(oI, oJ, oA, onnz);
  return SPGEMM_OK;
}

// ---- hip_gpuRmclIter[_f64] on one device: host arrays in, the device loop on the default handle, malloc()ed arrays out ----
// Host CSR -> pool blocks on the current device; arrays without entries get their (never empty) blocks and no copy.
template <class V>
static int csr_to_device(const int* I, const int* J, const V* A, int rows, int nnz, DevCSRT<V>* M) {
  auto up = [](auto& buf, const auto* src, size_t n) {
    const int rc = spgemm_hip_malloc((void**)&buf.p, sizeof(*src) * std::max<size_t>(n, 1));
    return rc || n == 0 ? rc : spgemm_hip_memcpy_h2d(buf.p, src, sizeof(*src) * n);
  };
  M->nnz = nnz;
  int rc;
  if ((rc = up(M->I, I, (size_t)rows + 1)) || (rc = up(M->J, J, (size_t)nnz)) || (rc = up(M->V, A, (size_t)nnz))) return rc;
  return SPGEMM_OK;
}
// A packed device CSR -> malloc()ed host arrays (never of size zero); the caller free()s them.
template <class V>
static int csr_to_host(const DevCSRT<V>& N, int rows, int** oI, int** oJ, V** oA, int* onnz) {
  int* hI = (int*)malloc(sizeof(int) * ((size_t)rows + 1));
  int* hJ = (int*)malloc(sizeof(int) * (size_t)std::max(N.nnz, 1));
  V* hA = (V*)malloc(sizeof(V) * (size_t)std::max(N.nnz, 1));
  int rc = SPGEMM_OK;
  if (!hI || !hJ || !hA) rc = fail(SPGEMM_ERR_NOMEM, "host malloc failed");
  else if ((rc = spgemm_hip_memcpy_d2h(hI, N.I, sizeof(int) * ((size_t)rows + 1))) == SPGEMM_OK && N.nnz > 0 &&
           (rc = spgemm_hip_memcpy_d2h(hJ, N.J, sizeof(int) * (size_t)N.nnz)) == SPGEMM_OK)
    rc = spgemm_hip_memcpy_d2h(hA, N.V, sizeof(V) * (size_t)N.nnz);
  if (rc) { free(hI); free(hJ); free(hA); return rc; }
  *oI = hI; *oJ = hJ; *oA = hA; *onnz = N.nnz;
  return SPGEMM_OK;
}
// loop: hip_gpuRmclIter_device or its _f64 twin
template <class V, class Loop>
static int rmcl_iter_host(Loop loop, int maxIter, int rows, const int* gIA, const int* gJA, const V* gA, int gnnz, const int* tIA,
                          const int* tJA, const V* tA, int tnnz, int** oIA, int** oJA, V** oA, int* onnz) {
  spgemm_handle* h = nullptr;
  CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  DevCSRT<V> Mg, Mt, N;
  CHK(csr_to_device(gIA, gJA, gA, rows, gnnz, &Mg));
  CHK(csr_to_device(tIA, tJA, tA, rows, tnnz, &Mt));
  CHK(loop(h, maxIter, rows, rows, Mg.I, Mg.J, Mg.V, gnnz, Mt.I, Mt.J, Mt.V, tnnz, &N.I.p, &N.J.p, &N.V.p, &N.nnz));
  Mt.reset();
  return csr_to_host(N, rows, oIA, oJA, oA, onnz);
}

struct spgemm_group;
static std::mutex g_rmcl_group_mu;                    // the group hip_gpuRmclIter keeps between calls (same device layout)
static spgemm_group* g_rmcl_group = nullptr;
static std::vector<int> g_rmcl_group_devs;
static int g_rmcl_devices_used = 1;
// devices the latest hip_gpuRmclIter of this process computed on (1 unless SPGEMM_RMCL_DEVICES asked for more)
extern "C" int spgemm_hip_rmcl_devices_used(void) { return g_rmcl_devices_used; }
extern "C" int spgemm_hip_group_create(spgemm_group** out, int nshards, const int* devices, int transport);
extern "C" int spgemm_hip_group_destroy(spgemm_group* g);
extern "C" int hip_gpuRmclIter_sharded(spgemm_group* g, int maxIter, int rows, int cols, const int* gIA, const int* gJA,
                                       const float* gA, int gnnz, const int* tIA, const int* tJA, const float* tA, int tnnz,
                                       int** oIA, int** oJA, float** oA, int* onnz);

extern "C" int hip_gpuRmclIter(int maxIter, int rows, int cols, const int* gIA, const int* gJA, const float* gA, int gnnz,
                               const int* tIA, const int* tJA, const float* tA, int tnnz, int** oIA, int** oJA,
                               float** oA, int* onnz) {
  CHK(rmcl_loop_args(maxIter, rows, cols, gIA, gJA, gA, gnnz, tIA, tJA, tA, tnnz, oIA, oJA, oA, onnz));
  CHK(validate_host_csr(gIA, gJA, rows, cols, gnnz, "Mgt"));
  CHK(validate_host_csr(tIA, tJA, rows, cols, tnnz, "Mt"));
  {
    // Several devices, when the caller asks for them: Mgt's rows are cut into flops-balanced blocks, one per GPU, Mt is
    // replicated and the pruned blocks are gathered every iteration (sharded.hpp) -- behind the same call the reference's
    // driver makes (nlibs/qrmcl.cc:149-152).  OPT-IN (round 3 sharded over every visible device by default: a 100-row graph
    // was cut over 8 GPUs, and a process-per-GPU job would have opened contexts and communicators on all of them from every
    // rank): SPGEMM_RMCL_DEVICES=N|all uses N devices (0..N-1); SPGEMM_RMCL_SHARDS=K asks for K LOGICAL shards spread
    // round-robin over those devices (the one-GPU rehearsal of the sharded loop).  Unset: one device, the default handle's.
    // The group is kept for the next call with the same layout (the C++ mirror's --stats mode calls this once per iteration:
    // handles, RCCL communicators and pinned buffers are made once).
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
    int use = 1;
    if (const char* e = getenv("SPGEMM_RMCL_DEVICES")) use = !strcasecmp(e, "all") ? ndev : std::max(1, std::min(ndev, atoi(e)));
    int shards = use;
    if (const char* e = getenv("SPGEMM_RMCL_SHARDS")) shards = std::max(1, std::min(64, atoi(e)));
    g_rmcl_devices_used = 1;
    if (shards > 1 && rows >= shards) {
      std::vector<int> devs((size_t)shards);
      for (int i = 0; i < shards; ++i) devs[(size_t)i] = i % std::max(use, 1);
      std::lock_guard<std::mutex> lk(g_rmcl_group_mu);
      int rc = SPGEMM_OK;
      if (!g_rmcl_group || g_rmcl_group_devs != devs) {
        if (g_rmcl_group) { spgemm_hip_group_destroy(g_rmcl_group); g_rmcl_group = nullptr; }
        rc = spgemm_hip_group_create(&g_rmcl_group, shards, devs.data(), SPGEMM_XCHG_AUTO);
        if (rc == SPGEMM_OK) g_rmcl_group_devs = devs;
        else g_rmcl_group = nullptr;
      }
      if (rc == SPGEMM_OK)
        rc = hip_gpuRmclIter_sharded(g_rmcl_group, maxIter, rows, cols, gIA, gJA, gA, gnnz, tIA, tJA, tA, tnnz, oIA, oJA, oA, onnz);
      if (rc == SPGEMM_OK) { g_rmcl_devices_used = std::min(use, shards); return rc; }
      // the caller asked for an R-MCL result, not for a particular number of GPUs: say what went wrong and carry on with one
      fprintf(stderr, "hip_gpuRmclIter: the %d-shard loop failed (%s); running on one device\n", shards, spgemm_hip_last_error());
    }
  }
  return rmcl_iter_host<float>(hip_gpuRmclIter_device, maxIter, rows, gIA, gJA, gA, gnnz, tIA, tJA, tA, tnnz, oIA, oJA, oA, onnz);
}

// ------------------------------------------------------------------------------------------------
// R-MCL with double values: fused step and loop on one device (the prune, the entry points' checks and the host copies
// are the templates above).  The float path's structure with two differences: the symbolic pass always runs (the f64
// tables are sized from the exact L_i), so the scratch C has nnz(C) entries, not one per product; and every step leaves
// a packed matrix (the unpacked {start, kept} layout of the float loop is not carried over).
// ------------------------------------------------------------------------------------------------
using DevCSR64 = DevCSRT<double>;

// Give-up route (no rows, no products, or a product beyond the cap): hip_gpuSpMM_f64 + prune.
static int rmcl_two_steps64(spgemm_handle* h, const Product<double>& p, int nnzB, DevCSR64* out) {
  DevCSR64 C;
  CHK(hip_gpuSpMM_f64(h, p.IA, p.JA, p.A, p.nnzA, p.IB, p.JB, p.B, nnzB, p.m, p.k, p.n, &C.I.p, &C.J.p, &C.V.p, &C.nnz));
  return rmcl_prune_impl<double>(h, p.m, C.nnz, C.I, C.J, C.V, out);
}

// One R-MCL iteration in double, *out = prune(A * B), packed: shared classification, symbolic pass and scan (the int32
// refusal and the error word are hip_gpuSpMM_f64's), a scratch C of nnz(C) entries, the f64 numeric launches with the row
// rule in their epilogues (+ k_rmcl_fix_rows<double> for the rows that do not finish in one LDS table), the scan of the kept
// counts and rmcl_pack_result.  Arguments are checked by the callers.
static int rmcl_expand_prune64_core(spgemm_handle* h, const Product<double>& p, int nnzB, DevCSR64* out) {
  out->reset();
  HIPCHK(hipSetDevice(h->device));
  if (p.m == 0) return rmcl_two_steps64(h, p, nnzB, out);
  CHK(ws_ensure(h, p.m));
  hipStream_t s = h->stream;
  const int m = p.m;
  DevCSR64 C;                                          // the scratch product: row starts of the full rows, nnz(C) slots;
  if (C.I.alloc((size_t)m + 1) || C.len.alloc((size_t)m + 1)) return rmcl_hipfail("device allocation failed");   // len: kept per row
  int nnzC = 0;
  int rc = symbolic_phase(h, p.IA, p.JA, p.nnzA, p.IB, p.JB, m, p.k, p.n, nullptr, C.I, &nnzC, false);
  h->sym_m = -1;                                       // the phase is finished here, not by hip_spgemm_numeric_f64
  if (rc) return drained(s, rc);
  const unsigned long long P = h->mirror.totalP;
  if (P == 0 || P > rmcl_max_products()) {             // the float step's cap and its test hook
    C.reset();                                         // (symbolic_phase waited for the stream)
    return rmcl_two_steps64(h, p, nnzB, out);
  }
  if (hipMemsetAsync(C.len, 0, sizeof(int) * ((size_t)m + 1), s) != hipSuccess) return drained(s, rmcl_hipfail("memset"));
  if (C.alloc_entries(nnzC)) return drained(s, rmcl_hipfail("device allocation of the scratch product failed"));
  {
    F64Scratch scratch;
    hipEventRecord(h->ev[4], s);
    if (nnzC > 0 && (rc = launch_numeric_f64(h, p.IA, p.A, p.JB, p.B, h->cur_rowIds, h->mirror.binPtr, C.I, C.J, C.V, &scratch, C.len)))
      return drained(s, rc);
    hipEventRecord(h->ev[5], s);
    if ((rc = launch_scan(h, C.len, m, &h->dsmall->kept64))) return drained(s, rc);
    if ((rc = read_mirror(h, "rmcl expand+prune (f64)"))) return drained(s, rc);
  }                                                    // (read_mirror waited for the stream: the scratch goes back)
  spgemm_stats& st = h->stats;
  hipEventElapsedTime(&st.ms_numeric, h->ev[4], h->ev[5]);
  st.ms_total += st.ms_numeric;
  collect_kernel_times(h, false);
  CHK(rmcl_pack_result(h, m, (int)h->mirror.kept64, &C));   // kept <= nnz(C) < 2^31; the scanned counts become the row pointer
  *out = std::move(C);
  return SPGEMM_OK;
}

extern "C" int hip_rmcl_expand_prune_f64(spgemm_handle* h, const int* dIA, const int* dJA, const double* dA, int nnzA,
                                         const int* dIB, const int* dJB, const double* dB, int nnzB, int m, int k, int n,
                                         int** dIN, int** dJN, double** dCN, int* nnzN) {
  CHK(rmcl_step_args(dIA, dJA, dA, nnzA, dIB, dJB, dB, nnzB, m, k, n, dIN, dJN, dCN, nnzN));
  if (!h) CHK(default_handle(&h));
  DevCSR64 N;
  CHK(rmcl_expand_prune64_core(h, {dIA, dJA, dA, nnzA, dIB, dJB, dB, m, k, n}, nnzB, &N));
  N.give(dIN, dJN, dCN, nnzN);
  return SPGEMM_OK;
}

// gpuRmclIter on device arrays with QValue double: maxIter iterations Mt <- prune(Mgt * Mt) from (tI, tJ, tA), which are
// left alone; the result is a packed device CSR of the pool.  Mt is packed after every iteration.
extern "C" int hip_gpuRmclIter_device_f64(spgemm_handle* h, int maxIter, int rows, int cols, const int* dgI, const int* dgJ,
                                          const double* dgA, int gnnz, const int* dtI, const int* dtJ, const double* dtA,
                                          int tnnz, int** oI, int** oJ, double** oA, int* onnz) {
  CHK(rmcl_loop_args(maxIter, rows, cols, dgI, dgJ, dgA, gnnz, dtI, dtJ, dtA, tnnz, oI, oJ, oA, onnz));
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  DevCSR64 cur;                                        // the current Mt once the loop owns one; until then the caller's
  for (int it = 0; it < maxIter; ++it) {
    DevCSR64 next;
    const Product<double> p{dgI, dgJ, dgA, gnnz, it ? cur.I.p : dtI, it ? cur.J.p : dtJ, it ? cur.V.p : dtA, rows, cols, cols};
    if (int rc = rmcl_expand_prune64_core(h, p, it ? cur.nnz : tnnz, &next)) return drained(s, rc);
    cur = std::move(next);                             // (every step waits for its kernels: the old Mt is idle)
  }
  if (maxIter == 0) CHK(rmcl_copy_of_mt(s, rows, dtI, dtJ, dtA, tnnz, &cur));
  cur.give(oI, oJ, oA, onnz);
  return SPGEMM_OK;
}

// host arrays in, malloc()ed host arrays out; one device (the default handle's), whatever SPGEMM_RMCL_DEVICES says
extern "C" int hip_gpuRmclIter_f64(int maxIter, int rows, int cols, const int* gIA, const int* gJA, const double* gA, int gnnz,
                                   const int* tIA, const int* tJA, const double* tA, int tnnz, int** oIA, int** oJA,
                                   double** oA, int* onnz) {
  CHK(rmcl_loop_args(maxIter, rows, cols, gIA, gJA, gA, gnnz, tIA, tJA, tA, tnnz, oIA, oJA, oA, onnz));
  CHK(validate_host_csr(gIA, gJA, rows, cols, gnnz, "Mgt"));
  CHK(validate_host_csr(tIA, tJA, rows, cols, tnnz, "Mt"));
  return rmcl_iter_host<double>(hip_gpuRmclIter_device_f64, maxIter, rows, gIA, gJA, gA, gnnz, tIA, tJA, tA, tnnz, oIA, oJA, oA, onnz);
}

// ------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------
template <class V>
static int sort_rows(spgemm_handle* h, int m, const int* dIC, int* dJC, V* dC) {
  if (m < 0 || !dIC) return fail(SPGEMM_ERR_ARG, "bad argument");
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  if (m == 0) return SPGEMM_OK;
  clear_stale_hip_error();
  hipStream_t s = h->stream;
  DevBuf<int> dcnt, JS;
  DevBuf<V> CS;
  auto hipfail = [&](const char* what) { return fail(SPGEMM_ERR_HIP, "sort rows: %s: %s", what, hipGetErrorString(hipGetLastError())); };
  if (dcnt.alloc(1) != hipSuccess) return hipfail("allocation");
  if (hipMemsetAsync(dcnt, 0, sizeof(int), s) != hipSuccess) return hipfail("memset");
  hipLaunchKernelGGL(k_sort_rows<V>, dim3(clampi(m, 1, h->numCU * 8)), dim3(256), 0, s, m, dIC, dJC, dC, dcnt.p);
  int info[2] = {0, 0};                                // unsorted rows longer than SORT_MAX, nnz
  if (hipMemcpyAsync(&info[0], dcnt, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(&info[1], dIC + m, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return hipfail("short rows");
  if (info[0] > 0 && info[1] > 0) {
    // the long rows sort between their segment of (JC, C) and the same segment of a scratch copy
    if (JS.alloc((size_t)info[1]) != hipSuccess || CS.alloc((size_t)info[1]) != hipSuccess) return hipfail("scratch allocation");
    // column bits: the columns of a valid CSR are < 2^31; take the width from the largest possible key
    const int keyBits = 31;
    hipLaunchKernelGGL(k_sort_long_rows<V>, dim3(clampi(info[0], 1, h->numCU * 4)), dim3(256), 0, s, m, dIC, dJC, dC, JS.p, CS.p, keyBits);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return hipfail("long rows");
  }
  return SPGEMM_OK;
}

extern "C" int hip_csr_sort_rows(spgemm_handle* h, int m, const int* dIC, int* dJC, float* dC) {
  return sort_rows<float>(h, m, dIC, dJC, dC);
}

extern "C" int hip_csr_sort_rows_f64(spgemm_handle* h, int m, const int* dIC, int* dJC, double* dC) {
  return sort_rows<double>(h, m, dIC, dJC, dC);
}

extern "C" int spgemm_hip_selftest(spgemm_handle* h) {
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  const int nb = 64;
  std::vector<int> host(nb * WAVE);
  unsigned x = 12345u;
  for (auto& v : host) { x = x * 1664525u + 1013904223u; v = (int)((x >> 8) & 0xfffff); }
  DevBlock<int> din, dbad;
  HIPCHK(din.reserve(host.size()));
  HIPCHK(dbad.reserve(1));
  HIPCHK(hipMemcpy(din, host.data(), sizeof(int) * host.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dbad, 0, sizeof(int)));
  clear_stale_hip_error();
  hipLaunchKernelGGL(k_selftest, dim3(nb), dim3(WAVE), 0, h->stream, din.p, dbad.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  int bad = -1;
  HIPCHK(hipMemcpy(&bad, dbad, sizeof(int), hipMemcpyDeviceToHost));
  if (bad != 0) return fail(SPGEMM_ERR_INTERNAL, "wave primitive self-test: %d lanes disagree", bad);
  return SPGEMM_OK;
}


// ------------------------------------------------------------------------------------------------
// what the six device CSR format headers below share: prologue, Scratch, validation, scan, radix sort, tile copy
// ------------------------------------------------------------------------------------------------
#include "csr_common_device.hpp"

// ------------------------------------------------------------------------------------------------
// COO -> CSR on the device (the step in front of the path)
// ------------------------------------------------------------------------------------------------
#include "coo_device.hpp"

// ------------------------------------------------------------------------------------------------
// reordering a device CSR: row / column permutations, transpose
// ------------------------------------------------------------------------------------------------
#include "reorder_device.hpp"

// ------------------------------------------------------------------------------------------------
// comparing two device CSRs: diff report, differs, differsStats
// ------------------------------------------------------------------------------------------------
#include "compare_device.hpp"

// ------------------------------------------------------------------------------------------------
// column-partitioned CSR: split into column blocks, blockwise product, join
// ------------------------------------------------------------------------------------------------
#include "pcsr_device.hpp"

// ------------------------------------------------------------------------------------------------
// blocked CSR (BCSR): CSR -> r x c dense tiles and back
// ------------------------------------------------------------------------------------------------
#include "bcsr_device.hpp"

// ------------------------------------------------------------------------------------------------
// mixed CSR (MCSR): a tiled top-left corner plus a CSR remainder, and back
// ------------------------------------------------------------------------------------------------
#include "mcsr_device.hpp"

// ------------------------------------------------------------------------------------------------
// edge-list text -> COO triplets: the parse in front of hip_coo_to_csr
// ------------------------------------------------------------------------------------------------
#include "edges_device.hpp"

// ------------------------------------------------------------------------------------------------
// device CSR -> edge-list text: the way out, the inverse of the parse
// ------------------------------------------------------------------------------------------------
#include "edges_write_device.hpp"

// ------------------------------------------------------------------------------------------------
// dense matrix: CSR -> dense, dense -> CSR, the dense product
// ------------------------------------------------------------------------------------------------
#include "dense_device.hpp"

// ------------------------------------------------------------------------------------------------
// clusters from a finished R-MCL result: attractors, connected components, labels -> clusters
// ------------------------------------------------------------------------------------------------
#include "clusters_device.hpp"

// ------------------------------------------------------------------------------------------------
// sparse add, diagonal scaling, degree factors and the symmetrisations of a directed graph
// ------------------------------------------------------------------------------------------------
#include "symmetrize_device.hpp"

// ------------------------------------------------------------------------------------------------
// selection: the k largest entries of every row, and the R-MCL loop with that row cap
// ------------------------------------------------------------------------------------------------
#include "topk_device.hpp"

#undef CSR_ALLOC                                   // csr_common_device.hpp's pair, used by the twelve headers above
#undef CSR_HIP

// ------------------------------------------------------------------------------------------------
// multi-GPU: groups of shards, sharded SpGEMM, sharded R-MCL
// ------------------------------------------------------------------------------------------------
#include "sharded.hpp"

#ifdef SMF_STAMPS
// diagnostic build only: the phase cycles k_num_bighash has accumulated since the last call (and reset)
extern "C" int spgemm_hip_debug_stamps(unsigned long long* out16) {
  unsigned long long z[16] = {0};
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamps), sizeof(z)) != hipSuccess) return fail(SPGEMM_ERR_HIP, "stamps");
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z)) != hipSuccess) return fail(SPGEMM_ERR_HIP, "stamps reset");
  return SPGEMM_OK;
}
extern "C" int spgemm_hip_debug_chain_stamps(unsigned long long* out16) {
  unsigned long long z[16] = {0};
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_cstamps), sizeof(z)) != hipSuccess) return fail(SPGEMM_ERR_HIP, "stamps");
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_cstamps), z, sizeof(z)) != hipSuccess) return fail(SPGEMM_ERR_HIP, "stamps reset");
  return SPGEMM_OK;
}
#endif
