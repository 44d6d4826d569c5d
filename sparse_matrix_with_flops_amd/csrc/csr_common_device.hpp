// What the device CSR format headers share (coo, reorder, compare, pcsr, bcsr, mcsr, edges): the call prologue and the per-call
// Scratch, the validation of a CSR with its single flag read-back, the library's scan with its 64-bit total, the stable
// LSD radix sort, the entry-dealing helpers (row search, tile rows, lower bound) and the staged tile copy.
// Included in spgemm_hip.hip ahead of those headers (uses its pool / error helpers and the k_scan_* kernels).
#pragma once

namespace csrdev {

constexpr int CP_THREADS = 256, CP_ITEMS = 4, CP_TILE = CP_THREADS * CP_ITEMS;              // entry-dealing kernels
constexpr int RS_THREADS = 256, RS_ITEMS = 8, RS_TILE = RS_THREADS * RS_ITEMS, RS_RADIX = 256;  // radix passes
enum { BAD_ROWPTR = 1, BAD_ROWSRC = 2, BAD_COLMAP = 4, BAD_COLUMN = 8, BAD_PERM = 16 };

// pass 1 of a digit: how many keys of every digit value each block holds; blockHist is digit-major [256][nblk]
__global__ __launch_bounds__(RS_THREADS) void k_radix_hist(int n, const unsigned long long* __restrict__ keys, int shift,
                                                           int nblk, int* __restrict__ blockHist) {
  __shared__ int hist[RS_RADIX];
  const int tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * RS_TILE;
#pragma unroll
  for (int i = 0; i < RS_ITEMS; ++i) {
    const long long idx = base + i * RS_THREADS + tid;
    if (idx < n) atomicAdd(&hist[(int)((keys[idx] >> shift) & 255ull)], 1);
  }
  __syncthreads();
  blockHist[(size_t)tid * nblk + blockIdx.x] = hist[tid];
}

// pass 2: stable scatter.  blockOff = exclusive scan of blockHist (digit-major, block-minor): where the block's keys
// of each digit start.  Inside the block the order is (round, wave, lane) = index order: per round every wave ranks its
// lanes among the lanes with the same digit (8 ballots), one thread per digit turns the per-wave counts into offsets.
__global__ __launch_bounds__(RS_THREADS) void k_radix_scatter(int n, const unsigned long long* __restrict__ keysIn,
                                                              const int* __restrict__ idxIn,
                                                              unsigned long long* __restrict__ keysOut, int* __restrict__ idxOut,
                                                              int shift, int nblk, const int* __restrict__ blockOff) {
  constexpr int NWV = RS_THREADS / smf::WAVE;
  __shared__ int wcnt[NWV][RS_RADIX];
  __shared__ int woff[NWV][RS_RADIX];
  __shared__ int run[RS_RADIX];
  const int tid = threadIdx.x, w = tid >> 6;
  run[tid] = blockOff[(size_t)tid * nblk + blockIdx.x];
  const long long base = (long long)blockIdx.x * RS_TILE;
  for (int i = 0; i < RS_ITEMS; ++i) {
#pragma unroll
    for (int q = 0; q < NWV; ++q) wcnt[q][tid] = 0;
    __syncthreads();
    const long long idx = base + i * RS_THREADS + tid;
    const bool valid = idx < n;
    unsigned long long key = 0ull;
    int payload = 0;
    if (valid) { key = keysIn[idx]; payload = idxIn[idx]; }
    const int d = (int)((key >> shift) & 255ull);
    unsigned long long peers = smf::ballot64(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long mb = smf::ballot64(valid && ((d >> b) & 1));
      peers &= ((d >> b) & 1) ? mb : ~mb;
    }
    const int rank = smf::mask_rank(peers);
    if (valid && rank == 0) wcnt[w][d] = __popcll(peers);
    __syncthreads();
    {
      int r = run[tid];
#pragma unroll
      for (int q = 0; q < NWV; ++q) { woff[q][tid] = r; r += wcnt[q][tid]; }
      run[tid] = r;
    }
    __syncthreads();
    if (valid) {
      const int dst = woff[w][d] + rank;
      keysOut[dst] = key;
      idxOut[dst] = payload;
    }
  }
}

// rowPtr[0] = 0, monotone, rowPtr[m] = nnz (nnz < 0: the end is not checked); lens / maxLen optional
__global__ void k_check_rowptr(int m, int nnz, const int* __restrict__ IA, int* __restrict__ lens, int* __restrict__ maxLen,
                               int* __restrict__ bad) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const int a = IA[r], b = IA[r + 1];
  const bool wrong = a < 0 || b < a || (nnz >= 0 && b > nnz) || (r == 0 && a != 0) || (nnz >= 0 && r == m - 1 && b != nnz);
  if (wrong) { atomicOr(bad, BAD_ROWPTR); return; }
  if (lens) lens[r] = b - a;
  if (maxLen) atomicMax(maxLen, b - a);
}

__global__ void k_check_cols(int nnz, int n, const int* __restrict__ JA, int* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nnz && (unsigned)JA[i] >= (unsigned)n) atomicOr(bad, BAD_COLUMN);
}

// first index in [lo, hi) of the ascending array whose element is not below want (hi if there is none)
template <class T>
__device__ __forceinline__ int first_at_least(const T* __restrict__ sorted, int lo, int hi, T want) {
  while (lo < hi) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if (sorted[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the row in [lo, hi] that holds entry o: rowPtr[r] <= o < rowPtr[r+1] (empty rows are skipped); o < rowPtr[hi+1]
__device__ __forceinline__ int row_of_entry(const int* __restrict__ rowPtr, int lo, int hi, int o) {
  while (lo < hi) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if (rowPtr[mid + 1] > o) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// rows of the first and the last entry of a block's tile [base, base + CP_TILE): every search of the block stays inside
__device__ __forceinline__ void tile_rows(const int* __restrict__ rowPtr, int m, int nnz, long long base, int (&rows)[2]) {
  if (threadIdx.x == 0) {
    const long long last = base + CP_TILE - 1 < nnz ? base + CP_TILE - 1 : nnz - 1;
    rows[0] = row_of_entry(rowPtr, 0, m - 1, (int)base);
    rows[1] = row_of_entry(rowPtr, rows[0], m - 1, (int)last);
  }
  __syncthreads();
}

template <class V>
__device__ __forceinline__ void store4(V* __restrict__ dst, const V (&v)[4]) {
  if constexpr (sizeof(V) == 4) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *reinterpret_cast<double2*>(dst) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2*>(dst + 2) = make_double2(v[2], v[3]);
  }
}

// Write side of a staged tile (sc / sv: the block's CP_TILE columns / values in LDS, entry base + t at index t): after the
// barrier every lane takes 4 consecutive entries back out of LDS and stores them with one 16-byte (index) and one
// 16/32-byte (value) store; the tile that holds the end of the array finishes entry by entry.
template <class V>
__device__ __forceinline__ void tile_store(long long base, int nnz, const int (&sc)[CP_TILE], const V (&sv)[CP_TILE],
                                           int* __restrict__ JC, V* __restrict__ C) {
  __syncthreads();
  const int t0 = threadIdx.x * CP_ITEMS;
  const long long o0 = base + t0;
  if (o0 >= nnz) return;
  if (o0 + CP_ITEMS <= nnz) {
    *reinterpret_cast<int4*>(JC + o0) = *reinterpret_cast<const int4*>(sc + t0);
    const V v[CP_ITEMS] = {sv[t0], sv[t0 + 1], sv[t0 + 2], sv[t0 + 3]};
    store4<V>(C + o0, v);
  } else {
    for (int k = 0; o0 + k < nnz; ++k) { JC[o0 + k] = sc[t0 + k]; C[o0 + k] = sv[t0 + k]; }
  }
}

// The body of the copy kernels that deal OUTPUT entries: one tile of the output's entries per block (CP_THREADS lanes).
// Read side, lane-strided (entry base + k * 256 + lane: consecutive lanes read consecutive entries of a row, so a wave's
// load is contiguous inside a source row): the row by a search in the output rowPtr IC bounded by the tile's rows, then
// src(row, offset in the row, column&, value&) says where that entry comes from; staged in LDS for tile_store.
template <class V, class Src>
__device__ __forceinline__ void tile_copy(int m, int nnz, const int* __restrict__ IC, int* __restrict__ JC, V* __restrict__ C,
                                          const Src& src) {
  __shared__ int rows[2];
  __shared__ __attribute__((aligned(16))) int sc[CP_TILE];
  __shared__ __attribute__((aligned(16))) V sv[CP_TILE];
  const long long base = (long long)blockIdx.x * CP_TILE;
  tile_rows(IC, m, nnz, base, rows);
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const int t = k * CP_THREADS + threadIdx.x;
    const long long o = base + t;
    if (o < nnz) {
      const int r = row_of_entry(IC, rows[0], rows[1], (int)o);
      src(r, (int)o - IC[r], sc[t], sv[t]);
    }
  }
  tile_store<V>(base, nnz, sc, sv, JC, C);
}

static inline int bits_of(int maxval) { return maxval > 0 ? 32 - __builtin_clz((unsigned)maxval) : 0; }
static inline dim3 grid256(long long n) { return dim3((unsigned)std::max<long long>(1, (n + 255) / 256)); }

// scratch of the scans below: tile[0] = total, tile + 1 = per-tile sums, for arrays of up to `longest` ints
static inline size_t scan_scratch_bytes(long long longest) {
  return sizeof(unsigned long long) * (size_t)((longest + SCAN_TILE - 1) / SCAN_TILE + 2);
}

// in-place exclusive scan of data[0..cnt), data[cnt] = total (the k_scan_* kernels of the SpGEMM path)
static inline void scan_inplace(hipStream_t s, int* data, int cnt, unsigned long long* tile) {
  scan_launches(s, data, cnt, tile + 1, tile, true);
}

// scan_inplace, then its 64-bit total on the host (one blocking read-back); what counts as an overflow is the caller's
static inline hipError_t scan_total(hipStream_t s, int* data, int cnt, unsigned long long* tile, unsigned long long* total) {
  scan_inplace(s, data, cnt, tile);
  const hipError_t e = hipMemcpyAsync(total, tile, sizeof(*total), hipMemcpyDeviceToHost, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}

// stable LSD passes over key bits [lo, hi), 8 per pass; the sorted arrays end up in (keyA, idxA) (the pointers are
// swapped after every pass).  bhist: int[nblk * 256 + 1].
static inline void radix_sort_bits(hipStream_t s, int total, int lo, int hi, unsigned long long*& keyA,
                                   unsigned long long*& keyB, int*& idxA, int*& idxB, int* bhist,
                                   unsigned long long* tile) {
  const int nblk = cdiv(total, RS_TILE);
  for (int shift = lo; shift < hi; shift += 8) {
    hipLaunchKernelGGL(k_radix_hist, dim3(nblk), dim3(RS_THREADS), 0, s, total, keyA, shift, nblk, bhist);
    scan_inplace(s, bhist, nblk * RS_RADIX, tile);
    hipLaunchKernelGGL(k_radix_scatter, dim3(nblk), dim3(RS_THREADS), 0, s, total, keyA, idxA, keyB, idxB, shift, nblk, bhist);
    std::swap(keyA, keyB);
    std::swap(idxA, idxB);
  }
}

// temporaries of one call: everything goes back to the pool when the call ends, outputs only on failure
struct Scratch {
  std::vector<void*> tmp, out;
  template <class T> bool get(T** p, size_t bytes, bool output = false) {
    void* q = nullptr;
    if (pool().alloc(&q, std::max<size_t>(bytes, 1)) != hipSuccess) return false;
    (output ? out : tmp).push_back(q);
    *p = (T*)q;
    return true;
  }
  int done(int rc) {
    for (void* p : tmp) pool().release(p);
    if (rc != SPGEMM_OK) for (void* p : out) pool().release(p);
    tmp.clear(); out.clear();
    return rc;
  }
};

// for functions with a `Scratch sc`; #undef'd in spgemm_hip.hip behind the last header that uses them
#define CSR_ALLOC(...) if (!sc.get(__VA_ARGS__)) return sc.done(fail(SPGEMM_ERR_HIP, "device allocation failed"))
#define CSR_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return sc.done(fail(SPGEMM_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_))); } while (0)

// the call prologue behind the argument checks: the default handle if none was given, its device, its stream
static int enter(spgemm_handle*& h, hipStream_t* s) {
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  clear_stale_hip_error();
  *s = h->stream;
  return SPGEMM_OK;
}

// the host-side checks of an m x n CSR argument with nnz entries
template <class V>
static int check_csr_args(int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA) {
  if (m < 0 || n < 0 || nnz < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if ((m > 0 && !dIA) || (nnz > 0 && (!dJA || !dA))) return fail(SPGEMM_ERR_ARG, "CSR arrays null with m=%d nnz=%d", m, nnz);
  if (m == 0 && nnz > 0) return fail(SPGEMM_ERR_ARG, "nnz=%d in a matrix without rows", nnz);
  return SPGEMM_OK;
}

// Device validation, ONE blocking read-back per call: flag_begin makes the zeroed flag, any number of checks are queued
// on it (queue_csr_checks and whatever else the caller needs), read_flag brings the BAD_* bits back.  Nothing that forms
// an address from a checked value is queued before the read.  The caller maps the bits to its own messages.
static int flag_begin(Scratch& sc, hipStream_t s, int** bad) {
  if (!sc.get(bad, sizeof(int))) return fail(SPGEMM_ERR_HIP, "device allocation failed");
  const hipError_t e = hipMemsetAsync(*bad, 0, sizeof(int), s);
  if (e != hipSuccess) return fail(SPGEMM_ERR_HIP, "hipMemsetAsync(bad, 0, sizeof(int), s) failed: %s", hipGetErrorString(e));
  return SPGEMM_OK;
}

// rowPtr against nnz for m > 0; with dJA given, the nnz > 0 columns against [0, n)
static void queue_csr_checks(hipStream_t s, int m, int n, int nnz, const int* dIA, const int* dJA, int* bad) {
  if (m > 0) hipLaunchKernelGGL(k_check_rowptr, grid256(m), dim3(256), 0, s, m, nnz, dIA, (int*)nullptr, (int*)nullptr, bad);
  if (dJA && nnz > 0) hipLaunchKernelGGL(k_check_cols, grid256(nnz), dim3(256), 0, s, nnz, n, dJA, bad);
}

static int read_flag(hipStream_t s, const int* dflag, int* hflag) {
  if (hipMemcpyAsync(hflag, dflag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(SPGEMM_ERR_HIP, "reading the validation flag failed: %s", hipGetErrorString(hipGetLastError()));
  return SPGEMM_OK;
}

// the three in one go, for the callers with nothing else to check
static int validate_csr(Scratch& sc, hipStream_t s, int m, int n, int nnz, const int* dIA, const int* dJA, int* hbad) {
  int* bad = nullptr;
  CHK(flag_begin(sc, s, &bad));
  queue_csr_checks(s, m, n, nnz, dIA, dJA, bad);
  return read_flag(s, bad, hbad);
}

}  // namespace csrdev
