// Reordering a device CSR: row / column permutations, the permutation helpers and the transpose.
//
// Replaces, on device arrays,
//   CSR::PM / MP / PMPt / PtMP                nlibs/CSR.cc:431-482   (rows taken in a new order, columns renamed)
//   CSR::rowDescendingOrderPermutation        nlibs/CSR.cc:484-494   (key_value_qsort on the row lengths)
//   permutationTranspose                      nlibs/tools/util.cc:162-168
//   the transposed load readSNAPFile(isTrans) nlibs/COO.h:19         (here: any device CSR, not only at parse time)
//
// hip_csr_permute is one pass over the entries: row lengths gathered through rowSrc, the library's scan, one copy kernel
// that deals OUTPUT entries (1024 per block: lane-strided reads staged in LDS, 4 consecutive entries stored per lane) and
// finds their row by a search in the new rowPtr -- a 20 000-entry row next to empty ones is spread over 20 blocks like any other 20 000 entries.
// The two sorts are the stable LSD radix passes of coo_device.hpp over exactly the bits the shape needs:
//   transpose   key = (col << rowBits) | row, passes over the column bits only (a CSR is in row order already, so a stable
//               sort by column gives (column, row) order); payload = the value's bits (float) or the source index (double)
//   descending  key = maxLen - len, payload = row id (equal lengths keep ascending row id)
// Every value that becomes an address (rowSrc, colMap, a permutation to invert, columns renamed through colMap, rowPtr)
// is checked first by kernels that only read the input and write a flag / mark array of our own; the host reads the flag
// before anything is queued that indexes with those values.
// Included at the end of spgemm_hip.hip behind coo_device.hpp (uses its radix kernels, the pool / error helpers, k_scan_*).
#pragma once

namespace reorder {

constexpr int CP_THREADS = 256, CP_ITEMS = 4, CP_TILE = CP_THREADS * CP_ITEMS;
enum { BAD_ROWPTR = 1, BAD_ROWSRC = 2, BAD_COLMAP = 4, BAD_COLUMN = 8, BAD_PERM = 16 };

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

// P is a permutation of 0..len-1  <=>  every value is in range and none is seen twice (mark: zeroed int[len] of ours)
__global__ void k_check_perm(int len, const int* __restrict__ P, int* __restrict__ mark, int* __restrict__ bad, int bit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= len) return;
  const int v = P[i];
  if ((unsigned)v >= (unsigned)len) { atomicOr(bad, bit); return; }
  if (atomicExch(&mark[v], 1) != 0) atomicOr(bad, bit);
}

__global__ void k_check_cols(int nnz, int n, const int* __restrict__ JA, int* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nnz && (unsigned)JA[i] >= (unsigned)n) atomicOr(bad, BAD_COLUMN);
}

__global__ void k_invert_perm(int len, const int* __restrict__ P, int* __restrict__ Pt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < len) Pt[P[i]] = i;
}

__global__ void k_gather_lens(int m, const int* __restrict__ IA, const int* __restrict__ rowSrc, int* __restrict__ IB) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int r = rowSrc ? rowSrc[i] : i;
  IB[i] = IA[r + 1] - IA[r];
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

// One tile of B's entries per block.  Read side, lane-strided (entry base + k * 256 + lane: consecutive lanes read
// consecutive entries of a source row, so a wave's load is contiguous inside a row): row by a search in IB bounded by the
// tile's rows, source position through rowSrc, column through colMap, staged in LDS.  Write side: every lane takes 4
// consecutive entries back out of LDS and stores them with one 16-byte (index) and one 16/32-byte (value) store.
template <class V>
__global__ __launch_bounds__(CP_THREADS) void k_permute_copy(int m, int nnz, const int* __restrict__ IA,
                                                             const int* __restrict__ JA, const V* __restrict__ A,
                                                             const int* __restrict__ rowSrc, const int* __restrict__ colMap,
                                                             const int* __restrict__ IB, int* __restrict__ JB,
                                                             V* __restrict__ B) {
  __shared__ int rows[2];
  __shared__ __attribute__((aligned(16))) int sc[CP_TILE];
  __shared__ __attribute__((aligned(16))) V sv[CP_TILE];
  const long long base = (long long)blockIdx.x * CP_TILE;
  tile_rows(IB, m, nnz, base, rows);
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const int t = k * CP_THREADS + threadIdx.x;
    const long long o = base + t;
    if (o < nnz) {
      const int r = row_of_entry(IB, rows[0], rows[1], (int)o);
      const int p = IA[rowSrc ? rowSrc[r] : r] + ((int)o - IB[r]);
      const int cc = JA[p];
      sc[t] = colMap ? colMap[cc] : cc;
      sv[t] = A[p];
    }
  }
  __syncthreads();
  const int t0 = threadIdx.x * CP_ITEMS;
  const long long o0 = base + t0;
  if (o0 >= nnz) return;
  if (o0 + CP_ITEMS <= nnz) {
    *reinterpret_cast<int4*>(JB + o0) = *reinterpret_cast<const int4*>(sc + t0);
    const V v[CP_ITEMS] = {sv[t0], sv[t0 + 1], sv[t0 + 2], sv[t0 + 3]};
    store4<V>(B + o0, v);
  } else {
    for (int k = 0; o0 + k < nnz; ++k) { JB[o0 + k] = sc[t0 + k]; B[o0 + k] = sv[t0 + k]; }
  }
}

// transpose keys, dealt by entries (lane-strided inside the block's tile: every access coalesced): key = (col << rowBits)
// | row (rowPtr and the columns have been validated).  payload: value bits (4-byte values) or entry index.
template <class V>
__global__ __launch_bounds__(CP_THREADS) void k_transpose_keys(int m, int nnz, int rowBits, const int* __restrict__ IA,
                                                               const int* __restrict__ JA, const V* __restrict__ A,
                                                               unsigned long long* __restrict__ keys, int* __restrict__ payload) {
  __shared__ int rows[2];
  const long long base = (long long)blockIdx.x * CP_TILE;
  tile_rows(IA, m, nnz, base, rows);
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const long long o = base + k * CP_THREADS + threadIdx.x;
    if (o >= nnz) break;
    const int r = row_of_entry(IA, rows[0], rows[1], (int)o);
    const int c = JA[o];
    keys[o] = ((unsigned long long)(unsigned)c << rowBits) | (unsigned)r;
    if constexpr (sizeof(V) == 4) payload[o] = __float_as_int(A[o]); else payload[o] = (int)o;
  }
}

template <class V>
__global__ void k_transpose_emit(int nnz, int rowBits, const unsigned long long* __restrict__ keys,
                                 const int* __restrict__ payload, const V* __restrict__ A, int* __restrict__ JT,
                                 V* __restrict__ AT) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  JT[i] = (int)(keys[i] & ((1ull << rowBits) - 1ull));
  if constexpr (sizeof(V) == 4) AT[i] = __int_as_float(payload[i]); else AT[i] = A[payload[i]];
}

// IT[c] = first sorted key of column c or later (one search per output row, like coo::k_row_starts), c = 0..n
__global__ void k_col_starts(int n, int nnz, int rowBits, const unsigned long long* __restrict__ keys, int* __restrict__ IT) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > n) return;
  const unsigned long long want = (unsigned long long)(unsigned)c << rowBits;
  int lo = 0, hi = nnz;
  while (lo < hi) {
    const int mid = (int)(((long long)lo + hi) >> 1);
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  IT[c] = lo;
}

__global__ void k_desc_keys(int m, int maxLen, const int* __restrict__ lens, unsigned long long* __restrict__ keys,
                            int* __restrict__ ids) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  keys[r] = (unsigned long long)(unsigned)(maxLen - lens[r]);
  ids[r] = r;
}

__global__ void k_iota(int m, int* __restrict__ ids) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < m) ids[r] = r;
}

static inline int bits_of(int maxval) { return maxval > 0 ? 32 - __builtin_clz((unsigned)maxval) : 0; }
static inline dim3 grid256(long long n) { return dim3((unsigned)std::max<long long>(1, (n + 255) / 256)); }

// scratch of the scans below: tile[0] = total, tile + 1 = per-tile sums, for arrays of up to `longest` ints
static inline size_t scan_scratch_bytes(long long longest) {
  return sizeof(unsigned long long) * (size_t)((longest + SCAN_TILE - 1) / SCAN_TILE + 2);
}

// in-place exclusive scan of data[0..cnt), data[cnt] = total (the k_scan_* kernels of the SpGEMM path)
static inline void scan_inplace(hipStream_t s, int* data, int cnt, unsigned long long* tile) {
  const int ntiles = std::max(1, cdiv(cnt, SCAN_TILE));
  hipLaunchKernelGGL(k_scan_tile_sums, dim3(ntiles), dim3(SCAN_THREADS), 0, s, cnt, data, tile + 1);
  hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, s, ntiles, tile + 1, tile);
  hipLaunchKernelGGL(k_scan_apply, dim3(ntiles), dim3(SCAN_THREADS), 0, s, cnt, data, tile + 1, tile, 1);
}

// stable LSD passes over key bits [lo, hi) with the radix kernels of coo_device.hpp; the sorted arrays end up in
// (keyA, idxA) (the pointers are swapped after every pass).  bhist: int[nblk * 256 + 1].
static inline void radix_sort_bits(hipStream_t s, int total, int lo, int hi, unsigned long long*& keyA,
                                   unsigned long long*& keyB, int*& idxA, int*& idxB, int* bhist,
                                   unsigned long long* tile) {
  const int nblk = cdiv(total, coo::RS_TILE);
  for (int shift = lo; shift < hi; shift += 8) {
    hipLaunchKernelGGL(coo::k_radix_hist, dim3(nblk), dim3(coo::RS_THREADS), 0, s, total, keyA, shift, nblk, bhist);
    scan_inplace(s, bhist, nblk * coo::RS_RADIX, tile);
    hipLaunchKernelGGL(coo::k_radix_scatter, dim3(nblk), dim3(coo::RS_THREADS), 0, s, total, keyA, idxA, keyB, idxB, shift,
                       nblk, bhist);
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

#define RO_ALLOC(...) if (!sc.get(__VA_ARGS__)) return sc.done(fail(SPGEMM_ERR_HIP, "device allocation failed"))
#define RO_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return sc.done(fail(SPGEMM_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_))); } while (0)

static int read_flag(hipStream_t s, const int* dflag, int* hflag) {
  if (hipMemcpyAsync(hflag, dflag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fail(SPGEMM_ERR_HIP, "reading the validation flag failed: %s", hipGetErrorString(hipGetLastError()));
  return SPGEMM_OK;
}

template <class V>
static int permute(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, const int* dRowSrc,
                   const int* dColMap, int** dIB, int** dJB, V** dB) {
  if (!dIB || !dJB || !dB) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIB = nullptr; *dJB = nullptr; *dB = nullptr;
  if (m < 0 || n < 0 || nnz < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if ((m > 0 && !dIA) || (nnz > 0 && (!dJA || !dA))) return fail(SPGEMM_ERR_ARG, "CSR arrays null with m=%d nnz=%d", m, nnz);
  if (m == 0 && nnz > 0) return fail(SPGEMM_ERR_ARG, "nnz=%d in a matrix without rows", nnz);
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  clear_stale_hip_error();
  hipStream_t s = h->stream;
  Scratch sc;
  int *bad = nullptr, *mark = nullptr, *IB = nullptr, *JB = nullptr;
  V* B = nullptr;
  unsigned long long* tile = nullptr;
  // (1) validation: rowPtr, the two permutations, and the columns that will index colMap
  RO_ALLOC(&bad, sizeof(int));
  RO_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
  if (m > 0) hipLaunchKernelGGL(k_check_rowptr, grid256(m), dim3(256), 0, s, m, nnz, dIA, (int*)nullptr, (int*)nullptr, bad);
  const long long marks = (dRowSrc ? (long long)m : 0) + (dColMap ? (long long)n : 0);
  if (marks > 0) {
    RO_ALLOC(&mark, sizeof(int) * (size_t)marks);
    RO_HIP(hipMemsetAsync(mark, 0, sizeof(int) * (size_t)marks, s));
  }
  if (dRowSrc && m > 0) hipLaunchKernelGGL(k_check_perm, grid256(m), dim3(256), 0, s, m, dRowSrc, mark, bad, (int)BAD_ROWSRC);
  if (dColMap) {
    if (n > 0) hipLaunchKernelGGL(k_check_perm, grid256(n), dim3(256), 0, s, n, dColMap, mark + (dRowSrc ? m : 0), bad, (int)BAD_COLMAP);
    if (nnz > 0) hipLaunchKernelGGL(k_check_cols, grid256(nnz), dim3(256), 0, s, nnz, n, dJA, bad);
  }
  int hbad = 0;
  if (read_flag(s, bad, &hbad)) return sc.done(SPGEMM_ERR_HIP);
  if (hbad & BAD_ROWPTR) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer ending at nnz=%d", nnz));
  if (hbad & BAD_ROWSRC) return sc.done(fail(SPGEMM_ERR_INPUT, "rowSrc is not a permutation of 0..%d", m - 1));
  if (hbad & BAD_COLMAP) return sc.done(fail(SPGEMM_ERR_INPUT, "colMap is not a permutation of 0..%d", n - 1));
  if (hbad & BAD_COLUMN) return sc.done(fail(SPGEMM_ERR_INPUT, "column outside [0,%d)", n));
  // (2) new rowPtr: lengths through rowSrc, scanned
  RO_ALLOC(&IB, sizeof(int) * ((size_t)m + 1), true);
  RO_ALLOC(&JB, sizeof(int) * (size_t)std::max(nnz, 1), true);
  RO_ALLOC(&B, sizeof(V) * (size_t)std::max(nnz, 1), true);
  RO_ALLOC(&tile, scan_scratch_bytes((long long)m + 1));
  if (m > 0) hipLaunchKernelGGL(k_gather_lens, grid256(m), dim3(256), 0, s, m, dIA, dRowSrc, IB);
  scan_inplace(s, IB, m, tile);
  // (3) entries: gathered and renamed in one pass
  if (nnz > 0)
    hipLaunchKernelGGL(k_permute_copy<V>, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, dIA, dJA, dA,
                       dRowSrc, dColMap, IB, JB, B);
  RO_HIP(hipGetLastError());
  RO_HIP(hipStreamSynchronize(s));
  *dIB = IB; *dJB = JB; *dB = B;
  return sc.done(SPGEMM_OK);
}

template <class V>
static int transpose(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, int** dIT,
                     int** dJT, V** dAT) {
  if (!dIT || !dJT || !dAT) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIT = nullptr; *dJT = nullptr; *dAT = nullptr;
  if (m < 0 || n < 0 || nnz < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if ((m > 0 && !dIA) || (nnz > 0 && (!dJA || !dA))) return fail(SPGEMM_ERR_ARG, "CSR arrays null with m=%d nnz=%d", m, nnz);
  if (m == 0 && nnz > 0) return fail(SPGEMM_ERR_ARG, "nnz=%d in a matrix without rows", nnz);
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  clear_stale_hip_error();
  hipStream_t s = h->stream;
  Scratch sc;
  int *bad = nullptr, *IT = nullptr, *JT = nullptr, *idxA = nullptr, *idxB = nullptr, *bhist = nullptr;
  V* AT = nullptr;
  unsigned long long *keyA = nullptr, *keyB = nullptr, *tile = nullptr;
  RO_ALLOC(&bad, sizeof(int));
  RO_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
  // validation, one read-back: rowPtr (the key kernel searches it) and the column range
  if (m > 0) hipLaunchKernelGGL(k_check_rowptr, grid256(m), dim3(256), 0, s, m, nnz, dIA, (int*)nullptr, (int*)nullptr, bad);
  if (nnz > 0) hipLaunchKernelGGL(k_check_cols, grid256(nnz), dim3(256), 0, s, nnz, n, dJA, bad);
  int hbad = 0;
  if (read_flag(s, bad, &hbad)) return sc.done(SPGEMM_ERR_HIP);
  if (hbad & BAD_ROWPTR) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer ending at nnz=%d", nnz));
  if (hbad & BAD_COLUMN) return sc.done(fail(SPGEMM_ERR_INPUT, "column outside [0,%d)", n));
  RO_ALLOC(&IT, sizeof(int) * ((size_t)n + 1), true);
  RO_ALLOC(&JT, sizeof(int) * (size_t)std::max(nnz, 1), true);
  RO_ALLOC(&AT, sizeof(V) * (size_t)std::max(nnz, 1), true);
  if (nnz == 0) {
    RO_HIP(hipMemsetAsync(IT, 0, sizeof(int) * ((size_t)n + 1), s));
    RO_HIP(hipStreamSynchronize(s));
    *dIT = IT; *dJT = JT; *dAT = AT;
    return sc.done(SPGEMM_OK);
  }
  const int rowBits = std::max(1, bits_of(m - 1)), colBits = std::max(1, bits_of(n - 1));
  const int nblk = cdiv(nnz, coo::RS_TILE);
  RO_ALLOC(&keyA, sizeof(unsigned long long) * (size_t)nnz);
  RO_ALLOC(&keyB, sizeof(unsigned long long) * (size_t)nnz);
  RO_ALLOC(&idxA, sizeof(int) * (size_t)nnz);
  RO_ALLOC(&idxB, sizeof(int) * (size_t)nnz);
  RO_ALLOC(&bhist, sizeof(int) * ((size_t)nblk * coo::RS_RADIX + 1));
  RO_ALLOC(&tile, scan_scratch_bytes((long long)nblk * coo::RS_RADIX + 1));
  hipLaunchKernelGGL(k_transpose_keys<V>, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, rowBits, dIA,
                     dJA, dA, keyA, idxA);
  radix_sort_bits(s, nnz, rowBits, rowBits + colBits, keyA, keyB, idxA, idxB, bhist, tile);
  hipLaunchKernelGGL(k_transpose_emit<V>, grid256(nnz), dim3(256), 0, s, nnz, rowBits, keyA, idxA, dA, JT, AT);
  hipLaunchKernelGGL(k_col_starts, grid256((long long)n + 1), dim3(256), 0, s, n, nnz, rowBits, keyA, IT);
  RO_HIP(hipGetLastError());
  RO_HIP(hipStreamSynchronize(s));
  *dIT = IT; *dJT = JT; *dAT = AT;
  return sc.done(SPGEMM_OK);
}

}  // namespace reorder

extern "C" int hip_csr_permute(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                               const int* dRowSrc, const int* dColMap, int** dIB, int** dJB, float** dB) {
  return reorder::permute<float>(h, m, n, nnz, dIA, dJA, dA, dRowSrc, dColMap, dIB, dJB, dB);
}

extern "C" int hip_csr_permute_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                                   const int* dRowSrc, const int* dColMap, int** dIB, int** dJB, double** dB) {
  return reorder::permute<double>(h, m, n, nnz, dIA, dJA, dA, dRowSrc, dColMap, dIB, dJB, dB);
}

extern "C" int hip_csr_transpose(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                                 int** dIT, int** dJT, float** dAT) {
  return reorder::transpose<float>(h, m, n, nnz, dIA, dJA, dA, dIT, dJT, dAT);
}

extern "C" int hip_csr_transpose_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                                     int** dIT, int** dJT, double** dAT) {
  return reorder::transpose<double>(h, m, n, nnz, dIA, dJA, dA, dIT, dJT, dAT);
}

extern "C" int hip_permutation_transpose(spgemm_handle* h, int len, const int* dP, int* dPt) {
  using namespace reorder;
  if (len < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (len > 0 && (!dP || !dPt)) return fail(SPGEMM_ERR_ARG, "permutation arrays null with len=%d", len);
  if (len == 0) return SPGEMM_OK;
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  clear_stale_hip_error();
  hipStream_t s = h->stream;
  Scratch sc;
  int *bad = nullptr, *mark = nullptr;
  RO_ALLOC(&bad, sizeof(int));
  RO_ALLOC(&mark, sizeof(int) * (size_t)len);
  RO_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
  RO_HIP(hipMemsetAsync(mark, 0, sizeof(int) * (size_t)len, s));
  hipLaunchKernelGGL(k_check_perm, grid256(len), dim3(256), 0, s, len, dP, mark, bad, (int)BAD_PERM);
  int hbad = 0;
  if (read_flag(s, bad, &hbad)) return sc.done(SPGEMM_ERR_HIP);
  if (hbad) return sc.done(fail(SPGEMM_ERR_INPUT, "P is not a permutation of 0..%d", len - 1));
  hipLaunchKernelGGL(k_invert_perm, grid256(len), dim3(256), 0, s, len, dP, dPt);
  RO_HIP(hipGetLastError());
  RO_HIP(hipStreamSynchronize(s));
  return sc.done(SPGEMM_OK);
}

extern "C" int hip_csr_row_descending_permutation(spgemm_handle* h, int m, const int* dIA, int** dP) {
  using namespace reorder;
  if (!dP) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dP = nullptr;
  if (m < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (m > 0 && !dIA) return fail(SPGEMM_ERR_ARG, "rowPtr is null with m=%d", m);
  if (!h) CHK(default_handle(&h));
  HIPCHK(hipSetDevice(h->device));
  clear_stale_hip_error();
  hipStream_t s = h->stream;
  Scratch sc;
  int *flags = nullptr, *lens = nullptr, *idxA = nullptr, *idxB = nullptr, *bhist = nullptr;
  unsigned long long *keyA = nullptr, *keyB = nullptr, *tile = nullptr;
  RO_ALLOC(&idxA, sizeof(int) * (size_t)std::max(m, 1), true);
  if (m == 0) { *dP = idxA; return sc.done(SPGEMM_OK); }
  RO_ALLOC(&flags, sizeof(int) * 2);                      // {bad, maxLen}
  RO_ALLOC(&lens, sizeof(int) * (size_t)m);
  RO_HIP(hipMemsetAsync(flags, 0, sizeof(int) * 2, s));
  hipLaunchKernelGGL(k_check_rowptr, grid256(m), dim3(256), 0, s, m, -1, dIA, lens, flags + 1, flags);
  int hf[2] = {0, 0};
  RO_HIP(hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, s));
  RO_HIP(hipStreamSynchronize(s));
  if (hf[0]) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer"));
  const int maxLen = hf[1], keyBits = bits_of(maxLen);
  if (keyBits == 0) {                                     // no entries at all: every row ties, ascending row id
    hipLaunchKernelGGL(k_iota, grid256(m), dim3(256), 0, s, m, idxA);
  } else {
    const int nblk = cdiv(m, coo::RS_TILE);
    RO_ALLOC(&idxB, sizeof(int) * (size_t)m);
    RO_ALLOC(&keyA, sizeof(unsigned long long) * (size_t)m);
    RO_ALLOC(&keyB, sizeof(unsigned long long) * (size_t)m);
    RO_ALLOC(&bhist, sizeof(int) * ((size_t)nblk * coo::RS_RADIX + 1));
    RO_ALLOC(&tile, scan_scratch_bytes((long long)nblk * coo::RS_RADIX + 1));
    hipLaunchKernelGGL(k_desc_keys, grid256(m), dim3(256), 0, s, m, maxLen, lens, keyA, idxA);
    int* const outBuf = idxA;
    radix_sort_bits(s, m, 0, keyBits, keyA, keyB, idxA, idxB, bhist, tile);
    if (idxA != outBuf)                                   // an odd number of passes left the ids in the scratch array
      RO_HIP(hipMemcpyAsync(outBuf, idxA, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, s));
    idxA = outBuf;
  }
  RO_HIP(hipGetLastError());
  RO_HIP(hipStreamSynchronize(s));
  *dP = idxA;
  return sc.done(SPGEMM_OK);
}

#undef RO_ALLOC
#undef RO_HIP
