// Column-partitioned CSR on the device: split into c column blocks, blockwise product, join.
//
// Replaces, on device arrays,
//   PCSR::PCSR(const CSR&, c)                 nlibs/PCSR.cc:3-56     (count per block, blockPtr, a second pass that fills)
//   PCSR::isEqual's row walk                  nlibs/PCSR.h:52-100    (block 0's row i, block 1's row i, ...: hip_pcsr_join)
//   spmm(A, pB)                               correctTests/pcsrTest.cc:7-19  (one product per block: hip_pcsr_spmm)
//
// Layout (the reference's): stride = ceil(n / c); an entry with column col belongs to block b = col / stride with local
// column col - b * stride; rowPtr is int[c * (m + 1)], block b's at b * (m + 1), starting at 0; colInd / values hold nnz
// entries, block b's at blockPtr[b]; inside a block the entries are in row order, inside a row in A's storage order.
//
// Split.  A CSR is in row order already, so a stable sort of the entries by block id alone gives (block, row, storage
// order): exactly that layout.  As hip_csr_transpose does with the column, the block id goes on top of a 64-bit key and
// the stable LSD radix passes of csr_common_device.hpp run over the bits_of(c - 1) block bits only -- one pass for any c <= 64,
// none for c == 1.  key = ((block << rowBits) | row) << colBits | local column.  The local column rides in the low bits
// because the payload of a float entry is its value's bits (nothing then leads back to the source entry; a double entry
// carries its source index instead, and its value is gathered by the emit kernel): bits_of(c - 1) + bits_of(stride - 1)
// <= 32 and rowBits <= 31, so the key always fits.  The c * (m + 1) rowPtr entries and blockPtr are the boundaries of the
// sorted keys (one search per entry, inside its block), made block-local.  No per-(row, block) counters, no atomics.
//
// Join.  Row lengths summed over the blocks, the library's scan, then one copy kernel that deals OUTPUT entries, 1024 per
// block as k_permute_copy does: the row by a search in the new rowPtr bounded by the tile's rows, the block by walking the
// at most c block lengths of that row, lane-strided reads staged in LDS, 16-byte stores.  A 20 000-entry row is spread
// over 20 blocks like any other 20 000 entries.  The 3 c block pointers reach the kernels as ONE BY-VALUE KERNEL ARGUMENT
// (Blocks<V>, 1.5 KB of the 4 KB kernarg segment): no table upload, and the pointers are read through the kernarg segment
// like any other constant.
//
// Every value that becomes an address (rowPtr of A / of every block, the column that selects a block) is checked first by
// k_check_rowptr / k_check_cols; the host reads the flag before anything is queued that indexes with them.
// Uses csr_common_device.hpp (the checks and their one read-back, row search, lower bound, scan, radix sort, tile copy,
// Scratch).
#pragma once

namespace pcsr {

using namespace csrdev;

template <class V>
struct Blocks {
  const int* I[SPGEMM_PCSR_MAX_BLOCKS];
  const int* J[SPGEMM_PCSR_MAX_BLOCKS];
  const V* A[SPGEMM_PCSR_MAX_BLOCKS];
};

static inline int stride_of(int n, int c) { return std::max(1, (int)(((long long)n + c - 1) / c)); }

// split keys, dealt by entries (lane-strided inside the block's tile: every access coalesced); rowPtr and the columns have
// been validated, so block < c.  payload: value bits (4-byte values) or entry index.
template <class V>
__global__ __launch_bounds__(CP_THREADS) void k_split_keys(int m, int nnz, int stride, int rowBits, int colBits,
                                                           const int* __restrict__ IA, const int* __restrict__ JA,
                                                           const V* __restrict__ A, unsigned long long* __restrict__ keys,
                                                           int* __restrict__ payload) {
  __shared__ int rows[2];
  const long long base = (long long)blockIdx.x * CP_TILE;
  tile_rows(IA, m, nnz, base, rows);
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const long long o = base + k * CP_THREADS + threadIdx.x;
    if (o >= nnz) break;
    const int r = row_of_entry(IA, rows[0], rows[1], (int)o);
    const int col = JA[o], b = col / stride;
    keys[o] = (((((unsigned long long)(unsigned)b) << rowBits) | (unsigned)r) << colBits) | (unsigned)(col - b * stride);
    if constexpr (sizeof(V) == 4) payload[o] = __float_as_int(A[o]); else payload[o] = (int)o;
  }
}

template <class V>
__global__ void k_split_emit(int nnz, int colBits, const unsigned long long* __restrict__ keys,
                             const int* __restrict__ payload, const V* __restrict__ A, int* __restrict__ JP,
                             V* __restrict__ P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  JP[i] = (int)(keys[i] & ((1ull << colBits) - 1ull));
  if constexpr (sizeof(V) == 4) P[i] = __int_as_float(payload[i]); else P[i] = A[payload[i]];
}

// blockPtr[b] = first sorted key of block b or later, b = 0..c
__global__ void k_block_starts(int c, int nnz, int shift, const unsigned long long* __restrict__ keys,
                               int* __restrict__ blockPtr) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b <= c) blockPtr[b] = first_at_least(keys, 0, nnz, (unsigned long long)(unsigned)b << shift);
}

// IP[b * (m + 1) + r] = entries of block b in rows below r, r = 0..m: one search per entry, inside the block
__global__ void k_split_rowptr(int m, int c, int rowBits, int colBits, const unsigned long long* __restrict__ keys,
                               const int* __restrict__ blockPtr, int* __restrict__ IP) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)c * (m + 1)) return;
  const int b = (int)(i / (m + 1)), r = (int)(i - (long long)b * (m + 1));
  const int s = blockPtr[b];
  const unsigned long long want = (((unsigned long long)(unsigned)b << rowBits) + (unsigned)r) << colBits;   // r == m: the next block
  IP[i] = first_at_least(keys, s, blockPtr[b + 1], want) - s;
}

template <class V>
__global__ void k_join_lens(int m, int c, Blocks<V> blk, int* __restrict__ IC) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  int len = 0;
  for (int b = 0; b < c; ++b) len += blk.I[b][r + 1] - blk.I[b][r];
  IC[r] = len;
}

// One tile of C's entries per block, as tile_copy: the row by a search in IC bounded by the tile's rows, the block by
// walking the row's block lengths, the source position from that block's rowPtr; column made global; staged in LDS for
// tile_store.  The gather loop is written out here: as a tile_copy functor the block walk compiled to a longer loop.
template <class V>
__global__ __launch_bounds__(CP_THREADS) void k_join_copy(int m, int nnz, int c, int stride, Blocks<V> blk,
                                                          const int* __restrict__ IC, int* __restrict__ JC,
                                                          V* __restrict__ C) {
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
      int off = (int)o - IC[r], b = 0, s = blk.I[0][r], len = blk.I[0][r + 1] - s;
      while (off >= len && b + 1 < c) {             // the lengths add up to the row's: ends at the latest in the last block
        off -= len;
        ++b;
        s = blk.I[b][r];
        len = blk.I[b][r + 1] - s;
      }
      sc[t] = blk.J[b][s + off] + b * stride;
      sv[t] = blk.A[b][s + off];
    }
  }
  tile_store<V>(base, nnz, sc, sv, JC, C);
}

static int check_block_count(int c) {
  if (c < 1 || c > SPGEMM_PCSR_MAX_BLOCKS) return fail(SPGEMM_ERR_ARG, "c=%d outside [1,%d]", c, SPGEMM_PCSR_MAX_BLOCKS);
  return SPGEMM_OK;
}

template <class V>
static int split_columns(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, int c,
                         int** dIP, int** dJP, V** dP, int* blockPtr) {
  if (!dIP || !dJP || !dP || !blockPtr) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIP = nullptr; *dJP = nullptr; *dP = nullptr;
  CHK(check_block_count(c));
  CHK(check_csr_args(m, n, nnz, dIA, dJA, dA));
  const long long ipLen = (long long)c * ((long long)m + 1);
  if (ipLen > INT_MAX) return fail(SPGEMM_ERR_OVERFLOW, "c * (m + 1) = %lld row pointer entries do not fit int32", ipLen);
  for (int b = 0; b <= c; ++b) blockPtr[b] = 0;
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *IP = nullptr, *JP = nullptr, *idxA = nullptr, *idxB = nullptr, *bhist = nullptr, *dBlockPtr = nullptr;
  V* P = nullptr;
  unsigned long long *keyA = nullptr, *keyB = nullptr, *tile = nullptr;
  // validation, one read-back: rowPtr (the key kernel searches it) and the column range (the block id becomes an address)
  int hbad = 0;
  if (int rc = validate_csr(sc, s, m, n, nnz, dIA, dJA, &hbad)) return sc.done(rc);
  if (hbad & BAD_ROWPTR) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer ending at nnz=%d", nnz));
  if (hbad & BAD_COLUMN) return sc.done(fail(SPGEMM_ERR_INPUT, "column outside [0,%d)", n));
  CSR_ALLOC(&IP, sizeof(int) * (size_t)ipLen, true);
  CSR_ALLOC(&JP, sizeof(int) * (size_t)std::max(nnz, 1), true);
  CSR_ALLOC(&P, sizeof(V) * (size_t)std::max(nnz, 1), true);
  if (nnz == 0) {
    CSR_HIP(hipMemsetAsync(IP, 0, sizeof(int) * (size_t)ipLen, s));
    CSR_HIP(hipStreamSynchronize(s));
    *dIP = IP; *dJP = JP; *dP = P;
    return sc.done(SPGEMM_OK);
  }
  const int stride = stride_of(n, c);
  const int rowBits = std::max(1, bits_of(m - 1)), colBits = std::max(1, bits_of(stride - 1)), blockBits = bits_of(c - 1);
  const int nblk = cdiv(nnz, RS_TILE);
  CSR_ALLOC(&keyA, sizeof(unsigned long long) * (size_t)nnz);
  CSR_ALLOC(&idxA, sizeof(int) * (size_t)nnz);
  CSR_ALLOC(&dBlockPtr, sizeof(int) * ((size_t)c + 1));
  if (blockBits > 0) {
    CSR_ALLOC(&keyB, sizeof(unsigned long long) * (size_t)nnz);
    CSR_ALLOC(&idxB, sizeof(int) * (size_t)nnz);
    CSR_ALLOC(&bhist, sizeof(int) * ((size_t)nblk * RS_RADIX + 1));
    CSR_ALLOC(&tile, scan_scratch_bytes((long long)nblk * RS_RADIX + 1));
  }
  hipLaunchKernelGGL(k_split_keys<V>, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, stride, rowBits,
                     colBits, dIA, dJA, dA, keyA, idxA);
  radix_sort_bits(s, nnz, rowBits + colBits, rowBits + colBits + blockBits, keyA, keyB, idxA, idxB, bhist, tile);
  hipLaunchKernelGGL(k_split_emit<V>, grid256(nnz), dim3(256), 0, s, nnz, colBits, keyA, idxA, dA, JP, P);
  hipLaunchKernelGGL(k_block_starts, dim3(1), dim3(128), 0, s, c, nnz, rowBits + colBits, keyA, dBlockPtr);
  hipLaunchKernelGGL(k_split_rowptr, grid256(ipLen), dim3(256), 0, s, m, c, rowBits, colBits, keyA, dBlockPtr, IP);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipMemcpyAsync(blockPtr, dBlockPtr, sizeof(int) * ((size_t)c + 1), hipMemcpyDeviceToHost, s));
  CSR_HIP(hipStreamSynchronize(s));
  *dIP = IP; *dJP = JP; *dP = P;
  return sc.done(SPGEMM_OK);
}

// the c blocks of a partitioned matrix as the caller hands them over: host arrays of device pointers and counts
template <class V>
static int check_blocks(int rows, int c, const int* const* dIB, const int* const* dJB, const V* const* dB, const int* nnzB,
                        long long* total) {
  if (!dIB || !dJB || !dB || !nnzB) return fail(SPGEMM_ERR_ARG, "block table is null");
  *total = 0;
  for (int b = 0; b < c; ++b) {
    if (nnzB[b] < 0) return fail(SPGEMM_ERR_ARG, "block %d: negative nnz", b);
    if (!dIB[b]) return fail(SPGEMM_ERR_ARG, "block %d: rowPtr is null", b);
    if (nnzB[b] > 0 && (!dJB[b] || !dB[b])) return fail(SPGEMM_ERR_ARG, "block %d: colInd/values null with nnz=%d", b, nnzB[b]);
    if (rows == 0 && nnzB[b] > 0) return fail(SPGEMM_ERR_ARG, "block %d: nnz=%d in a matrix without rows", b, nnzB[b]);
    *total += nnzB[b];
  }
  return SPGEMM_OK;
}

template <class V>
static int join(spgemm_handle* h, int m, int n, int c, const int* const* dIB, const int* const* dJB, const V* const* dB,
                const int* nnzB, int** dIC, int** dJC, V** dC, int* nnzC) {
  if (!dIC || !dJC || !dC || !nnzC) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIC = nullptr; *dJC = nullptr; *dC = nullptr; *nnzC = 0;
  CHK(check_block_count(c));
  if (m < 0 || n < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  long long total = 0;
  CHK(check_blocks<V>(m, c, dIB, dJB, dB, nnzB, &total));
  if (total > INT_MAX) return fail(SPGEMM_ERR_OVERFLOW, "%lld entries do not fit the int32 CSR", total);
  const int nnz = (int)total, stride = stride_of(n, c);
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *bad = nullptr, *IC = nullptr, *JC = nullptr;
  V* C = nullptr;
  unsigned long long* tile = nullptr;
  Blocks<V> blk = {};
  for (int b = 0; b < c; ++b) { blk.I[b] = dIB[b]; blk.J[b] = dJB[b]; blk.A[b] = dB[b]; }
  // validation, one read-back: every block's rowPtr against its count (they become addresses), every local column inside
  // [0, stride) and its global column below n (the result must be a valid m x n CSR)
  if (int rc = flag_begin(sc, s, &bad)) return sc.done(rc);
  for (int b = 0; b < c; ++b) {
    const long long room = std::min<long long>(stride, (long long)n - (long long)b * stride);
    queue_csr_checks(s, m, (int)std::max<long long>(room, 0), nnzB[b], dIB[b], dJB[b], bad);
  }
  int hbad = 0;
  if (read_flag(s, bad, &hbad)) return sc.done(SPGEMM_ERR_HIP);
  if (hbad & BAD_ROWPTR) return sc.done(fail(SPGEMM_ERR_INPUT, "a block's rowPtr is not a monotone row pointer ending at its nnz"));
  if (hbad & BAD_COLUMN) return sc.done(fail(SPGEMM_ERR_INPUT, "a block's column is outside [0,%d) or its global column outside [0,%d)", stride, n));
  CSR_ALLOC(&IC, sizeof(int) * ((size_t)m + 1), true);
  CSR_ALLOC(&JC, sizeof(int) * (size_t)std::max(nnz, 1), true);
  CSR_ALLOC(&C, sizeof(V) * (size_t)std::max(nnz, 1), true);
  CSR_ALLOC(&tile, scan_scratch_bytes((long long)m + 1));
  if (m > 0) hipLaunchKernelGGL(k_join_lens<V>, grid256(m), dim3(256), 0, s, m, c, blk, IC);
  scan_inplace(s, IC, m, tile);
  if (nnz > 0)
    hipLaunchKernelGGL(k_join_copy<V>, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, c, stride, blk, IC,
                       JC, C);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  *dIC = IC; *dJC = JC; *dC = C; *nnzC = nnz;
  return sc.done(SPGEMM_OK);
}

static int block_product(spgemm_handle* h, const int* dIA, const int* dJA, const float* dA, int nnzA, const int* dIB,
                         const int* dJB, const float* dB, int nnzB, int m, int k, int n, int** dIC, int** dJC, float** dC,
                         int* nnzC) {
  return hip_gpuSpMM(h, dIA, dJA, dA, nnzA, dIB, dJB, dB, nnzB, m, k, n, dIC, dJC, dC, nnzC);
}
static int block_product(spgemm_handle* h, const int* dIA, const int* dJA, const double* dA, int nnzA, const int* dIB,
                         const int* dJB, const double* dB, int nnzB, int m, int k, int n, int** dIC, int** dJC, double** dC,
                         int* nnzC) {
  return hip_gpuSpMM_f64(h, dIA, dJA, dA, nnzA, dIB, dJB, dB, nnzB, m, k, n, dIC, dJC, dC, nnzC);
}

// spmm(A, pB): one product of the existing path per block, on one handle; a host loop, no kernel of its own
template <class V>
static int spmm(spgemm_handle* h, const int* dIA, const int* dJA, const V* dA, int nnzA, int m, int k, int n, int c,
                const int* const* dIB, const int* const* dJB, const V* const* dB, const int* nnzB, int** dIC, int** dJC,
                V** dC, int* nnzC) {
  CHK(check_block_count(c));
  if (!dIC || !dJC || !dC || !nnzC) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  for (int b = 0; b < c; ++b) { dIC[b] = nullptr; dJC[b] = nullptr; dC[b] = nullptr; nnzC[b] = 0; }
  if (m < 0 || k < 0 || n < 0) return fail(SPGEMM_ERR_ARG, "negative dimension m=%d k=%d n=%d", m, k, n);
  CHK(check_common(dIA, dJA, dA, nnzA, "A"));
  long long total = 0;
  CHK(check_blocks<V>(k, c, dIB, dJB, dB, nnzB, &total));
  const int stride = stride_of(n, c);
  for (int b = 0; b < c; ++b) {
    const int rc = block_product(h, dIA, dJA, dA, nnzA, dIB[b], dJB[b], dB[b], nnzB[b], m, k, stride, &dIC[b], &dJC[b],
                                 &dC[b], &nnzC[b]);
    if (rc == SPGEMM_OK) continue;
    for (int q = 0; q <= b; ++q) {                  // the failing block's message stays in spgemm_hip_last_error
      pool().release(dIC[q]); pool().release(dJC[q]); pool().release(dC[q]);
      dIC[q] = nullptr; dJC[q] = nullptr; dC[q] = nullptr; nnzC[q] = 0;
    }
    return rc;
  }
  return SPGEMM_OK;
}

}  // namespace pcsr

extern "C" int hip_csr_split_columns(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                                     int c, int** dIP, int** dJP, float** dP, int* blockPtr) {
  return pcsr::split_columns<float>(h, m, n, nnz, dIA, dJA, dA, c, dIP, dJP, dP, blockPtr);
}

extern "C" int hip_csr_split_columns_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA,
                                         const double* dA, int c, int** dIP, int** dJP, double** dP, int* blockPtr) {
  return pcsr::split_columns<double>(h, m, n, nnz, dIA, dJA, dA, c, dIP, dJP, dP, blockPtr);
}

extern "C" int hip_pcsr_join(spgemm_handle* h, int m, int n, int c, const int* const* dIB, const int* const* dJB,
                             const float* const* dB, const int* nnzB, int** dIC, int** dJC, float** dC, int* nnzC) {
  return pcsr::join<float>(h, m, n, c, dIB, dJB, dB, nnzB, dIC, dJC, dC, nnzC);
}

extern "C" int hip_pcsr_join_f64(spgemm_handle* h, int m, int n, int c, const int* const* dIB, const int* const* dJB,
                                 const double* const* dB, const int* nnzB, int** dIC, int** dJC, double** dC, int* nnzC) {
  return pcsr::join<double>(h, m, n, c, dIB, dJB, dB, nnzB, dIC, dJC, dC, nnzC);
}

extern "C" int hip_pcsr_spmm(spgemm_handle* h, const int* dIA, const int* dJA, const float* dA, int nnzA, int m, int k, int n,
                             int c, const int* const* dIB, const int* const* dJB, const float* const* dB, const int* nnzB,
                             int** dIC, int** dJC, float** dC, int* nnzC) {
  return pcsr::spmm<float>(h, dIA, dJA, dA, nnzA, m, k, n, c, dIB, dJB, dB, nnzB, dIC, dJC, dC, nnzC);
}

extern "C" int hip_pcsr_spmm_f64(spgemm_handle* h, const int* dIA, const int* dJA, const double* dA, int nnzA, int m, int k,
                                 int n, int c, const int* const* dIB, const int* const* dJB, const double* const* dB,
                                 const int* nnzB, int** dIC, int** dJC, double** dC, int* nnzC) {
  return pcsr::spmm<double>(h, dIA, dJA, dA, nnzA, m, k, n, c, dIB, dJB, dB, nnzB, dIC, dJC, dC, nnzC);
}
