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
// The two sorts are the stable LSD radix passes of csr_common_device.hpp over exactly the bits the shape needs:
//   transpose   key = (col << rowBits) | row, passes over the column bits only (a CSR is in row order already, so a stable
//               sort by column gives (column, row) order); payload = the value's bits (float) or the source index (double)
//   descending  key = maxLen - len, payload = row id (equal lengths keep ascending row id)
// Every value that becomes an address (rowSrc, colMap, a permutation to invert, columns renamed through colMap, rowPtr)
// is checked first by kernels that only read the input and write a flag / mark array of our own; the host reads the flag
// before anything is queued that indexes with those values.
// Uses csr_common_device.hpp (the checks and their one read-back, row search, scan, radix sort, tile copy, Scratch).
#pragma once

namespace reorder {

using namespace csrdev;

// P is a permutation of 0..len-1  <=>  every value is in range and none is seen twice (mark: zeroed int[len] of ours)
__global__ void k_check_perm(int len, const int* __restrict__ P, int* __restrict__ mark, int* __restrict__ bad, int bit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= len) return;
  const int v = P[i];
  if ((unsigned)v >= (unsigned)len) { atomicOr(bad, bit); return; }
  if (atomicExch(&mark[v], 1) != 0) atomicOr(bad, bit);
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

// One tile of B's entries per block (tile_copy): entry `off` of B's row r is entry `off` of A's row rowSrc[r], its column
// renamed through colMap.
template <class V>
__global__ __launch_bounds__(CP_THREADS) void k_permute_copy(int m, int nnz, const int* __restrict__ IA,
                                                             const int* __restrict__ JA, const V* __restrict__ A,
                                                             const int* __restrict__ rowSrc, const int* __restrict__ colMap,
                                                             const int* __restrict__ IB, int* __restrict__ JB,
                                                             V* __restrict__ B) {
  tile_copy<V>(m, nnz, IB, JB, B, [&](int r, int off, int& col, V& val) {
    const int p = IA[rowSrc ? rowSrc[r] : r] + off;
    const int cc = JA[p];
    col = colMap ? colMap[cc] : cc;
    val = A[p];
  });
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

// IT[c] = first sorted key of column c or later (one search per output row), c = 0..n
__global__ void k_col_starts(int n, int nnz, int rowBits, const unsigned long long* __restrict__ keys, int* __restrict__ IT) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= n) IT[c] = first_at_least(keys, 0, nnz, (unsigned long long)(unsigned)c << rowBits);
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

template <class V>
static int permute(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, const int* dRowSrc,
                   const int* dColMap, int** dIB, int** dJB, V** dB) {
  if (!dIB || !dJB || !dB) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIB = nullptr; *dJB = nullptr; *dB = nullptr;
  CHK(check_csr_args(m, n, nnz, dIA, dJA, dA));
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *bad = nullptr, *mark = nullptr, *IB = nullptr, *JB = nullptr;
  V* B = nullptr;
  unsigned long long* tile = nullptr;
  // (1) validation: rowPtr, the two permutations, and the columns that will index colMap
  if (int rc = flag_begin(sc, s, &bad)) return sc.done(rc);
  queue_csr_checks(s, m, n, nnz, dIA, nullptr, bad);      // the columns are checked below, and only for a colMap
  const long long marks = (dRowSrc ? (long long)m : 0) + (dColMap ? (long long)n : 0);
  if (marks > 0) {
    CSR_ALLOC(&mark, sizeof(int) * (size_t)marks);
    CSR_HIP(hipMemsetAsync(mark, 0, sizeof(int) * (size_t)marks, s));
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
  CSR_ALLOC(&IB, sizeof(int) * ((size_t)m + 1), true);
  CSR_ALLOC(&JB, sizeof(int) * (size_t)std::max(nnz, 1), true);
  CSR_ALLOC(&B, sizeof(V) * (size_t)std::max(nnz, 1), true);
  CSR_ALLOC(&tile, scan_scratch_bytes((long long)m + 1));
  if (m > 0) hipLaunchKernelGGL(k_gather_lens, grid256(m), dim3(256), 0, s, m, dIA, dRowSrc, IB);
  scan_inplace(s, IB, m, tile);
  // (3) entries: gathered and renamed in one pass
  if (nnz > 0)
    hipLaunchKernelGGL(k_permute_copy<V>, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, dIA, dJA, dA,
                       dRowSrc, dColMap, IB, JB, B);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  *dIB = IB; *dJB = JB; *dB = B;
  return sc.done(SPGEMM_OK);
}

template <class V>
static int transpose(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, int** dIT,
                     int** dJT, V** dAT) {
  if (!dIT || !dJT || !dAT) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIT = nullptr; *dJT = nullptr; *dAT = nullptr;
  CHK(check_csr_args(m, n, nnz, dIA, dJA, dA));
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *IT = nullptr, *JT = nullptr, *idxA = nullptr, *idxB = nullptr, *bhist = nullptr;
  V* AT = nullptr;
  unsigned long long *keyA = nullptr, *keyB = nullptr, *tile = nullptr;
  // validation, one read-back: rowPtr (the key kernel searches it) and the column range
  int hbad = 0;
  if (int rc = validate_csr(sc, s, m, n, nnz, dIA, dJA, &hbad)) return sc.done(rc);
  if (hbad & BAD_ROWPTR) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer ending at nnz=%d", nnz));
  if (hbad & BAD_COLUMN) return sc.done(fail(SPGEMM_ERR_INPUT, "column outside [0,%d)", n));
  CSR_ALLOC(&IT, sizeof(int) * ((size_t)n + 1), true);
  CSR_ALLOC(&JT, sizeof(int) * (size_t)std::max(nnz, 1), true);
  CSR_ALLOC(&AT, sizeof(V) * (size_t)std::max(nnz, 1), true);
  if (nnz == 0) {
    CSR_HIP(hipMemsetAsync(IT, 0, sizeof(int) * ((size_t)n + 1), s));
    CSR_HIP(hipStreamSynchronize(s));
    *dIT = IT; *dJT = JT; *dAT = AT;
    return sc.done(SPGEMM_OK);
  }
  const int rowBits = std::max(1, bits_of(m - 1)), colBits = std::max(1, bits_of(n - 1));
  const int nblk = cdiv(nnz, RS_TILE);
  CSR_ALLOC(&keyA, sizeof(unsigned long long) * (size_t)nnz);
  CSR_ALLOC(&keyB, sizeof(unsigned long long) * (size_t)nnz);
  CSR_ALLOC(&idxA, sizeof(int) * (size_t)nnz);
  CSR_ALLOC(&idxB, sizeof(int) * (size_t)nnz);
  CSR_ALLOC(&bhist, sizeof(int) * ((size_t)nblk * RS_RADIX + 1));
  CSR_ALLOC(&tile, scan_scratch_bytes((long long)nblk * RS_RADIX + 1));
  hipLaunchKernelGGL(k_transpose_keys<V>, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, rowBits, dIA,
                     dJA, dA, keyA, idxA);
  radix_sort_bits(s, nnz, rowBits, rowBits + colBits, keyA, keyB, idxA, idxB, bhist, tile);
  hipLaunchKernelGGL(k_transpose_emit<V>, grid256(nnz), dim3(256), 0, s, nnz, rowBits, keyA, idxA, dA, JT, AT);
  hipLaunchKernelGGL(k_col_starts, grid256((long long)n + 1), dim3(256), 0, s, n, nnz, rowBits, keyA, IT);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
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
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *bad = nullptr, *mark = nullptr;
  if (int rc = flag_begin(sc, s, &bad)) return sc.done(rc);
  CSR_ALLOC(&mark, sizeof(int) * (size_t)len);
  CSR_HIP(hipMemsetAsync(mark, 0, sizeof(int) * (size_t)len, s));
  hipLaunchKernelGGL(k_check_perm, grid256(len), dim3(256), 0, s, len, dP, mark, bad, (int)BAD_PERM);
  int hbad = 0;
  if (read_flag(s, bad, &hbad)) return sc.done(SPGEMM_ERR_HIP);
  if (hbad) return sc.done(fail(SPGEMM_ERR_INPUT, "P is not a permutation of 0..%d", len - 1));
  hipLaunchKernelGGL(k_invert_perm, grid256(len), dim3(256), 0, s, len, dP, dPt);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  return sc.done(SPGEMM_OK);
}

extern "C" int hip_csr_row_descending_permutation(spgemm_handle* h, int m, const int* dIA, int** dP) {
  using namespace reorder;
  if (!dP) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dP = nullptr;
  if (m < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (m > 0 && !dIA) return fail(SPGEMM_ERR_ARG, "rowPtr is null with m=%d", m);
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *flags = nullptr, *lens = nullptr, *idxA = nullptr, *idxB = nullptr, *bhist = nullptr;
  unsigned long long *keyA = nullptr, *keyB = nullptr, *tile = nullptr;
  CSR_ALLOC(&idxA, sizeof(int) * (size_t)std::max(m, 1), true);
  if (m == 0) { *dP = idxA; return sc.done(SPGEMM_OK); }
  CSR_ALLOC(&flags, sizeof(int) * 2);                      // {bad, maxLen}
  CSR_ALLOC(&lens, sizeof(int) * (size_t)m);
  CSR_HIP(hipMemsetAsync(flags, 0, sizeof(int) * 2, s));
  hipLaunchKernelGGL(k_check_rowptr, grid256(m), dim3(256), 0, s, m, -1, dIA, lens, flags + 1, flags);
  int hf[2] = {0, 0};
  CSR_HIP(hipMemcpyAsync(hf, flags, sizeof(hf), hipMemcpyDeviceToHost, s));
  CSR_HIP(hipStreamSynchronize(s));
  if (hf[0]) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer"));
  const int maxLen = hf[1], keyBits = bits_of(maxLen);
  if (keyBits == 0) {                                     // no entries at all: every row ties, ascending row id
    hipLaunchKernelGGL(k_iota, grid256(m), dim3(256), 0, s, m, idxA);
  } else {
    const int nblk = cdiv(m, RS_TILE);
    CSR_ALLOC(&idxB, sizeof(int) * (size_t)m);
    CSR_ALLOC(&keyA, sizeof(unsigned long long) * (size_t)m);
    CSR_ALLOC(&keyB, sizeof(unsigned long long) * (size_t)m);
    CSR_ALLOC(&bhist, sizeof(int) * ((size_t)nblk * RS_RADIX + 1));
    CSR_ALLOC(&tile, scan_scratch_bytes((long long)nblk * RS_RADIX + 1));
    hipLaunchKernelGGL(k_desc_keys, grid256(m), dim3(256), 0, s, m, maxLen, lens, keyA, idxA);
    int* const outBuf = idxA;
    radix_sort_bits(s, m, 0, keyBits, keyA, keyB, idxA, idxB, bhist, tile);
    if (idxA != outBuf)                                   // an odd number of passes left the ids in the scratch array
      CSR_HIP(hipMemcpyAsync(outBuf, idxA, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, s));
    idxA = outBuf;
  }
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  *dP = idxA;
  return sc.done(SPGEMM_OK);
}
