// COO -> CSR on the device: the step in front of the SpGEMM path.
//
// Replaces, on device arrays,
//   COO::addSelfLoopIfNeeded                       nlibs/COO.cc:160-188
//   COO::makeOrdered / orderedAndDuplicatesRemoving nlibs/COO.cc:222-266   (std::sort on (row,col) tuples; duplicates summed)
//   COO::toCSR                                      nlibs/COO.cc:268-291
//   CSR::averAndNormRowQValue                       nlibs/CSR.cc:88-95      (every entry of row i becomes 1/count(i))
//   CSR::toAbs                                      nlibs/CSR.h:152-158
// i.e. what rmclInit (nlibs/qrmcl.cc:126-134) and the Matrix-Market/SNAP loaders do after parsing the text.
//
// The sort is our own stable LSD radix sort (8 bits per pass: per-block digit histograms in LDS, the library's scan
// kernels over the digit-major histogram, ballot-ranked stable scatter) of the 64-bit key (row << colBits) | col carrying
// the entry's value, over exactly the bits the shape needs.  Stable order = input order inside a run of equal
// (row,col), so duplicates are summed left to right like the CPU loop (bit-exact floats; a run is summed by one lane,
// which is what keeps the order -- a pair repeated very many times serialises that lane).
// Generic over the value type V.  The sort's payload is one int: for float it is the value's bits, so the emit step reads
// keys and values in order; a double does not fit, so for double the payload is the entry's INDEX (nnz + k for the k-th
// appended self loop) and the emit step gathers dVal[index], an index >= nnz standing for 1.0.  Sums, |.| and 1/count are
// computed in V.
// Uses csr_common_device.hpp (the radix sort, scan, Scratch, call prologue).
#pragma once

namespace coo {

using namespace csrdev;

__global__ void k_check_and_diag(int nnz, int rows, int cols, const int* __restrict__ ri, const int* __restrict__ ci,
                                 unsigned char* __restrict__ hasDiag, int* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const int r = ri[i], c = ci[i];
  if ((unsigned)r >= (unsigned)rows || (unsigned)c >= (unsigned)cols) { atomicOr(bad, 1); return; }
  if (hasDiag && r == c) hasDiag[r] = 1;
}

__global__ void k_missing_flags(int rows, const unsigned char* __restrict__ hasDiag, int* __restrict__ miss) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < rows) miss[r] = hasDiag[r] ? 0 : 1;
}

// the payload of entry i (i >= nnz: an appended self loop, value 1.0) and the value a sorted payload stands for
__device__ __forceinline__ int payload_of(const float* __restrict__ val, int nnz, int i) {
  return __float_as_int(i < nnz ? val[i] : 1.0f);
}
__device__ __forceinline__ int payload_of(const double*, int, int i) { return i; }
__device__ __forceinline__ float value_of(const float*, int, int payload) { return __int_as_float(payload); }
__device__ __forceinline__ double value_of(const double* __restrict__ val, int nnz, int payload) {
  return (unsigned)payload < (unsigned)nnz ? val[payload] : 1.0;
}

// keys of the original entries and of the appended self loops: (row << colBits) | col, same order as row * cols + col
// without a 64-bit division on the way back.  The payload that travels with a key through the (stable) sort is, for
// float, the entry's VALUE: the emit step then reads keys and values in order instead of gathering values through an
// index.  For double it is the index (see the top of the file).
template <class V>
__global__ void k_make_keys(int nnz, int rows, int colBits, const int* __restrict__ ri, const int* __restrict__ ci,
                            const V* __restrict__ val, const int* __restrict__ missPos, const int* __restrict__ miss,
                            unsigned long long* __restrict__ keys, int* __restrict__ payload) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nnz) {
    keys[i] = ((unsigned long long)(unsigned)ri[i] << colBits) | (unsigned)ci[i];
    payload[i] = payload_of(val, nnz, i);
  }
  if (miss && i < rows && miss[i]) {            // self loop (i,i,1.0) appended behind the input, in row order
    const int p = nnz + missPos[i];
    keys[p] = ((unsigned long long)(unsigned)i << colBits) | (unsigned)i;
    payload[p] = payload_of(val, nnz, p);
  }
}

__global__ void k_heads(int n, const unsigned long long* __restrict__ keys, int dedupe, int* __restrict__ head) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) head[i] = (!dedupe || i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// one thread per output entry (= head of a run of equal keys): column and summed value (input order inside a run)
template <class V>
__global__ void k_emit(int n, int colBits, const unsigned long long* __restrict__ keys, const int* __restrict__ payload,
                       const int* __restrict__ head, const int* __restrict__ pos, const V* __restrict__ val, int nnz,
                       int dedupe, int useAbs, int* __restrict__ JA, V* __restrict__ A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !head[i]) return;
  const unsigned long long k = keys[i];
  V s = value_of(val, nnz, payload[i]);
  if (dedupe)
    for (int j = i + 1; j < n && keys[j] == k; ++j) s += value_of(val, nnz, payload[j]);
  const int o = pos[i];
  JA[o] = (int)(k & ((1ull << colBits) - 1ull));
  A[o] = useAbs ? (V)fabs(s) : s;                // fabs of a float is exact in double and back
}

// rowPtr straight from the sorted keys: IA[r] = output position of the first key of row r or later (binary search, one
// thread per row; pos[n] = number of output entries).  No per-entry atomics, no scan, empty rows need no special case.
__global__ void k_row_starts(int rows, int n, int colBits, const unsigned long long* __restrict__ keys,
                             const int* __restrict__ pos, int* __restrict__ IA) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > rows) return;
  IA[r] = pos[first_at_least(keys, 0, n, (unsigned long long)(unsigned)r << colBits)];
}

template <class V>
__global__ void k_row_normalise(int rows, const int* __restrict__ IA, V* __restrict__ A) {
  const int r = blockIdx.x * (blockDim.x >> 4) + (threadIdx.x >> 4), gl = threadIdx.x & 15;
  if (r >= rows) return;
  const int s = IA[r], e = IA[r + 1];
  const V w = (V)(1.0 / (double)(e - s));          // double division, narrowed for float (nlibs/CSR.cc:88-95)
  for (int p = s + gl; p < e; p += 16) A[p] = w;
}

template <class V>
static int coo_to_csr(spgemm_handle* h, int rows, int cols, int nnz, const int* dRow, const int* dCol, const V* dVal,
                      int flags, int** dIA, int** dJA, V** dA, int* nnzOut) {
  if (!dIA || !dJA || !dA || !nnzOut) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIA = nullptr; *dJA = nullptr; *dA = nullptr; *nnzOut = 0;
  if (rows < 0 || cols < 0 || nnz < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (nnz > 0 && (!dRow || !dCol || !dVal)) return fail(SPGEMM_ERR_ARG, "COO arrays null with nnz=%d", nnz);
  if ((flags & SPGEMM_COO_SELF_LOOPS) && rows != cols) return fail(SPGEMM_ERR_ARG, "self loops need a square matrix");
  hipStream_t s;
  CHK(enter(h, &s));
  const int dedupe = (flags & SPGEMM_COO_DEDUPE) ? 1 : 0;
  const bool loops = (flags & SPGEMM_COO_SELF_LOOPS) != 0;
  const long long maxTotal = (long long)nnz + (loops ? rows : 0);
  if (maxTotal > 0x7fffffffLL) return fail(SPGEMM_ERR_OVERFLOW, "nnz does not fit int32");

  Scratch sc;
  unsigned char* hasDiag = nullptr;
  int *bad = nullptr, *miss = nullptr, *missPos = nullptr, *idxA = nullptr, *idxB = nullptr, *head = nullptr, *pos = nullptr;
  unsigned long long *keyA = nullptr, *keyB = nullptr, *tile = nullptr;
  int* bhist = nullptr;                          // digit-major per-block histograms / offsets of the radix passes
  int *IA = nullptr, *JA = nullptr;
  V* A = nullptr;
  const int colBits = std::max(1, bits_of(cols - 1));      // key = (row << colBits) | col
  const int keyBits = std::max(1, bits_of(rows - 1) + colBits);
  // scratch of the scans: tile sums of the longest array scanned below (entries, rows + 1, or 256 x radix blocks)
  const long long nblkMax = (maxTotal + RS_TILE - 1) / RS_TILE + 1;
  const long long longest = std::max<long long>(std::max<long long>(maxTotal, (long long)rows + 1), nblkMax * RS_RADIX) + 1;
  CSR_ALLOC(&tile, scan_scratch_bytes(longest));
  if (int rc = flag_begin(sc, s, &bad)) return sc.done(rc);
  // (1) validation, diagonal flags, self loops to append
  int extra = 0;
  if (loops && rows > 0) {
    CSR_ALLOC(&hasDiag, (size_t)rows);
    CSR_ALLOC(&miss, sizeof(int) * (size_t)rows);
    CSR_ALLOC(&missPos, sizeof(int) * ((size_t)rows + 1));
    CSR_HIP(hipMemsetAsync(hasDiag, 0, (size_t)rows, s));
  }
  if (nnz > 0) hipLaunchKernelGGL(k_check_and_diag, grid256(nnz), dim3(256), 0, s, nnz, rows, cols, dRow, dCol, hasDiag, bad);
  if (loops && rows > 0) {
    hipLaunchKernelGGL(k_missing_flags, grid256(rows), dim3(256), 0, s, rows, hasDiag, miss);
    CSR_HIP(hipMemcpyAsync(missPos, miss, sizeof(int) * (size_t)rows, hipMemcpyDeviceToDevice, s));
    unsigned long long nmiss = 0;
    CSR_HIP(scan_total(s, missPos, rows, tile, &nmiss));
    extra = (int)nmiss;
  }
  int hbad = 0;
  if (read_flag(s, bad, &hbad)) return sc.done(SPGEMM_ERR_HIP);
  if (hbad) return sc.done(fail(SPGEMM_ERR_INPUT, "COO entry outside the %d x %d matrix", rows, cols));
  const int total = nnz + extra;
  CSR_ALLOC(&IA, sizeof(int) * ((size_t)rows + 1), true);
  CSR_HIP(hipMemsetAsync(IA, 0, sizeof(int) * ((size_t)rows + 1), s));
  if (total == 0) {
    CSR_ALLOC(&JA, sizeof(int), true);
    CSR_ALLOC(&A, sizeof(V), true);
    CSR_HIP(hipStreamSynchronize(s));
    *dIA = IA; *dJA = JA; *dA = A; *nnzOut = 0;
    return sc.done(SPGEMM_OK);
  }
  // (2) keys + stable sort over exactly the bits the shape needs; the sorted arrays are (keyA, idxA)
  CSR_ALLOC(&keyA, sizeof(unsigned long long) * (size_t)total);
  CSR_ALLOC(&keyB, sizeof(unsigned long long) * (size_t)total);
  CSR_ALLOC(&idxA, sizeof(int) * (size_t)total);
  CSR_ALLOC(&idxB, sizeof(int) * (size_t)total);
  CSR_ALLOC(&bhist, sizeof(int) * ((size_t)cdiv(total, RS_TILE) * RS_RADIX + 1));
  hipLaunchKernelGGL(k_make_keys<V>, grid256(std::max(nnz, loops ? rows : 0)), dim3(256), 0, s, nnz, rows, colBits, dRow, dCol,
                     dVal, missPos, loops ? miss : (int*)nullptr, keyA, idxA);
  radix_sort_bits(s, total, 0, keyBits, keyA, keyB, idxA, idxB, bhist, tile);
  CSR_HIP(hipGetLastError());
  // (3) heads of runs -> output positions
  CSR_ALLOC(&head, sizeof(int) * (size_t)total);
  CSR_ALLOC(&pos, sizeof(int) * ((size_t)total + 1));
  hipLaunchKernelGGL(k_heads, grid256(total), dim3(256), 0, s, total, keyA, dedupe, pos);
  CSR_HIP(hipMemcpyAsync(head, pos, sizeof(int) * (size_t)total, hipMemcpyDeviceToDevice, s));
  unsigned long long nheads = 0;
  CSR_HIP(scan_total(s, pos, total, tile, &nheads));
  const int outN = (int)nheads;
  // (4) emit columns / values / row counts, scan the counts, optional row normalisation
  CSR_ALLOC(&JA, sizeof(int) * (size_t)std::max(outN, 1), true);
  CSR_ALLOC(&A, sizeof(V) * (size_t)std::max(outN, 1), true);
  hipLaunchKernelGGL(k_emit<V>, grid256(total), dim3(256), 0, s, total, colBits, keyA, idxA, head, pos, dVal, nnz, dedupe,
                     (flags & SPGEMM_COO_ABS) ? 1 : 0, JA, A);
  hipLaunchKernelGGL(k_row_starts, grid256((long long)rows + 1), dim3(256), 0, s, rows, total, colBits, keyA, pos, IA);
  if ((flags & SPGEMM_COO_ROW_NORMALISE) && rows > 0)
    hipLaunchKernelGGL(k_row_normalise<V>, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, s, rows, IA, A);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  *dIA = IA; *dJA = JA; *dA = A; *nnzOut = outN;
  return sc.done(SPGEMM_OK);
}

}  // namespace coo

extern "C" int hip_coo_to_csr(spgemm_handle* h, int rows, int cols, int nnz, const int* dRow, const int* dCol,
                              const float* dVal, int flags, int** dIA, int** dJA, float** dA, int* nnzOut) {
  return coo::coo_to_csr<float>(h, rows, cols, nnz, dRow, dCol, dVal, flags, dIA, dJA, dA, nnzOut);
}

extern "C" int hip_coo_to_csr_f64(spgemm_handle* h, int rows, int cols, int nnz, const int* dRow, const int* dCol,
                                  const double* dVal, int flags, int** dIA, int** dJA, double** dA, int* nnzOut) {
  return coo::coo_to_csr<double>(h, rows, cols, nnz, dRow, dCol, dVal, flags, dIA, dJA, dA, nnzOut);
}

// ------------------------------------------------------------------------------------------------
// Workload statistics: the reference's 13-bucket power-of-two histogram of per-row flops
// (pushToStats / flopsStats, nlibs/tools/stats.cc:3-55): bucket i counts rows with 2^(i-1) < flops <= 2^i, bucket 0
// rows with flops <= 1, the last bucket everything above 2^11.  Row flops come from the path's own K1 kernel.
// ------------------------------------------------------------------------------------------------
namespace coo {
// val != nullptr: values themselves; otherwise differences of neighbours of `ptr` (row lengths of a CSR rowPtr)
__global__ void k_pow2_hist(int m, const int* __restrict__ val, const int* __restrict__ ptr, int nb,
                            int* __restrict__ hist /*[nb]*/) {
  __shared__ int sh[32];
  if (threadIdx.x < 32) sh[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) {
    const long long v = val ? (long long)val[i] : (long long)ptr[i + 1] - (long long)ptr[i];
    int b = nb - 1;
    for (int q = 0; q < nb - 1; ++q) if (v <= (1ll << q)) { b = q; break; }
    atomicAdd(&sh[b], 1);
  }
  __syncthreads();
  if (threadIdx.x < nb && sh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], sh[threadIdx.x]);
}
}  // namespace coo

extern "C" int hip_flopsStats(spgemm_handle* h, const int* dIA, const int* dJA, const int* dIB, int m,
                              int stats[SPGEMM_STATS_LEN]) {
  using namespace coo;
  if (!stats) return fail(SPGEMM_ERR_ARG, "stats is null");
  for (int i = 0; i < SPGEMM_STATS_LEN; ++i) stats[i] = 0;
  if (m < 0 || !dIA) return fail(SPGEMM_ERR_ARG, "bad argument");
  if (m == 0) return SPGEMM_OK;
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *flops = nullptr, *hist = nullptr;
  CSR_ALLOC(&flops, sizeof(int) * (size_t)m);
  CSR_ALLOC(&hist, sizeof(int) * SPGEMM_STATS_LEN);
  int rc = hip_csr_row_flops(h, dIA, dJA, dIB, m, flops, nullptr);
  if (rc) return sc.done(rc);
  if (hipMemsetAsync(hist, 0, sizeof(int) * SPGEMM_STATS_LEN, s) != hipSuccess) return sc.done(fail(SPGEMM_ERR_HIP, "memset failed"));
  hipLaunchKernelGGL(k_pow2_hist, grid256(m), dim3(256), 0, s, m, flops, (const int*)nullptr, SPGEMM_STATS_LEN, hist);
  if (hipMemcpyAsync(stats, hist, sizeof(int) * SPGEMM_STATS_LEN, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return sc.done(fail(SPGEMM_ERR_HIP, "flops statistics failed: %s", hipGetErrorString(hipGetLastError())));
  return sc.done(SPGEMM_OK);
}

// vector<int> CSR::nnzStats() (nlibs/CSR.cc:241-248): 18 power-of-two buckets of the ROW LENGTHS of a device CSR
extern "C" int hip_nnzStats(spgemm_handle* h, const int* dIA, int m, int stats[SPGEMM_NNZ_STATS_LEN]) {
  using namespace coo;
  if (!stats) return fail(SPGEMM_ERR_ARG, "stats is null");
  for (int i = 0; i < SPGEMM_NNZ_STATS_LEN; ++i) stats[i] = 0;
  if (m < 0 || !dIA) return fail(SPGEMM_ERR_ARG, "bad argument");
  if (m == 0) return SPGEMM_OK;
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int* hist = nullptr;
  CSR_ALLOC(&hist, sizeof(int) * SPGEMM_NNZ_STATS_LEN);
  if (hipMemsetAsync(hist, 0, sizeof(int) * SPGEMM_NNZ_STATS_LEN, s) != hipSuccess) return sc.done(fail(SPGEMM_ERR_HIP, "memset failed"));
  hipLaunchKernelGGL(k_pow2_hist, grid256(m), dim3(256), 0, s, m, (const int*)nullptr, dIA, SPGEMM_NNZ_STATS_LEN, hist);
  if (hipMemcpyAsync(stats, hist, sizeof(int) * SPGEMM_NNZ_STATS_LEN, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return sc.done(fail(SPGEMM_ERR_HIP, "row-length statistics failed: %s", hipGetErrorString(hipGetLastError())));
  return sc.done(SPGEMM_OK);
}

// ------------------------------------------------------------------------------------------------
// Per-bin correctness report: resultsComparison / isPartialRawEqual (mindex2-cuda/nGpuSpMM.cc:85-240) compare the GPU
// result hC with a CPU result rC bin by bin (rows of reference bin b sit at hqueue[hv[b]-1 .. hv[b+1]-1), flops.cu) so
// that a wrong kernel shows up as "its" bin.  Host arrays in (this is a checking aid, not a device path); rows are
// compared as sets of (column, value): row lengths, columns, values within `rel` relative (|x-y| <= rel*max(|x|,|y|)).
// ------------------------------------------------------------------------------------------------
extern "C" int hip_resultsComparison(int m, int n, const int* hIC, const int* hJC, const float* hC, const int* rIC,
                                     const int* rJC, const float* rC, const int hv[SPGEMM_HV_LEN], int hv_len,
                                     const int* hqueue, double rel, spgemm_bin_report report[SPGEMM_HV_LEN - 1]) {
  if (!hIC || !rIC || !hv || !hqueue || !report) return fail(SPGEMM_ERR_ARG, "null argument");
  if (m < 0 || n < 0 || hv_len < 2 || hv_len > SPGEMM_HV_LEN) return fail(SPGEMM_ERR_ARG, "bad size");
  std::vector<float> val((size_t)std::max(n, 1), 0.f);
  std::vector<int> stamp((size_t)std::max(n, 1), -1);
  for (int b = 0; b < SPGEMM_HV_LEN - 1; ++b) {
    spgemm_bin_report& R = report[b];
    R.rows = 0; R.rows_differ = 0; R.first_bad_row = -1; R.max_rel_err = 0.0;
    if (b + 1 >= hv_len) continue;
    const int lo = std::max(hv[b] - 1, 0), hi = hv[b + 1] - 1;      // element 0 of the (m+1)-long bin array is a dummy
    for (int q = lo; q < hi; ++q) {
      const int row = hqueue[q];
      if ((unsigned)row >= (unsigned)m) return fail(SPGEMM_ERR_INPUT, "queue entry %d is not a row", row);
      ++R.rows;
      bool bad = (hIC[row + 1] - hIC[row]) != (rIC[row + 1] - rIC[row]);
      for (int p = rIC[row]; p < rIC[row + 1]; ++p) {
        if ((unsigned)rJC[p] >= (unsigned)n) return fail(SPGEMM_ERR_INPUT, "column out of range in rC");
        stamp[rJC[p]] = row; val[rJC[p]] = rC[p];
      }
      for (int p = hIC[row]; p < hIC[row + 1]; ++p) {
        const int c = hJC[p];
        if ((unsigned)c >= (unsigned)n) return fail(SPGEMM_ERR_INPUT, "column out of range in hC");
        if (stamp[c] != row) { bad = true; continue; }
        const double x = hC[p], y = val[c];
        const double den = std::max(std::fabs(x), std::fabs(y));
        const double e = den > 0.0 ? std::fabs(x - y) / den : 0.0;
        if (e > R.max_rel_err) R.max_rel_err = e;
        if (e > rel) bad = true;
      }
      if (bad) { ++R.rows_differ; if (R.first_bad_row < 0) R.first_bad_row = row; }
    }
  }
  return SPGEMM_OK;
}
