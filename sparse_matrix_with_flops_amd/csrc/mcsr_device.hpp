// Mixed CSR (MCSR) on the device: the top-left blockRows x blockCols corner as r x c dense tiles, the rest as a CSR; and
// the two parts written back out as one CSR.
//
// Replaces, on device arrays,
//   MCSR::MCSR(const CSR&, r, c, blockRows, blockCols)   nlibs/MCSR.cc:3-97   (the FILL pass, lines 58-92, is the
//                                                                              definition; see below for the count pass)
// and defines the inverse, which the reference lacks (there is no MCSR::isEqual).
//
// Layout.  An entry (i, col) with i < blockRows and col < blockCols belongs to the corner: tile (i / r, col / c), cell
// (i % r) * c + col % c of a BCSR with bm = blockRows / r block rows and bn = ceil(blockCols / c) block columns -- exactly
// what bcsr::to_bcsr makes of the blockRows x blockCols CSR of those entries in A's storage order.  Everything else is the
// remainder, an m x n CSR with global columns: row i < blockRows keeps its entries with col >= blockCols in storage order,
// row i >= blockRows is A's row.
//
// The reference's COUNT pass (nlibs/MCSR.cc:16-40) resets `top` per block row, not per row, so for r > 1 its remainder
// rowPtr over-counts whenever a row other than the last of its block row has remainder entries, and assert(nnz == top)
// fails.  That defect is not reproduced: the remainder rowPtr here is the one the fill pass implies.
//
// Forward.  A CSR is in row order, so ONE stable two-way partition of the first nTop = IA[blockRows] entries by the flag
// col < blockCols yields both parts in CSR order; no sort, no per-row work:
//   * k_flags, dealt by entries, then the library's scan: scan[o] = corner entries before o, scan[nTop] = nCorner;
//   * k_scatter, dealt by entries (coalesced reads): a corner entry goes to scan[o] of the temporary corner CSR (its column
//     is local already), a remainder entry to o - scan[o];
//   * entries nTop..nnz are copied in bulk behind the remainder's top part;
//   * k_rowptrs: corner rowPtr[i] = scan[IA[i]], remainder rowPtr[i] = IA[i] - scan[IA[i]] up to blockRows, IA[i] - nCorner
//     above;
//   * bcsr::to_bcsr on the temporary corner CSR, which goes back to the pool before the call returns.
// A 20 000-entry row is spread over blocks like any other 20 000 entries.  No atomics on values; every position is a
// function of the input alone, so the result is the same bytes every time.
//
// Inverse.  bcsr::to_csr on the corner (m = blockRows, n = blockCols: a temporary CSR), then a row-wise concatenation with
// the remainder: row lengths added, the library's scan (its 64-bit total decides the overflow), one copy kernel dealt by
// OUTPUT entries (tile_copy).
//
// Every value that becomes an address (rowPtr, the columns, the block rowPtr and columns) is checked first by
// k_check_rowptr / k_check_cols (here or inside the calls into bcsr_device.hpp); the host reads the flag before anything
// is queued that indexes with them.  Uses csr_common_device.hpp (the checks and their one read-back, scan, tile copy,
// Scratch) and bcsr_device.hpp.
#pragma once

namespace mcsr {

using namespace csrdev;

// flag[o] = 1 where entry o < nTop lies left of blockCols (its row is above blockRows by the choice of nTop)
__global__ __launch_bounds__(CP_THREADS) void k_flags(int nTop, int blockCols, const int* __restrict__ JA,
                                                      int* __restrict__ flag) {
  const long long base = (long long)blockIdx.x * CP_TILE;
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const long long o = base + k * CP_THREADS + threadIdx.x;
    if (o >= nTop) break;
    flag[o] = JA[o] < blockCols ? 1 : 0;
  }
}

// the stable partition: scan[o] corner entries precede entry o, so o - scan[o] remainder entries do
template <class V>
__global__ __launch_bounds__(CP_THREADS) void k_scatter(int nTop, int blockCols, const int* __restrict__ JA,
                                                        const V* __restrict__ A, const int* __restrict__ scan,
                                                        int* __restrict__ JK, V* __restrict__ K, int* __restrict__ JR,
                                                        V* __restrict__ R) {
  const long long base = (long long)blockIdx.x * CP_TILE;
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const long long o = base + k * CP_THREADS + threadIdx.x;
    if (o >= nTop) break;
    const int col = JA[o], before = scan[o];
    const V v = A[o];
    if (col < blockCols) { JK[before] = col; K[before] = v; }
    else { const int p = (int)o - before; JR[p] = col; R[p] = v; }
  }
}

// IK[i] (i = 0..blockRows): the corner CSR's rowPtr; IR[i] (i = 0..m): the remainder's.  IA has been validated, so
// IA[i] <= nTop for i <= blockRows.
__global__ void k_rowptrs(int m, int blockRows, int nCorner, const int* __restrict__ IA, const int* __restrict__ scan,
                          int* __restrict__ IK, int* __restrict__ IR) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > m) return;
  const int a = IA[i];
  if (i <= blockRows) {
    const int before = scan[a];
    IK[i] = before;
    IR[i] = a - before;
  } else {
    IR[i] = a - nCorner;
  }
}

// ---- inverse ------------------------------------------------------------------------------------------------------------
// IC[i] = corner row length (i < blockRows) + remainder row length, as an unsigned sum (each is below 2^31; the scan
// adds unsigned into a 64-bit total)
__global__ void k_cat_lens(int m, int blockRows, const int* __restrict__ IT, const int* __restrict__ IR,
                           int* __restrict__ IC) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  unsigned len = (unsigned)(IR[i + 1] - IR[i]);
  if (i < blockRows) len += (unsigned)(IT[i + 1] - IT[i]);
  IC[i] = (int)len;
}

// One tile of C's entries per block (tile_copy): the corner's row first and the remainder's behind it.  The corner sits
// at the top left, so its columns are global already.
template <class V>
__global__ __launch_bounds__(CP_THREADS) void k_cat_copy(int m, int nnz, int blockRows, const int* __restrict__ IT,
                                                         const int* __restrict__ JT, const V* __restrict__ T,
                                                         const int* __restrict__ IR, const int* __restrict__ JR,
                                                         const V* __restrict__ R, const int* __restrict__ IC,
                                                         int* __restrict__ JC, V* __restrict__ C) {
  tile_copy<V>(m, nnz, IC, JC, C, [&](int r, int off, int& col, V& val) {
    int s = 0, len = 0;
    if (r < blockRows) { s = IT[r]; len = IT[r + 1] - s; }
    if (off < len) {
      col = JT[s + off];
      val = T[s + off];
    } else {
      const int p = IR[r] + (off - len);
      col = JR[p];
      val = R[p];
    }
  });
}

static int check_corner(int m, int n, int r, int c, int blockRows, int blockCols) {
  CHK(bcsr::check_tile_shape(r, c));
  if (m < 0 || n < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (blockRows < 0 || blockRows > m || blockCols < 0 || blockCols > n)
    return fail(SPGEMM_ERR_ARG, "corner %d x %d outside the %d x %d matrix", blockRows, blockCols, m, n);
  if (blockRows % r != 0)                          // the reference's assert, nlibs/MCSR.cc:15
    return fail(SPGEMM_ERR_ARG, "blockRows=%d is not a multiple of r=%d", blockRows, r);
  return SPGEMM_OK;
}

template <class V>
static int to_mcsr(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, int r, int c,
                   int blockRows, int blockCols, int** dIB, int** dJB, V** dB, int* nnzb, int** dIR, int** dJR, V** dR,
                   int* nnzR) {
  if (!dIB || !dJB || !dB || !nnzb || !dIR || !dJR || !dR || !nnzR) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIB = nullptr; *dJB = nullptr; *dB = nullptr; *nnzb = 0;
  *dIR = nullptr; *dJR = nullptr; *dR = nullptr; *nnzR = 0;
  if (nnz < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  CHK(check_corner(m, n, r, c, blockRows, blockCols));
  CHK(check_csr_args(m, n, nnz, dIA, dJA, dA));
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *bad = nullptr, *scan = nullptr, *IK = nullptr, *JK = nullptr, *IR = nullptr, *JR = nullptr;
  V *K = nullptr, *R = nullptr;
  unsigned long long* tile = nullptr;
  // validation, one read-back: rowPtr (IA[blockRows] cuts the entries, scan is indexed with IA) and the column range
  if (int rc = flag_begin(sc, s, &bad)) return sc.done(rc);
  queue_csr_checks(s, m, n, nnz, dIA, dJA, bad);
  int hbad = 0, nTop = 0;
  if (blockRows > 0) CSR_HIP(hipMemcpyAsync(&nTop, dIA + blockRows, sizeof(int), hipMemcpyDeviceToHost, s));
  if (read_flag(s, bad, &hbad)) return sc.done(SPGEMM_ERR_HIP);
  if (hbad & BAD_ROWPTR) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer ending at nnz=%d", nnz));
  if (hbad & BAD_COLUMN) return sc.done(fail(SPGEMM_ERR_INPUT, "column outside [0,%d)", n));
  // (1) the flags of the top entries and their scan; its total sizes the two parts
  CSR_ALLOC(&scan, sizeof(int) * ((size_t)nTop + 1));
  CSR_ALLOC(&tile, scan_scratch_bytes((long long)nTop + 1));
  const dim3 topGrid((unsigned)std::max(1, cdiv(nTop, CP_TILE)));
  if (nTop > 0) hipLaunchKernelGGL(k_flags, topGrid, dim3(CP_THREADS), 0, s, nTop, blockCols, dJA, scan);
  scan_inplace(s, scan, nTop, tile);
  int nCorner = 0;
  CSR_HIP(hipMemcpyAsync(&nCorner, scan + nTop, sizeof(int), hipMemcpyDeviceToHost, s));
  CSR_HIP(hipStreamSynchronize(s));
  const int nRest = nnz - nCorner;
  CSR_ALLOC(&IK, sizeof(int) * ((size_t)blockRows + 1));
  CSR_ALLOC(&JK, sizeof(int) * (size_t)std::max(nCorner, 1));
  CSR_ALLOC(&K, sizeof(V) * (size_t)std::max(nCorner, 1));
  CSR_ALLOC(&IR, sizeof(int) * ((size_t)m + 1), true);
  CSR_ALLOC(&JR, sizeof(int) * (size_t)std::max(nRest, 1), true);
  CSR_ALLOC(&R, sizeof(V) * (size_t)std::max(nRest, 1), true);
  // (2) the partition of the top entries, the bulk copy of the rest, the two rowPtr arrays
  if (nTop > 0) hipLaunchKernelGGL(k_scatter<V>, topGrid, dim3(CP_THREADS), 0, s, nTop, blockCols, dJA, dA, scan, JK, K, JR, R);
  if (nnz > nTop) {
    const size_t cnt = (size_t)(nnz - nTop), at = (size_t)(nTop - nCorner);
    CSR_HIP(hipMemcpyAsync(JR + at, dJA + nTop, sizeof(int) * cnt, hipMemcpyDeviceToDevice, s));
    CSR_HIP(hipMemcpyAsync(R + at, dA + nTop, sizeof(V) * cnt, hipMemcpyDeviceToDevice, s));
  }
  if (m > 0) hipLaunchKernelGGL(k_rowptrs, grid256((long long)m + 1), dim3(256), 0, s, m, blockRows, nCorner, dIA, scan, IK, IR);
  else CSR_HIP(hipMemsetAsync(IR, 0, sizeof(int), s));
  CSR_HIP(hipGetLastError());
  // (3) the corner CSR (blockRows x blockCols, local columns) as tiles; on the same stream, it returns after its work
  const int rc = bcsr::to_bcsr<V>(h, blockRows, blockCols, nCorner, IK, JK, K, r, c, dIB, dJB, dB, nnzb);
  if (rc != SPGEMM_OK) {
    hipStreamSynchronize(s);
    return sc.done(rc);
  }
  *dIR = IR; *dJR = JR; *dR = R; *nnzR = nRest;
  return sc.done(SPGEMM_OK);
}

template <class V>
static int to_csr(spgemm_handle* h, int m, int n, int r, int c, int blockRows, int blockCols, int nnzb, const int* dIB,
                  const int* dJB, const V* dB, int nnzR, const int* dIR, const int* dJR, const V* dR, double drop_tol,
                  int** dIC, int** dJC, V** dC, int* nnzC) {
  if (!dIC || !dJC || !dC || !nnzC) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIC = nullptr; *dJC = nullptr; *dC = nullptr; *nnzC = 0;
  if (nnzb < 0 || nnzR < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  CHK(check_corner(m, n, r, c, blockRows, blockCols));
  if (!(drop_tol >= 0.0)) return fail(SPGEMM_ERR_ARG, "drop_tol=%g is negative or NaN", drop_tol);
  if ((blockRows > 0 && !dIB) || (nnzb > 0 && (!dJB || !dB)))
    return fail(SPGEMM_ERR_ARG, "BCSR arrays null with blockRows=%d nnzb=%d", blockRows, nnzb);
  if (blockRows == 0 && nnzb > 0) return fail(SPGEMM_ERR_ARG, "nnzb=%d in a corner without rows", nnzb);
  CHK(check_csr_args(m, n, nnzR, dIR, dJR, dR));
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *IT = nullptr, *JT = nullptr, *IC = nullptr, *JC = nullptr;
  V *T = nullptr, *C = nullptr;
  unsigned long long* tile = nullptr;
  // validation, one read-back: the remainder's rowPtr against its count and its columns (the result must be a valid m x n
  // CSR); the block rowPtr and the block columns are validated by bcsr::to_csr
  int hbad = 0;
  if (int rc = validate_csr(sc, s, m, n, nnzR, dIR, dJR, &hbad)) return sc.done(rc);
  if (hbad & BAD_ROWPTR) return sc.done(fail(SPGEMM_ERR_INPUT, "the remainder's rowPtr is not a monotone row pointer ending at nnz=%d", nnzR));
  if (hbad & BAD_COLUMN) return sc.done(fail(SPGEMM_ERR_INPUT, "a remainder column is outside [0,%d)", n));
  // (1) the corner's rows as a temporary CSR
  int nnzT = 0;
  const int rc = bcsr::to_csr<V>(h, blockRows, blockCols, r, c, nnzb, dIB, dJB, dB, drop_tol, &IT, &JT, &T, &nnzT);
  if (rc != SPGEMM_OK) return sc.done(rc);
  sc.tmp.push_back(IT); sc.tmp.push_back(JT); sc.tmp.push_back(T);
  // (2) row lengths, scan, copy
  CSR_ALLOC(&IC, sizeof(int) * ((size_t)m + 1), true);
  CSR_ALLOC(&tile, scan_scratch_bytes((long long)m + 1));
  if (m > 0) hipLaunchKernelGGL(k_cat_lens, grid256(m), dim3(256), 0, s, m, blockRows, IT, dIR, IC);
  unsigned long long total = 0;
  CSR_HIP(scan_total(s, IC, m, tile, &total));
  if (total > (unsigned long long)INT_MAX)
    return sc.done(fail(SPGEMM_ERR_OVERFLOW, "%llu entries do not fit the int32 CSR", total));
  const int nnz = (int)total;
  CSR_ALLOC(&JC, sizeof(int) * (size_t)std::max(nnz, 1), true);
  CSR_ALLOC(&C, sizeof(V) * (size_t)std::max(nnz, 1), true);
  if (nnz > 0)
    hipLaunchKernelGGL(k_cat_copy<V>, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, blockRows, IT, JT, T,
                       dIR, dJR, dR, IC, JC, C);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  *dIC = IC; *dJC = JC; *dC = C; *nnzC = nnz;
  return sc.done(SPGEMM_OK);
}

}  // namespace mcsr

extern "C" int hip_csr_to_mcsr(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA, int r,
                               int c, int blockRows, int blockCols, int** dIB, int** dJB, float** dB, int* nnzb, int** dIR,
                               int** dJR, float** dR, int* nnzR) {
  return mcsr::to_mcsr<float>(h, m, n, nnz, dIA, dJA, dA, r, c, blockRows, blockCols, dIB, dJB, dB, nnzb, dIR, dJR, dR, nnzR);
}

extern "C" int hip_csr_to_mcsr_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                                   int r, int c, int blockRows, int blockCols, int** dIB, int** dJB, double** dB, int* nnzb,
                                   int** dIR, int** dJR, double** dR, int* nnzR) {
  return mcsr::to_mcsr<double>(h, m, n, nnz, dIA, dJA, dA, r, c, blockRows, blockCols, dIB, dJB, dB, nnzb, dIR, dJR, dR, nnzR);
}

extern "C" int hip_mcsr_to_csr(spgemm_handle* h, int m, int n, int r, int c, int blockRows, int blockCols, int nnzb,
                               const int* dIB, const int* dJB, const float* dB, int nnzR, const int* dIR, const int* dJR,
                               const float* dR, double drop_tol, int** dIC, int** dJC, float** dC, int* nnzC) {
  return mcsr::to_csr<float>(h, m, n, r, c, blockRows, blockCols, nnzb, dIB, dJB, dB, nnzR, dIR, dJR, dR, drop_tol, dIC, dJC,
                             dC, nnzC);
}

extern "C" int hip_mcsr_to_csr_f64(spgemm_handle* h, int m, int n, int r, int c, int blockRows, int blockCols, int nnzb,
                                   const int* dIB, const int* dJB, const double* dB, int nnzR, const int* dIR, const int* dJR,
                                   const double* dR, double drop_tol, int** dIC, int** dJC, double** dC, int* nnzC) {
  return mcsr::to_csr<double>(h, m, n, r, c, blockRows, blockCols, nnzb, dIB, dJB, dB, nnzR, dIR, dJR, dR, drop_tol, dIC, dJC,
                              dC, nnzC);
}
