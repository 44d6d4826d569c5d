// Dense matrix on the device: CSR -> dense, dense -> CSR, and the dense product C = A * B.
//
// Replaces, on device arrays,
//   DenseMatrix::DenseMatrix(const CSR&)      nlibs/DenseMatrix.h:6-21   (zero-fill, then values[i * cols + col] = val)
//   CSR::initWithDenseMatrix                  nlibs/CSR.h:54-82          (row-major walk, a cell skipped when val < 1e-8)
//   cblas_dgemm(RowMajor, NoTrans, NoTrans)   correctTests/dense-somp.cc (alpha 1, beta 0)
//
// A dense matrix is row-major with a leading dimension ld >= columns, in elements; every dense offset is 64-bit.
//
// CSR -> dense.  The target's [i][0..n) is zeroed once (one memset when ld == n, else a kernel that skips the padding).
// The validation pass of csr_common_device.hpp gets one more check queued on its flag: is every row strictly ascending?
// If so no two entries share a cell and the entries are scattered directly, dealt by entries (a 20 000-entry row is
// spread like any other 20 000 entries).  If not, key = (row << colBits) | col with the storage index as payload goes
// through the stable radix passes; equal keys then sit together in storage order and only the LAST of a run stores, so no
// two stores ever aim at one cell and the reference's sequential last-wins result comes out the same on every run.
//
// dense -> CSR.  Count, the library's scan, emit.  The unit of work is a SEGMENT: DS_SEG consecutive cells of one row
// (the last segment of a row is shorter); a row of n <= DS_SEG cells is one segment.  A wave takes one segment when
// n > DS_SEG and DS_SEG / n whole rows otherwise, and walks its cells 64 per step in row-major order: so 1 x 4 000 000 is
// 977 waves and 4 000 000 x 1 is 977 waves too.  The kept lanes of a step form a ballot; a lane's place is the count its
// segment has carried so far plus its rank among the ballot's lanes of the same segment (v_mbcnt), which keeps column
// order without LDS or barriers.  The scan runs over segments in row-major order and rowPtr[i] is the scan at row i's
// first segment.  A step's load is 64 consecutive cells (256 / 512 contiguous bytes per wave).
//
// Product.  One block of 4 waves per GM_BM x GM_BN tile of C; per GM_BK slice of K the block stages A (row-major, one
// element of padding per row) and B (k-major) in LDS, every wave then feeds a 64 x 64 part of the tile through
// v_mfma_f32_32x32x2_f32 (2 x 2 instruction tiles) or v_mfma_f64_16x16x4_f64 (4 x 4).  Edges are masked in the loads
// (anything outside m, n, k reads as +0.0) and in the stores.  Each C[i][j] lives in ONE accumulator over ascending k from
// +0.0: K is never split across waves or accumulators.
//
// Uses csr_common_device.hpp (Scratch, enter, the checks and their one read-back, row search, scan, radix sort).
#pragma once

namespace dense {

using namespace csrdev;

constexpr int NOT_ASCENDING = 1 << 8;              // a flag bit of this header, above csr_common_device.hpp's BAD_*
constexpr int DS_SEG = 4096;                       // cells of a dense -> CSR segment (tests/dense_ref.py: SEG)
constexpr int DS_WAVES = 4;                        // waves per block of the dense -> CSR kernel
constexpr int GM_BM = 128, GM_BN = 128, GM_BK = 32;   // block tile of the product (tests/dense_ref.py: BM, BN, BK)
constexpr int GM_THREADS = 256;

// ---- CSR -> dense ---------------------------------------------------------------------------------------------------------
// Reads rowPtr BEFORE it is known to be good: the searches only ever index rowPtr[0..m] and JA[0..nnz), whatever they hold.
__global__ __launch_bounds__(CP_THREADS) void k_check_ascending(int m, int nnz, const int* __restrict__ IA,
                                                                const int* __restrict__ JA, int* __restrict__ bad) {
  __shared__ int rows[2];
  const long long base = (long long)blockIdx.x * CP_TILE;
  tile_rows(IA, m, nnz, base, rows);
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const long long o = base + k * CP_THREADS + threadIdx.x;
    if (o >= nnz || o == 0) continue;
    const int row = row_of_entry(IA, rows[0], rows[1], (int)o);
    if (IA[row] != (int)o && JA[o - 1] >= JA[o]) atomicOr(bad, NOT_ASCENDING);
  }
}

// D[i][0..n) = +0.0 for ld > n: a block per 1024-cell piece of a row
template <class V>
__global__ __launch_bounds__(256) void k_zero_rows(long long pieces, int perRow, int n, V* __restrict__ D, long long ld) {
  for (long long p = blockIdx.x; p < pieces; p += gridDim.x) {
    const long long row = p / perRow;
    const int c0 = (int)(p - row * perRow) * 1024;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long c = (long long)c0 + k * 256 + threadIdx.x;
      if (c < n) D[row * ld + c] = V(0);
    }
  }
}

// every row strictly ascending: no two entries share a cell
template <class V>
__global__ __launch_bounds__(CP_THREADS) void k_scatter(int m, int nnz, const int* __restrict__ IA, const int* __restrict__ JA,
                                                        const V* __restrict__ A, V* __restrict__ D, long long ld) {
  __shared__ int rows[2];
  const long long base = (long long)blockIdx.x * CP_TILE;
  tile_rows(IA, m, nnz, base, rows);
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const long long o = base + k * CP_THREADS + threadIdx.x;
    if (o >= nnz) break;
    const int row = row_of_entry(IA, rows[0], rows[1], (int)o);
    D[(long long)row * ld + JA[o]] = A[o];
  }
}

__global__ __launch_bounds__(CP_THREADS) void k_cell_keys(int m, int nnz, int colBits, const int* __restrict__ IA,
                                                          const int* __restrict__ JA, unsigned long long* __restrict__ keys,
                                                          int* __restrict__ payload) {
  __shared__ int rows[2];
  const long long base = (long long)blockIdx.x * CP_TILE;
  tile_rows(IA, m, nnz, base, rows);
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const long long o = base + k * CP_THREADS + threadIdx.x;
    if (o >= nnz) break;
    const int row = row_of_entry(IA, rows[0], rows[1], (int)o);
    keys[o] = (((unsigned long long)(unsigned)row) << colBits) | (unsigned)JA[o];
    payload[o] = (int)o;
  }
}

// the last of every run of equal keys writes its cell
template <class V>
__global__ void k_scatter_last(int nnz, int colBits, const unsigned long long* __restrict__ keys, const int* __restrict__ idx,
                               const V* __restrict__ A, V* __restrict__ D, long long ld) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const unsigned long long key = keys[i];
  if (i + 1 < nnz && keys[i + 1] == key) return;
  D[(long long)(key >> colBits) * ld + (long long)(key & ((1ull << colBits) - 1ull))] = A[idx[i]];
}

static int check_dense_args(int m, int n, const void* dD, long long ld) {
  if (m < 0 || n < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (ld < n) return fail(SPGEMM_ERR_ARG, "ld=%lld is below the %d columns", ld, n);
  if (m > 0 && n > 0 && !dD) return fail(SPGEMM_ERR_ARG, "dense array null with m=%d n=%d", m, n);
  return SPGEMM_OK;
}

template <class V>
static int to_dense(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, V* dD, long long ld) {
  CHK(check_csr_args(m, n, nnz, dIA, dJA, dA));
  CHK(check_dense_args(m, n, dD, ld));
  const int rowBits = bits_of(m - 1), colBits = bits_of(n - 1);
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  // validation, one read-back: rowPtr, the column range (both become addresses into dD), and whether rows ascend
  int* bad = nullptr;
  int hbad = 0;
  if (int rc = flag_begin(sc, s, &bad)) return sc.done(rc);
  queue_csr_checks(s, m, n, nnz, dIA, dJA, bad);
  if (nnz > 0) hipLaunchKernelGGL(k_check_ascending, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, dIA, dJA, bad);
  if (int rc = read_flag(s, bad, &hbad)) return sc.done(rc);
  if (hbad & BAD_ROWPTR) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer ending at nnz=%d", nnz));
  if (hbad & BAD_COLUMN) return sc.done(fail(SPGEMM_ERR_INPUT, "column outside [0,%d)", n));
  if (m == 0 || n == 0) return sc.done(SPGEMM_OK);
  if (ld == n) {
    CSR_HIP(hipMemsetAsync(dD, 0, sizeof(V) * (size_t)m * (size_t)n, s));
  } else {
    const int perRow = cdiv(n, 1024);
    const long long pieces = (long long)m * perRow;
    hipLaunchKernelGGL(k_zero_rows<V>, dim3((unsigned)std::min<long long>(pieces, 1 << 20)), dim3(256), 0, s, pieces, perRow, n, dD, ld);
  }
  if (nnz > 0 && !(hbad & NOT_ASCENDING)) {
    hipLaunchKernelGGL(k_scatter<V>, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, dIA, dJA, dA, dD, ld);
  } else if (nnz > 0) {
    int *idxA = nullptr, *idxB = nullptr, *bhist = nullptr;
    unsigned long long *keyA = nullptr, *keyB = nullptr, *tile = nullptr;
    const int nblk = cdiv(nnz, RS_TILE);
    CSR_ALLOC(&keyA, sizeof(unsigned long long) * (size_t)nnz);
    CSR_ALLOC(&keyB, sizeof(unsigned long long) * (size_t)nnz);
    CSR_ALLOC(&idxA, sizeof(int) * (size_t)nnz);
    CSR_ALLOC(&idxB, sizeof(int) * (size_t)nnz);
    CSR_ALLOC(&bhist, sizeof(int) * ((size_t)nblk * RS_RADIX + 1));
    CSR_ALLOC(&tile, scan_scratch_bytes((long long)nblk * RS_RADIX + 1));
    hipLaunchKernelGGL(k_cell_keys, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, colBits, dIA, dJA, keyA, idxA);
    radix_sort_bits(s, nnz, 0, rowBits + colBits, keyA, keyB, idxA, idxB, bhist, tile);
    hipLaunchKernelGGL(k_scatter_last<V>, grid256(nnz), dim3(256), 0, s, nnz, colBits, keyA, idxA, dA, dD, ld);
  }
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  return sc.done(SPGEMM_OK);
}

// ---- dense -> CSR ---------------------------------------------------------------------------------------------------------
template <class V>
__device__ __forceinline__ bool keeps(V v, int rule, double tol) {
  return rule == SPGEMM_DENSE_KEEP_REFERENCE ? !((double)v < tol) : fabs((double)v) > tol;
}

// A wave's `group` segments (group > 1 only when a row is one segment of n cells), cells 64 per step in row-major order.
// EMIT = false: cnt[segment] = its kept cells.  EMIT = true: cnt is the scanned array, the kept cells go to JC / C.
template <class V, bool EMIT>
__global__ __launch_bounds__(DS_WAVES * 64) void k_segments(long long nseg, int perRow, int group, int n,
                                                            const V* __restrict__ D, long long ld, int rule, double tol,
                                                            int* __restrict__ cnt, int* __restrict__ JC, V* __restrict__ C) {
  const long long first = ((long long)blockIdx.x * DS_WAVES + (threadIdx.x >> 6)) * group;
  if (first >= nseg) return;                                   // the whole wave
  const int lane = lane_id();
  const int here = nseg - first < group ? (int)(nseg - first) : group;
  int len, total;                                              // nominal cells per segment; cells of this wave
  if (perRow == 1) { len = n; total = here * n; }              // here * n <= DS_SEG
  else { len = DS_SEG; total = n - (int)(first % perRow) * DS_SEG; total = total < DS_SEG ? total : DS_SEG; }
  int carry = 0;                                               // kept cells of the segment that is open when a step begins
  for (int fb = 0; fb < total; fb += 64) {
    const int f = fb + lane;
    const bool valid = f < total;
    const int sidx = valid ? f / len : 0, c = f - sidx * len;
    const long long seg = first + sidx;
    const long long row = perRow == 1 ? seg : seg / perRow;
    const int col = perRow == 1 ? c : (int)(seg - row * perRow) * DS_SEG + c;
    V v = V(0);
    bool keep = false;
    if (valid) {
      v = D[row * ld + col];
      keep = keeps<V>(v, rule, tol);
    }
    const unsigned long long mk = ballot64(keep);
    const int start = sidx * len - fb;                         // lane where this lane's segment begins (< 0: an earlier step)
    const unsigned long long mine = mk & (~0ull << (start > 0 ? start : 0));
    const int before = mask_rank(mine) + (start < 0 ? carry : 0);
    if constexpr (EMIT) {
      if (keep) {
        const long long o = (long long)cnt[seg] + before;
        JC[o] = col;
        C[o] = v;
      }
    } else {
      if (valid && (c == len - 1 || f == total - 1)) cnt[seg] = before + (keep ? 1 : 0);
    }
    const int last = (fb + 63) / len * len - fb;               // the same for lane 63: what the next step inherits
    carry = __popcll(mk & (~0ull << (last > 0 ? last : 0))) + (last < 0 ? carry : 0);
  }
}

__global__ void k_row_starts(int m, int perRow, const int* __restrict__ segScan, long long nseg, int* __restrict__ IC) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= m) IC[i] = segScan[i < m ? (long long)i * perRow : nseg];
}

template <class V>
static int to_csr(spgemm_handle* h, int m, int n, const V* dD, long long ld, int rule, double tol, int** dIC, int** dJC,
                  V** dC, int* nnzC) {
  if (!dIC || !dJC || !dC || !nnzC) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIC = nullptr; *dJC = nullptr; *dC = nullptr; *nnzC = 0;
  CHK(check_dense_args(m, n, dD, ld));
  if (rule != SPGEMM_DENSE_KEEP_REFERENCE && rule != SPGEMM_DENSE_KEEP_ABS) return fail(SPGEMM_ERR_ARG, "rule=%d is neither 0 nor 1", rule);
  if (!(tol >= 0.0)) return fail(SPGEMM_ERR_ARG, "tol=%g is negative or NaN", tol);
  const int perRow = std::max(1, cdiv(n, DS_SEG));
  const long long nseg = (long long)m * perRow;
  if (nseg >= INT_MAX) return fail(SPGEMM_ERR_OVERFLOW, "%lld segments do not fit the int32 scan", nseg);
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *IC = nullptr, *JC = nullptr, *segScan = nullptr;
  V* C = nullptr;
  unsigned long long* tile = nullptr;
  CSR_ALLOC(&IC, sizeof(int) * ((size_t)m + 1), true);
  if (m == 0 || n == 0) {
    CSR_ALLOC(&JC, sizeof(int), true);
    CSR_ALLOC(&C, sizeof(V), true);
    CSR_HIP(hipMemsetAsync(IC, 0, sizeof(int) * ((size_t)m + 1), s));
    CSR_HIP(hipStreamSynchronize(s));
    *dIC = IC; *dJC = JC; *dC = C;
    return sc.done(SPGEMM_OK);
  }
  if (perRow == 1) segScan = IC;                               // one segment per row: the scan is rowPtr
  else CSR_ALLOC(&segScan, sizeof(int) * ((size_t)nseg + 1));
  CSR_ALLOC(&tile, scan_scratch_bytes(nseg + 1));
  const int group = perRow == 1 ? std::max(1, DS_SEG / n) : 1;
  const dim3 grid((unsigned)cdiv(cdiv(nseg, group), DS_WAVES)), block(DS_WAVES * 64);
  hipLaunchKernelGGL((k_segments<V, false>), grid, block, 0, s, nseg, perRow, group, n, dD, ld, rule, tol, segScan, (int*)nullptr, (V*)nullptr);
  unsigned long long total = 0;
  CSR_HIP(scan_total(s, segScan, (int)nseg, tile, &total));
  if (total > (unsigned long long)INT_MAX)
    return sc.done(fail(SPGEMM_ERR_OVERFLOW, "%llu kept cells do not fit the int32 CSR", total));
  CSR_ALLOC(&JC, sizeof(int) * (size_t)std::max<unsigned long long>(total, 1), true);
  CSR_ALLOC(&C, sizeof(V) * (size_t)std::max<unsigned long long>(total, 1), true);
  if (total > 0)
    hipLaunchKernelGGL((k_segments<V, true>), grid, block, 0, s, nseg, perRow, group, n, dD, ld, rule, tol, segScan, JC, C);
  if (perRow > 1) hipLaunchKernelGGL(k_row_starts, grid256((long long)m + 1), dim3(256), 0, s, m, perRow, segScan, nseg, IC);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  *dIC = IC; *dJC = JC; *dC = C; *nnzC = (int)total;
  return sc.done(SPGEMM_OK);
}

// ---- the product ----------------------------------------------------------------------------------------------------------
typedef float gm_f32x16 __attribute__((ext_vector_type(16)));
typedef double gm_f64x4 __attribute__((ext_vector_type(4)));

// One MFMA shape per value type.  T: side of the instruction's C tile; KS: k per instruction; lane l holds
// A[l % T][l / T] and B[l / T][l % T]; row_of(reg, lane) / lane % T is where accumulator register `reg` lands in the tile.
template <class V> struct Mma;
template <> struct Mma<float> {
  static constexpr int T = 32, KS = 2, REGS = 16;
  using Acc = gm_f32x16;
  static __device__ __forceinline__ Acc fma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row_of(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
};
template <> struct Mma<double> {
  static constexpr int T = 16, KS = 4, REGS = 4;
  using Acc = gm_f64x4;
  static __device__ __forceinline__ Acc fma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int row_of(int reg, int lane) { return (lane >> 4) + 4 * reg; }
};

template <class V>
__global__ __launch_bounds__(GM_THREADS) void k_gemm(int m, int n, int k, int bm, int bn, const V* __restrict__ A, long long lda,
                                                     const V* __restrict__ B, long long ldb, V* __restrict__ C, long long ldc) {
  using M = Mma<V>;
  constexpr int WT = 64 / M::T;                                // instruction tiles per side of a wave's 64 x 64 part
  __shared__ V As[GM_BM][GM_BK + 1];
  __shared__ V Bs[GM_BK][GM_BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int lr = lane % M::T, lk = lane / M::T;
  for (int by = blockIdx.y; by < bm; by += gridDim.y) {
    for (int bx = blockIdx.x; bx < bn; bx += gridDim.x) {
      const long long row0 = (long long)by * GM_BM, col0 = (long long)bx * GM_BN;
      typename M::Acc acc[WT][WT];
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j)
#pragma unroll
          for (int r = 0; r < M::REGS; ++r) acc[i][j][r] = V(0);
      for (long long k0 = 0; k0 < k; k0 += GM_BK) {
        // A: 32 consecutive k of one row per half wave; B: 128 consecutive columns of one k per two waves
#pragma unroll
        for (int i = 0; i < GM_BM * GM_BK / GM_THREADS; ++i) {
          const int r = (tid >> 5) + (GM_THREADS / GM_BK) * i, kk = tid & (GM_BK - 1);
          const long long gr = row0 + r, gk = k0 + kk;
          As[r][kk] = (gr < m && gk < k) ? A[gr * lda + gk] : V(0);
        }
#pragma unroll
        for (int i = 0; i < GM_BK * GM_BN / GM_THREADS; ++i) {
          const int kk = (tid >> 7) + (GM_THREADS / GM_BN) * i, c = tid & (GM_BN - 1);
          const long long gk = k0 + kk, gc = col0 + c;
          Bs[kk][c] = (gk < k && gc < n) ? B[gk * ldb + gc] : V(0);
        }
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < GM_BK; ks += M::KS) {
          V a[WT], b[WT];
#pragma unroll
          for (int i = 0; i < WT; ++i) a[i] = As[wm + i * M::T + lr][ks + lk];
#pragma unroll
          for (int j = 0; j < WT; ++j) b[j] = Bs[ks + lk][wn + j * M::T + lr];
#pragma unroll
          for (int i = 0; i < WT; ++i)
#pragma unroll
            for (int j = 0; j < WT; ++j) acc[i][j] = M::fma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
      }
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j)
#pragma unroll
          for (int r = 0; r < M::REGS; ++r) {
            const long long gr = row0 + wm + i * M::T + M::row_of(r, lane), gc = col0 + wn + j * M::T + lr;
            if (gr < m && gc < n) C[gr * ldc + gc] = acc[i][j][r];
          }
    }
  }
}

// [p, p + bytes of rows x cols with leading dimension ld): the address range a dense argument spans
template <class V>
static bool ranges_overlap(const V* a, int ra, int ca, long long lda, const V* b, int rb, int cb, long long ldb) {
  if (ra == 0 || ca == 0 || rb == 0 || cb == 0) return false;
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + sizeof(V) * ((size_t)(ra - 1) * (size_t)lda + (size_t)ca);
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + sizeof(V) * ((size_t)(rb - 1) * (size_t)ldb + (size_t)cb);
  return a0 < b1 && b0 < a1;
}

template <class V>
static int gemm(spgemm_handle* h, int m, int n, int k, const V* dA, long long lda, const V* dB, long long ldb, V* dC, long long ldc) {
  if (m < 0 || n < 0 || k < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  CHK(check_dense_args(m, k, dA, lda));
  CHK(check_dense_args(k, n, dB, ldb));
  CHK(check_dense_args(m, n, dC, ldc));
  if (ranges_overlap(dC, m, n, ldc, dA, m, k, lda) || ranges_overlap(dC, m, n, ldc, dB, k, n, ldb))
    return fail(SPGEMM_ERR_ARG, "C overlaps A or B");
  hipStream_t s;
  CHK(enter(h, &s));
  if (m == 0 || n == 0) return SPGEMM_OK;
  const int bm = cdiv(m, GM_BM), bn = cdiv(n, GM_BN);
  hipLaunchKernelGGL(k_gemm<V>, dim3((unsigned)std::min(bn, 1 << 16), (unsigned)std::min(bm, 65535)), dim3(GM_THREADS), 0, s, m, n, k,
                     bm, bn, dA, lda, dB, ldb, dC, ldc);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  return SPGEMM_OK;
}

}  // namespace dense

extern "C" int hip_csr_to_dense(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                                float* dD, long long ld) {
  return dense::to_dense<float>(h, m, n, nnz, dIA, dJA, dA, dD, ld);
}

extern "C" int hip_csr_to_dense_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                                    double* dD, long long ld) {
  return dense::to_dense<double>(h, m, n, nnz, dIA, dJA, dA, dD, ld);
}

extern "C" int hip_dense_to_csr(spgemm_handle* h, int m, int n, const float* dD, long long ld, int rule, double tol,
                                int** dIC, int** dJC, float** dC, int* nnzC) {
  return dense::to_csr<float>(h, m, n, dD, ld, rule, tol, dIC, dJC, dC, nnzC);
}

extern "C" int hip_dense_to_csr_f64(spgemm_handle* h, int m, int n, const double* dD, long long ld, int rule, double tol,
                                    int** dIC, int** dJC, double** dC, int* nnzC) {
  return dense::to_csr<double>(h, m, n, dD, ld, rule, tol, dIC, dJC, dC, nnzC);
}

extern "C" int hip_dense_gemm(spgemm_handle* h, int m, int n, int k, const float* dA, long long lda, const float* dB,
                              long long ldb, float* dC, long long ldc) {
  return dense::gemm<float>(h, m, n, k, dA, lda, dB, ldb, dC, ldc);
}

extern "C" int hip_dense_gemm_f64(spgemm_handle* h, int m, int n, int k, const double* dA, long long lda, const double* dB,
                                  long long ldb, double* dC, long long ldc) {
  return dense::gemm<double>(h, m, n, k, dA, lda, dB, ldb, dC, ldc);
}
