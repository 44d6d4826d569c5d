// Blocked CSR (BCSR) on the device: CSR -> r x c dense tiles, and the tiles written back out as a CSR.
//
// Replaces, on device arrays,
//   BCSR::BCSR(const CSR&, r, c)              nlibs/BCSR.cc:3-65     (a count pass and a fill pass, both sequential)
//   BCSR::isEqual's row walk                  nlibs/BCSR.cc:67-116   (tile after tile, cell after cell: hip_bcsr_to_csr)
//
// Layout (the reference's): bm = ceil(m / r), bn = ceil(n / c); rowPtr is int[bm + 1], colInd int[nnzb] block columns,
// values nnzb * r * c with tile k at k * r * c and entry (i, col) in cell (i % r) * c + col % c; every other cell +0.0.
// The tiles of a block row are in FIRST-OCCURRENCE order (the block row's rows ascending, each in A's storage order, a
// block column appended when first met), and of repeated (row, col) the LAST in storage order stays.
//
// Forward.  key = ((brow << bcolBits) | bcol) << cellBits | cell with the entry's storage index as payload, sorted by the
// stable LSD radix passes of csr_common_device.hpp over exactly the bits in use (bits_of(bm-1) + bits_of(bn-1) + bits_of(r*c-1)
// <= 64 for every legal shape; the host checks).  Then
//   * a group (one tile) is a run of equal (brow, bcol): head flags, the library's scan -> group id of every entry, nnzb;
//   * equal keys sit together in storage order, so the first of a run carries the smallest index that hits its cell and
//     the last of a run is the entry that writes it: no two stores ever aim at one cell;
//   * a tile's place in its block row is the rank of the smallest storage index among its entries.  Storage index ascends
//     with the row and so with the block row, hence sorting the nnzb groups by that index alone (key2 = minIdx, passes over
//     bits_of(nnz - 1) bits) is the final tile order; the minimum is an integer atomicMin per run head
//     (order-independent, so deterministic); rowPtr is one search per block row in the block rows of the sorted groups;
//   * values: memset to +0.0, then one scatter dealt by sorted entries (consecutive lanes hit ascending cells of a tile).
// No per-(block row, block column) counters and no floating-point atomics.
//
// Inverse.  One wave per output row: the row's ntiles * c cells are walked 64 at a time, the kept ones (global column
// < n, fabs((double)v) > drop_tol) counted with a ballot, then -- after the library's scan -- written at the wave's
// running offset plus the lane's rank in the ballot (v_mbcnt), which keeps the order inside the row.  A long block row is
// spread over the 64 lanes; nothing is staged in LDS.
//
// Every value that becomes an address (rowPtr, the columns, the block columns) is checked first by k_check_rowptr
// / k_check_cols; the host reads the flag before anything is queued that indexes with them.  dB is addressed with 64-bit
// offsets throughout.  Uses csr_common_device.hpp (the checks and their one read-back, row search, lower bound, scan,
// radix sort, Scratch).
#pragma once

namespace bcsr {

using namespace csrdev;

constexpr int ROW_WAVES = 4;                       // rows (waves) per block of the two inverse kernels

// sort keys, dealt by entries (lane-strided inside the block's tile); rowPtr and the columns have been validated
__global__ __launch_bounds__(CP_THREADS) void k_keys(int m, int nnz, int r, int c, int bcolBits, int cellBits,
                                                     const int* __restrict__ IA, const int* __restrict__ JA,
                                                     unsigned long long* __restrict__ keys, int* __restrict__ payload) {
  __shared__ int rows[2];
  const long long base = (long long)blockIdx.x * CP_TILE;
  tile_rows(IA, m, nnz, base, rows);
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const long long o = base + k * CP_THREADS + threadIdx.x;
    if (o >= nnz) break;
    const int row = row_of_entry(IA, rows[0], rows[1], (int)o);
    const int col = JA[o], brow = row / r, bcol = col / c;
    const unsigned cell = (unsigned)((row - brow * r) * c + (col - bcol * c));
    keys[o] = (((((unsigned long long)(unsigned)brow) << bcolBits) | (unsigned)bcol) << cellBits) | cell;
    payload[o] = (int)o;
  }
}

// head[i] = 1 where a new (brow, bcol) starts in the sorted keys; scanned in place afterwards, so that
// head[i + 1] - 1 is the group of sorted entry i and head[nnz] the number of groups
__global__ void k_group_heads(int nnz, int cellBits, const unsigned long long* __restrict__ keys, int* __restrict__ head) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  head[i] = (i == 0 || (keys[i] >> cellBits) != (keys[i - 1] >> cellBits)) ? 1 : 0;
}

// per group: its (brow, bcol) and the smallest storage index among its entries.  Only the first of a run of equal keys
// can hold the minimum of its cell (the sort is stable), so only those lanes touch minIdx (preset to 0xffffffff).
__global__ void k_group_min(int nnz, int cellBits, const unsigned long long* __restrict__ keys, const int* __restrict__ idx,
                            const int* __restrict__ gscan, unsigned long long* __restrict__ ghead,
                            unsigned* __restrict__ minIdx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const unsigned long long key = keys[i];
  if (i > 0 && keys[i - 1] == key) return;
  const int g = gscan[i + 1] - 1;
  atomicMin(&minIdx[g], (unsigned)idx[i]);
  if (gscan[i + 1] != gscan[i]) ghead[g] = key >> cellBits;
}

__global__ void k_group_keys(int nnzb, const unsigned* __restrict__ minIdx, unsigned long long* __restrict__ key2,
                             int* __restrict__ gid) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nnzb) return;
  key2[g] = minIdx[g];
  gid[g] = g;
}

// after the second sort: tile k is group gid[k]; its block row goes into tbrow[k] (ascending in k)
__global__ void k_group_rank(int nnzb, int bcolBits, const int* __restrict__ gid, const unsigned long long* __restrict__ ghead,
                             int* __restrict__ rank, int* __restrict__ tbrow, int* __restrict__ JB) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnzb) return;
  const int g = gid[k];
  const unsigned long long head = ghead[g];
  rank[g] = k;
  tbrow[k] = (int)(head >> bcolBits);
  JB[k] = (int)(head & ((1ull << bcolBits) - 1ull));
}

// IB[b] = first tile of block row b or later, b = 0..bm
__global__ void k_block_rowptr(int bm, int nnzb, const int* __restrict__ tbrow, int* __restrict__ IB) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b <= bm) IB[b] = first_at_least(tbrow, 0, nnzb, b);
}

// the last of every run of equal keys writes its cell (B has been zeroed)
template <class V>
__global__ void k_fill(int nnz, int rc, int cellBits, const unsigned long long* __restrict__ keys, const int* __restrict__ idx,
                       const int* __restrict__ gscan, const int* __restrict__ rank, const V* __restrict__ A,
                       V* __restrict__ B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz) return;
  const unsigned long long key = keys[i];
  if (i + 1 < nnz && keys[i + 1] == key) return;
  const long long cell = (long long)(key & ((1ull << cellBits) - 1ull));
  B[(long long)rank[gscan[i + 1] - 1] * rc + cell] = A[idx[i]];
}

// ---- inverse ------------------------------------------------------------------------------------------------------------
// The cells of one output row, 64 per step, all 64 lanes in every step (the trip count depends on the row alone): the
// lane's cell is (tile, ej) with ej the in-tile column; a step moves every lane on by 64 cells = 64 / c tiles and 64 % c
// columns, so nothing is divided inside the loop.  EMIT = false counts, EMIT = true writes at `pos` onwards.  Returns
// the number of kept cells.
template <class V, bool EMIT>
__device__ __forceinline__ unsigned long long walk_row(int n, int c, long long rc, int ei, int s, int ntiles,
                                                       const int* __restrict__ JB, const V* __restrict__ B, double tol,
                                                       long long pos, int* __restrict__ JC, V* __restrict__ C) {
  const int lane = lane_id(), stepTiles = 64 / c, stepCols = 64 % c;
  long long tile = lane / c;
  int ej = lane % c;
  unsigned long long kept = 0;
  for (long long t0 = 0; t0 < (long long)ntiles * c; t0 += 64) {
    bool keep = false;
    long long col = 0;
    V v = V(0);
    if (tile < ntiles) {
      const long long k = (long long)s + tile;
      col = (long long)JB[k] * c + ej;
      if (col < n) {
        v = B[k * rc + (long long)ei * c + ej];
        keep = fabs((double)v) > tol;                          // false for NaN
      }
    }
    const unsigned long long mk = ballot64(keep);
    if constexpr (EMIT) {
      if (keep) {
        const long long o = pos + (long long)kept + mask_rank(mk);
        JC[o] = (int)col;
        C[o] = v;
      }
    }
    kept += (unsigned long long)__popcll(mk);
    tile += stepTiles;
    ej += stepCols;
    if (ej >= c) { ej -= c; ++tile; }
  }
  return kept;
}

// EMIT = false: IC[row] = kept cells of the row (saturating at 2^32 - 1: the 64-bit total of the scan then shows the
// overflow).  EMIT = true: IC is the scanned rowPtr.
template <class V, bool EMIT>
__global__ __launch_bounds__(ROW_WAVES * 64) void k_rows(int m, int n, int r, int c, const int* __restrict__ IB,
                                                         const int* __restrict__ JB, const V* __restrict__ B, double tol,
                                                         int* __restrict__ IC, int* __restrict__ JC, V* __restrict__ C) {
  const long long row = (long long)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
  if (row >= m) return;                                        // the whole wave
  const int bi = (int)(row / r), ei = (int)(row - (long long)bi * r);
  const int s = IB[bi];
  const long long pos = EMIT ? (long long)IC[row] : 0;
  const unsigned long long kept = walk_row<V, EMIT>(n, c, (long long)r * c, ei, s, IB[bi + 1] - s, JB, B, tol, pos, JC, C);
  if constexpr (!EMIT) {
    if (lane_id() == 0) IC[row] = (int)(unsigned)(kept < 0xffffffffull ? kept : 0xffffffffull);
  }
}

static int check_tile_shape(int r, int c) {
  if (r < 1 || c < 1 || (long long)r * c > SPGEMM_BCSR_MAX_TILE)
    return fail(SPGEMM_ERR_ARG, "tile r=%d c=%d: need r >= 1, c >= 1, r * c <= %d", r, c, SPGEMM_BCSR_MAX_TILE);
  return SPGEMM_OK;
}

static inline int blocks_of(int len, int tile) { return (int)(((long long)len + tile - 1) / tile); }

template <class V>
static int to_bcsr(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, int r, int c,
                   int** dIB, int** dJB, V** dB, int* nnzb) {
  if (!dIB || !dJB || !dB || !nnzb) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIB = nullptr; *dJB = nullptr; *dB = nullptr; *nnzb = 0;
  CHK(check_tile_shape(r, c));
  CHK(check_csr_args(m, n, nnz, dIA, dJA, dA));
  const int bm = blocks_of(m, r), bn = blocks_of(n, c), rc = r * c;
  const int browBits = bits_of(bm - 1), bcolBits = bits_of(bn - 1), cellBits = bits_of(rc - 1);
  if (browBits + bcolBits + cellBits > 64)
    return fail(SPGEMM_ERR_INTERNAL, "sort key of %d + %d + %d bits", browBits, bcolBits, cellBits);
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *IB = nullptr, *JB = nullptr, *idxA = nullptr, *idxB = nullptr, *bhist = nullptr, *gscan = nullptr,
      *gidB = nullptr, *rank = nullptr, *tbrow = nullptr;
  unsigned* minIdx = nullptr;
  V* B = nullptr;
  unsigned long long *keyA = nullptr, *keyB = nullptr, *tile = nullptr, *ghead = nullptr, *key2B = nullptr;
  // validation, one read-back: rowPtr (the key kernel searches it) and the column range (the block column becomes an address)
  int hbad = 0;
  if (int rc = validate_csr(sc, s, m, n, nnz, dIA, dJA, &hbad)) return sc.done(rc);
  if (hbad & BAD_ROWPTR) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer ending at nnz=%d", nnz));
  if (hbad & BAD_COLUMN) return sc.done(fail(SPGEMM_ERR_INPUT, "column outside [0,%d)", n));
  CSR_ALLOC(&IB, sizeof(int) * ((size_t)bm + 1), true);
  if (nnz == 0) {
    CSR_ALLOC(&JB, sizeof(int), true);
    CSR_ALLOC(&B, sizeof(V), true);
    CSR_HIP(hipMemsetAsync(IB, 0, sizeof(int) * ((size_t)bm + 1), s));
    CSR_HIP(hipStreamSynchronize(s));
    *dIB = IB; *dJB = JB; *dB = B;
    return sc.done(SPGEMM_OK);
  }
  // (1) entries sorted by (block row, block column, cell), storage order inside equal keys
  const int nblk = cdiv(nnz, RS_TILE);
  CSR_ALLOC(&keyA, sizeof(unsigned long long) * (size_t)nnz);
  CSR_ALLOC(&keyB, sizeof(unsigned long long) * (size_t)nnz);
  CSR_ALLOC(&idxA, sizeof(int) * (size_t)nnz);
  CSR_ALLOC(&idxB, sizeof(int) * (size_t)nnz);
  CSR_ALLOC(&bhist, sizeof(int) * ((size_t)nblk * RS_RADIX + 1));
  CSR_ALLOC(&tile, scan_scratch_bytes(std::max<long long>((long long)nblk * RS_RADIX, nnz) + 1));
  CSR_ALLOC(&gscan, sizeof(int) * ((size_t)nnz + 1));
  hipLaunchKernelGGL(k_keys, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, r, c, bcolBits, cellBits,
                     dIA, dJA, keyA, idxA);
  radix_sort_bits(s, nnz, 0, browBits + bcolBits + cellBits, keyA, keyB, idxA, idxB, bhist, tile);
  // (2) the groups: one per tile; their number decides the size of the result
  hipLaunchKernelGGL(k_group_heads, grid256(nnz), dim3(256), 0, s, nnz, cellBits, keyA, gscan);
  scan_inplace(s, gscan, nnz, tile);
  int groups = 0;
  CSR_HIP(hipMemcpyAsync(&groups, gscan + nnz, sizeof(int), hipMemcpyDeviceToHost, s));
  CSR_HIP(hipStreamSynchronize(s));
  const long long cells = (long long)groups * rc;
  if (cells > INT_MAX)
    return sc.done(fail(SPGEMM_ERR_OVERFLOW, "%d tiles of %d x %d: %lld values do not fit int32", groups, r, c, cells));
  CSR_ALLOC(&JB, sizeof(int) * (size_t)groups, true);
  CSR_ALLOC(&B, sizeof(V) * (size_t)cells, true);
  CSR_ALLOC(&ghead, sizeof(unsigned long long) * (size_t)groups);
  CSR_ALLOC(&key2B, sizeof(unsigned long long) * (size_t)groups);
  CSR_ALLOC(&minIdx, sizeof(unsigned) * (size_t)groups);
  CSR_ALLOC(&gidB, sizeof(int) * (size_t)groups);
  CSR_ALLOC(&rank, sizeof(int) * (size_t)groups);
  CSR_ALLOC(&tbrow, sizeof(int) * (size_t)groups);
  CSR_HIP(hipMemsetAsync(minIdx, 0xff, sizeof(unsigned) * (size_t)groups, s));
  CSR_HIP(hipMemsetAsync(B, 0, sizeof(V) * (size_t)cells, s));
  hipLaunchKernelGGL(k_group_min, grid256(nnz), dim3(256), 0, s, nnz, cellBits, keyA, idxA, gscan, ghead, minIdx);
  // (3) the tiles of a block row in first-occurrence order: the groups sorted by their smallest storage index.  The
  // first sort's spare arrays hold nnz >= groups elements and serve as this sort's first pair.
  const int idxBits = std::max(1, bits_of(nnz - 1));
  unsigned long long* key2A = keyB;
  int* gidA = idxB;
  hipLaunchKernelGGL(k_group_keys, grid256(groups), dim3(256), 0, s, groups, minIdx, key2A, gidA);
  radix_sort_bits(s, groups, 0, idxBits, key2A, key2B, gidA, gidB, bhist, tile);
  hipLaunchKernelGGL(k_group_rank, grid256(groups), dim3(256), 0, s, groups, bcolBits, gidA, ghead, rank, tbrow, JB);
  hipLaunchKernelGGL(k_block_rowptr, grid256((long long)bm + 1), dim3(256), 0, s, bm, groups, tbrow, IB);
  // (4) values
  hipLaunchKernelGGL(k_fill<V>, grid256(nnz), dim3(256), 0, s, nnz, rc, cellBits, keyA, idxA, gscan, rank, dA, B);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  *dIB = IB; *dJB = JB; *dB = B; *nnzb = groups;
  return sc.done(SPGEMM_OK);
}

template <class V>
static int to_csr(spgemm_handle* h, int m, int n, int r, int c, int nnzb, const int* dIB, const int* dJB, const V* dB,
                  double drop_tol, int** dIC, int** dJC, V** dC, int* nnzC) {
  if (!dIC || !dJC || !dC || !nnzC) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *dIC = nullptr; *dJC = nullptr; *dC = nullptr; *nnzC = 0;
  CHK(check_tile_shape(r, c));
  if (m < 0 || n < 0 || nnzb < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (!(drop_tol >= 0.0)) return fail(SPGEMM_ERR_ARG, "drop_tol=%g is negative or NaN", drop_tol);
  if ((m > 0 && !dIB) || (nnzb > 0 && (!dJB || !dB))) return fail(SPGEMM_ERR_ARG, "BCSR arrays null with m=%d nnzb=%d", m, nnzb);
  if (m == 0 && nnzb > 0) return fail(SPGEMM_ERR_ARG, "nnzb=%d in a matrix without rows", nnzb);
  const int bm = blocks_of(m, r), bn = blocks_of(n, c);
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *IC = nullptr, *JC = nullptr;
  V* C = nullptr;
  unsigned long long* tile = nullptr;
  // validation, one read-back: the block rowPtr against nnzb and every block column (both become addresses into dB / JC)
  int hbad = 0;
  if (int rc = validate_csr(sc, s, bm, bn, nnzb, dIB, dJB, &hbad)) return sc.done(rc);
  if (hbad & BAD_ROWPTR) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone block row pointer ending at nnzb=%d", nnzb));
  if (hbad & BAD_COLUMN) return sc.done(fail(SPGEMM_ERR_INPUT, "block column outside [0,%d)", bn));
  CSR_ALLOC(&IC, sizeof(int) * ((size_t)m + 1), true);
  CSR_ALLOC(&tile, scan_scratch_bytes((long long)m + 1));
  const dim3 grid((unsigned)std::max(1, blocks_of(m, ROW_WAVES))), block(ROW_WAVES * 64);
  if (m > 0)
    hipLaunchKernelGGL((k_rows<V, false>), grid, block, 0, s, m, n, r, c, dIB, dJB, dB, drop_tol, IC, (int*)nullptr, (V*)nullptr);
  unsigned long long total = 0;
  CSR_HIP(scan_total(s, IC, m, tile, &total));
  if (total > (unsigned long long)INT_MAX)
    return sc.done(fail(SPGEMM_ERR_OVERFLOW, "%llu entries do not fit the int32 CSR", total));
  CSR_ALLOC(&JC, sizeof(int) * (size_t)std::max<unsigned long long>(total, 1), true);
  CSR_ALLOC(&C, sizeof(V) * (size_t)std::max<unsigned long long>(total, 1), true);
  if (total > 0)
    hipLaunchKernelGGL((k_rows<V, true>), grid, block, 0, s, m, n, r, c, dIB, dJB, dB, drop_tol, IC, JC, C);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  *dIC = IC; *dJC = JC; *dC = C; *nnzC = (int)total;
  return sc.done(SPGEMM_OK);
}

}  // namespace bcsr

extern "C" int hip_csr_to_bcsr(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA, int r,
                               int c, int** dIB, int** dJB, float** dB, int* nnzb) {
  return bcsr::to_bcsr<float>(h, m, n, nnz, dIA, dJA, dA, r, c, dIB, dJB, dB, nnzb);
}

extern "C" int hip_csr_to_bcsr_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                                   int r, int c, int** dIB, int** dJB, double** dB, int* nnzb) {
  return bcsr::to_bcsr<double>(h, m, n, nnz, dIA, dJA, dA, r, c, dIB, dJB, dB, nnzb);
}

extern "C" int hip_bcsr_to_csr(spgemm_handle* h, int m, int n, int r, int c, int nnzb, const int* dIB, const int* dJB,
                               const float* dB, double drop_tol, int** dIC, int** dJC, float** dC, int* nnzC) {
  return bcsr::to_csr<float>(h, m, n, r, c, nnzb, dIB, dJB, dB, drop_tol, dIC, dJC, dC, nnzC);
}

extern "C" int hip_bcsr_to_csr_f64(spgemm_handle* h, int m, int n, int r, int c, int nnzb, const int* dIB, const int* dJB,
                                   const double* dB, double drop_tol, int** dIC, int** dJC, double** dC, int* nnzC) {
  return bcsr::to_csr<double>(h, m, n, r, c, nnzb, dIB, dJB, dB, drop_tol, dIC, dJC, dC, nnzC);
}
