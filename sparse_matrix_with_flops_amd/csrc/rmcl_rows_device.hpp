// rmcl_rows_device.hpp — the R-MCL post-step (the step right after the SpGEMM in the reference's loop; SURVEY.md §8f
// rank 1) on rows that already sit in HBM, written once for both value types V = float, double.
// CPU: nlibs/tools/util.cc:4-69, nlibs/qrmcl.cc:96-117; reference GPU: nlibs/gpus/dutil.cuh:8-80 + thrust::remove
// (gpu_csr_kernel.cu:218-229,265-270).  The row rule: inflate v*v, row max and row sum, thresh = rmcl_threshold(avg, max),
// keep v*v >= thresh, divide the kept squares by their sum; every operation in V.
//
//   k_rmcl_stats<L, V> / k_rmcl_compact<L, V>   the rule on a C in HBM (hip_rmcl_prune[_n][_f64]), stable compaction
//   k_rmcl_fix_rows<V>                          the rows the fused numeric kernels wrote out in full: the rule in place
//   k_rmcl_move<L, V>                           packs the fronts of the scratch rows into the result CSR
//   k_zip_extents                               {start, end} of every scratch row (the float loop's unpacked Mt)
//
// What differs by type are two overload sets of spgemm_device.hpp, shared with the fused epilogues of the numeric kernels:
// rmcl_threshold (the float one keeps the reference's promotions) and the lane moves under rowL_sum / rowL_max (a double
// crosses lanes as two 32-bit halves).  Sums are L-lane tree reductions in V, so a value that sits within an ulp of the threshold can fall on
// the other side than in the sequential CPU loop (the reference's own GPU path has the same property).
#pragma once
#include "spgemm_device.hpp"
#include <type_traits>

namespace smf {

// pass 1: inflate (squares, recomputed where needed, never stored), per-row threshold and kept sum, kept count ->
// cnt[row].  L lanes per row: 16 for short rows, a whole wave once rows average ~100 entries (R-MCL products do);
// four loads in flight per lane.
template <int L, class V>
__global__ __launch_bounds__(256) void k_rmcl_stats(int m, const int* __restrict__ IC, const V* __restrict__ C,
                                                     int* __restrict__ cnt, V* __restrict__ thresh, V* __restrict__ ksum) {
  constexpr int RPB = 256 / L;                       // rows per block
  const int gl = threadIdx.x & (L - 1);
  const int nrowsL = (m + RPB - 1) / RPB * RPB;
  for (int row = blockIdx.x * RPB + threadIdx.x / L; row < nrowsL; row += gridDim.x * RPB) {
    const bool live = row < m;
    const int s = live ? IC[row] : 0, e = live ? IC[row + 1] : 0;
    V mx = V(0), sum = V(0);
    for (int p = s + gl; p < e; p += 4 * L) {
      V c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = p + i * L < e ? C[p + i * L] : V(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) { const V v = c[i] * c[i]; mx = rmcl_max(mx, v); sum += v; }   // inflate: v^2
    }
    mx = rowL_max<L>(mx);
    sum = rowL_sum<L>(sum);
    const V th = rmcl_threshold(sum / (V)(e - s), mx);
    V ks = V(0);
    int kc = 0;
    for (int p = s + gl; p < e; p += 4 * L) {          // the row was just read: L2
      V c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = p + i * L < e ? C[p + i * L] : V(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) { const V v = c[i] * c[i]; if (p + i * L < e && v >= th) { ks += v; ++kc; } }
    }
    ks = rowL_sum<L>(ks);
    kc = (int)rowL_sum<L>((V)kc);                      // (exact below 2^24 kept entries per row; 2^53 in double)
    if (live && gl == 0) { cnt[row] = kc; thresh[row] = th; ksum[row] = ks; }
  }
}

// pass 2: stable compaction of the kept entries, normalised, into the new arrays at [newPtr[row], newPtr[row + 1]).
// BOUND: no store past newPtr[row + 1], whatever pass 1 counted (nothing new is stored in a correct run).  On for double
// only: in the float 16-lane form the extra load and register measured 2-4 % of hip_rmcl_prune.
template <int L, class V, bool BOUND = std::is_same<V, double>::value>
__global__ __launch_bounds__(256) void k_rmcl_compact(int m, const int* __restrict__ IC, const int* __restrict__ JC,
                                                       const V* __restrict__ C, const int* __restrict__ newPtr,
                                                       const V* __restrict__ thresh, const V* __restrict__ ksum,
                                                       int* __restrict__ JN, V* __restrict__ CN) {
  constexpr int RPB = 256 / L;
  const int gl = threadIdx.x & (L - 1);
  const int lane = lane_id();
  const int nrowsL = (m + RPB - 1) / RPB * RPB;
  for (int row = blockIdx.x * RPB + threadIdx.x / L; row < nrowsL; row += gridDim.x * RPB) {
    const bool live = row < m;
    const int s = live ? IC[row] : 0, e = live ? IC[row + 1] : 0;
    const V th = live ? thresh[row] : V(0), ks = live ? ksum[row] : V(1);
    int out = live ? newPtr[row] : 0;
    const int lim = BOUND && live ? newPtr[row + 1] : 0;
    for (int p0 = s; p0 < e; p0 += 2 * L) {            // two steps of L entries, their loads issued together
      V c[2];
      int j[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int p = p0 + i * L + gl;
        c[i] = p < e ? C[p] : V(0);
        j[i] = p < e ? JC[p] : 0;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const V v = c[i] * c[i];
        const bool keep = p0 + i * L + gl < e && v >= th;
        const unsigned long long mk = ballot64(keep);
        const unsigned long long gm = L == 64 ? mk : ((mk >> (lane - gl)) & ((1ull << L) - 1ull));
        if (keep) { const int o = out + __popcll(gm & ((1ull << gl) - 1ull)); if (!BOUND || o < lim) { JN[o] = j[i]; CN[o] = v / ks; } }
        out += __popcll(gm);
      }
    }
  }
}

// fused path, loop form: {start, end} of every row's kept entries in the scratch arrays, one pair per row
__global__ __launch_bounds__(256) void k_zip_extents(int m, const int* __restrict__ IC, const int* __restrict__ cnt,
                                                      int2* __restrict__ se) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < m) { const int s = IC[r]; se[r] = make_int2(s, s + cnt[r]); }
}

// fused path, after the numeric kernels: the kept entries sit at the front of every row's scratch range
// [IC[row], ...), newPtr is the scan of their counts -- pack them into the new arrays
template <int L, class V>
__global__ __launch_bounds__(256) void k_rmcl_move(int m, const int* __restrict__ IC, const int* __restrict__ newPtr,
                                                    const int* __restrict__ JC, const V* __restrict__ C,
                                                    int* __restrict__ JN, V* __restrict__ CN) {
  constexpr int RPB = 256 / L;
  const int gl = threadIdx.x & (L - 1);
  for (int row = blockIdx.x * RPB + threadIdx.x / L; row < m; row += gridDim.x * RPB) {
    const int src = IC[row], dst = newPtr[row], n = newPtr[row + 1] - dst;
    for (int i = gl; i < n; i += L) { JN[dst + i] = JC[src + i]; CN[dst + i] = C[src + i]; }
  }
}

// fused path, rows the numeric kernels wrote out in full (float: bin 8, whose rows pass through LDS in several pieces;
// double: L_i > F64_LDS_MAXL): the row rule from HBM / L2 by one block per row, the kept entries compacted IN PLACE
// (stable) to the front of the row's range.  Rows of bins [binLo, binHi) with more than lmin entries.
template <class V>
__global__ __launch_bounds__(256) void k_rmcl_fix_rows(const int* __restrict__ binPtr, int binLo, int binHi,
                                                        const int* __restrict__ rowIds, const int* __restrict__ IC,
                                                        int* __restrict__ JC, V* __restrict__ C, int* __restrict__ cnt,
                                                        int lmin) {
  __shared__ V fred[2][4];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int first = binPtr[binLo], count = binPtr[binHi] - first;
  for (int q = blockIdx.x; q < count; q += gridDim.x) {
    const int row = rowIds[first + q];
    const int s = IC[row], e = IC[row + 1];
    if (e - s <= lmin) continue;                       // block-uniform: the fused epilogue took this row
    V mx = V(0), sum = V(0);
    for (int p = s + tid; p < e; p += 256) { const V c = C[p], v = c * c; mx = rmcl_max(mx, v); sum += v; }
    mx = rowL_max<64>(mx);
    sum = rowL_sum<64>(sum);
    if (lane == 0) { fred[0][w] = mx; fred[1][w] = sum; }
    __syncthreads();
    mx = rmcl_max(rmcl_max(fred[0][0], fred[0][1]), rmcl_max(fred[0][2], fred[0][3]));
    sum = ((fred[1][0] + fred[1][1]) + fred[1][2]) + fred[1][3];
    __syncthreads();
    const V th = rmcl_threshold(sum / (V)(e - s), mx);
    V ks = V(0);
    for (int p = s + tid; p < e; p += 256) { const V c = C[p], v = c * c; ks += v >= th ? v : V(0); }
    ks = rowL_sum<64>(ks);
    if (lane == 0) fred[0][w] = ks;
    __syncthreads();
    ks = ((fred[0][0] + fred[0][1]) + fred[0][2]) + fred[0][3];
    int out = 0;                                       // kept so far (block-uniform)
    for (int p0 = s; p0 < e; p0 += 256) {
      const int p = p0 + tid;
      const V c = p < e ? C[p] : V(0);
      const int j = p < e ? JC[p] : 0;
      asm volatile("" :: "v"(c), "v"(j));              // both loads have landed before the barrier: the writes below may
      const V v = c * c;                               // hit positions other lanes of this step read
      const bool keep = p < e && v >= th;
      const unsigned long long mk = ballot64(keep);
      if (lane == 0) wcnt[w] = __popcll(mk);
      __syncthreads();
      int base = out, total = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) { base += i < w ? wcnt[i] : 0; total += wcnt[i]; }
      if (keep) { const int o = s + base + mask_rank(mk); JC[o] = j; C[o] = v / ks; }
      out += total;
      __syncthreads();
    }
    if (tid == 0) cnt[row] = out;
  }
}

}  // namespace smf
