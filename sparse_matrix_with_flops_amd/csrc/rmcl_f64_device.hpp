// rmcl_f64_device.hpp — the R-MCL row rule with double values (the reference's FDOUBLE build of nlibs/tools/util.cc:4-69
// and nlibs/qrmcl.cc:96-117): inflate v*v, row max and row sum, thresh = clamp(0.90*avg*(1 - 2*(max - avg)), 1e-7, max)
// with avg = sum / stored entries, keep v*v >= thresh, divide the kept squares by their sum.  Every operation in double.
//
//   prune_emit_group64 / _block64   the rule on a finished row that still sits in the split LDS table (int keys, double
//                                   values) of the f64 numeric kernels (spgemm_f64_device.hpp, PRUNE = true): only the
//                                   kept, normalised entries reach the scratch C, at the front of the row's range
//   k_rmcl_fix_rows64               the rows those kernels write out in full (L_i > F64_LDS_MAXL): the rule in place
//   k_rmcl_move64                   packs the fronts of the scratch rows into the result CSR
//   k_rmcl_stats64 / _compact64     the rule on a C that already sits in HBM (hip_rmcl_prune_f64), stable compaction
//
// Cross-lane reductions of a double: the value is moved as its two 32-bit halves by v_mov_b32 DPP (the float path's
// butterfly: quad_perm, quad_perm, row_half_mirror, row_mirror), then one v_add_f64 / v_max_f64 per step.  gfx950 has no
// 64-bit DPP operand for these controls, and __shfl_xor of a double is two ds_bpermute_b32 plus the address VALU and a wait
// on the LDS queue per step; the DPP form is two VALU moves per step and stays off the LDS pipe, which the fused epilogues
// are reading their tables through at the same time.  The kernels are bandwidth-bound either way.
#pragma once
#include "spgemm_device.hpp"

namespace smf {

__device__ __forceinline__ double rmcl_threshold(double avg, double mx) {
  double ret = 0.90 * avg * (1 - 2 * (mx - avg));       // computeThreshold (util.cc:4-9) with QValue = double
  ret = (ret > 1.0e-7) ? ret : 1.0e-7;
  ret = (ret > mx) ? mx : ret;
  return ret;
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = SMF_DPP(__double2loint(v), CTRL, 0xf, 0), hi = SMF_DPP(__double2hiint(v), CTRL, 0xf, 0);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// all-reduce inside the L lanes that share a row (16: one DPP row; 64: the four row results combined in a fixed order)
template <int L, class Op>
__device__ __forceinline__ double rowL_allreduce(double v, Op op) {
  static_assert(L == 16 || L == 64, "16-lane groups or whole waves");
  v = op(v, dpp_f64<0xB1>(v));                       // quad_perm [1,0,3,2]
  v = op(v, dpp_f64<0x4E>(v));                       // quad_perm [2,3,0,1]
  v = op(v, dpp_f64<0x141>(v));                      // row_half_mirror
  v = op(v, dpp_f64<0x140>(v));                      // row_mirror
  if (L == 64) v = op(op(readlane_f64(v, 0), readlane_f64(v, 16)), op(readlane_f64(v, 32), readlane_f64(v, 48)));
  return v;
}
template <int L> __device__ __forceinline__ double rowL_sum(double v) { return rowL_allreduce<L>(v, [](double a, double b) { return a + b; }); }
template <int L> __device__ __forceinline__ double rowL_max(double v) { return rowL_allreduce<L>(v, [](double a, double b) { return fmax(a, b); }); }

// ---- fused epilogues ------------------------------------------------------------------------------------------------
// L lanes (a 16-lane group or a wave) own the row and sweep slots [0, per), per a multiple of L.  byKey: a hash table,
// occupied = key set; else the plain list of the row's `want` products.  Returns the kept count; *nocc = occupied slots.
template <int L>
__device__ __forceinline__ int prune_emit_group64(const int* keys, const double* vals, int per, int want, bool byKey,
                                                  bool live, int gl, int* __restrict__ JCrow, double* __restrict__ Crow,
                                                  int* nocc) {
  double mx = 0.0, sum = 0.0;
  int n = 0;
  for (int i0 = 0; i0 < per; i0 += L) {
    const bool occ = live && (byKey ? keys[i0 + gl] != EMPTY_KEY : i0 + gl < want);
    const double c = vals[i0 + gl], v = occ ? c * c : 0.0;
    mx = fmax(mx, v);
    sum += v;
    n += __popcll(group_mask<L>(ballot64(occ), gl));
  }
  mx = rowL_max<L>(mx);
  sum = rowL_sum<L>(sum);
  *nocc = n;
  const double th = rmcl_threshold(sum / (double)want, mx);
  double ks = 0.0;
  for (int i0 = 0; i0 < per; i0 += L) {
    const bool occ = live && (byKey ? keys[i0 + gl] != EMPTY_KEY : i0 + gl < want);
    const double c = vals[i0 + gl], v = c * c;
    ks += (occ && v >= th) ? v : 0.0;
  }
  ks = rowL_sum<L>(ks);
  const double inv = 1.0 / ks;                         // one division per row; v * inv is within an ulp of v / ks
  int pos = 0;
  for (int i0 = 0; i0 < per; i0 += L) {
    const int k = keys[i0 + gl];
    const bool occ = live && (byKey ? k != EMPTY_KEY : i0 + gl < want);
    const double c = vals[i0 + gl], v = c * c;
    const bool keep = occ && v >= th;
    const unsigned long long gm = group_mask<L>(ballot64(keep), gl);
    if (keep) {
      const int o = pos + __popcll(gm & ((1ull << gl) - 1ull));
      if (o < want) { st_out(JCrow + o, k); st_out(Crow + o, v * inv); }
    }
    pos += __popcll(gm);
  }
  return pos;
}

// the same for a block of NT threads on a table of `size` <= NT * MAXSTEPS slots.  One sweep of the table: every thread
// loads its MAXSTEPS slots back to back (the loads overlap; three dependent sweeps of a 4096-slot table cost more than the
// product walk of its row) and keeps key and squared value in registers, -1 marking an empty slot (never >= a threshold).
// Partials are combined in wave order by every thread, so the threshold, the kept sum and the places of the kept entries
// (wave by wave, step by step, lane by lane) do not depend on timing.
template <int NW> struct PruneShared64 { double mx[NW], sum[NW], ks[NW]; int occ[NW], kc[NW]; };

template <int NT, int MAXSTEPS>
__device__ __forceinline__ void prune_emit_block64(const int* keys, const double* vals, int size, int want,
                                                   PruneShared64<NT / WAVE>& ps, int* __restrict__ JCrow,
                                                   double* __restrict__ Crow, int* __restrict__ cntRow, int* __restrict__ err) {
  constexpr int NW = NT / WAVE;
  const int tid = threadIdx.x, lane = lane_id(), w = tid / WAVE;
  int k[MAXSTEPS];
  double v[MAXSTEPS];
#pragma unroll
  for (int sidx = 0; sidx < MAXSTEPS; ++sidx) {
    const int i = sidx * NT + tid;
    k[sidx] = i < size ? keys[i] : EMPTY_KEY;
    v[sidx] = i < size ? vals[i] : 0.0;
  }
  double mx = 0.0, sum = 0.0;
  int n = 0;
#pragma unroll
  for (int sidx = 0; sidx < MAXSTEPS; ++sidx) {
    if (sidx * NT < size) {                            // block-uniform: the steps beyond the table are skipped throughout
      const bool occ = k[sidx] != EMPTY_KEY;
      const double sq = v[sidx] * v[sidx];
      v[sidx] = occ ? sq : -1.0;
      mx = fmax(mx, v[sidx]);
      sum += occ ? sq : 0.0;
      n += __popcll(ballot64(occ));
    }
  }
  mx = rowL_max<64>(mx);
  sum = rowL_sum<64>(sum);
  if (lane == 0) { ps.mx[w] = mx; ps.sum[w] = sum; ps.occ[w] = n; }
  __syncthreads();
  mx = 0.0; sum = 0.0; n = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) { mx = fmax(mx, ps.mx[i]); sum += ps.sum[i]; n += ps.occ[i]; }
  const double th = rmcl_threshold(sum / (double)want, mx);
  double ks = 0.0;
  int kc = 0;                                          // kept by this wave (wave-uniform)
#pragma unroll
  for (int sidx = 0; sidx < MAXSTEPS; ++sidx) {
    const bool keep = sidx * NT < size && v[sidx] >= th;
    ks += keep ? v[sidx] : 0.0;
    kc += __popcll(ballot64(keep));
  }
  ks = rowL_sum<64>(ks);
  if (lane == 0) { ps.ks[w] = ks; ps.kc[w] = kc; }
  __syncthreads();
  ks = 0.0;
  int pos = 0, total = 0;                              // this wave's first place: the waves before it, in wave order
#pragma unroll
  for (int i = 0; i < NW; ++i) { ks += ps.ks[i]; pos += i < w ? ps.kc[i] : 0; total += ps.kc[i]; }
  const double inv = 1.0 / ks;                         // one division per row; v * inv is within an ulp of v / ks
#pragma unroll
  for (int sidx = 0; sidx < MAXSTEPS; ++sidx) {
    if (sidx * NT < size) {
      const bool keep = v[sidx] >= th;
      const unsigned long long mk = ballot64(keep);
      const int o = pos + mask_rank(mk);
      if (keep && o < want) { st_out(JCrow + o, k[sidx]); st_out(Crow + o, v[sidx] * inv); }
      pos += __popcll(mk);
    }
  }
  if (tid == 0) {
    *cntRow = min(total, want);
    if (n != want) atomicOr(err, ERRF_COUNT_MISMATCH);
  }
}

// ---- rows the numeric kernels wrote out in full: the rule from HBM / L2 by one block per row, the kept entries compacted
// IN PLACE (stable) to the front of the row's range.  Rows of bins [binLo, binHi) with more than lmin entries.
__global__ __launch_bounds__(256) void k_rmcl_fix_rows64(const int* __restrict__ binPtr, int binLo, int binHi,
                                                          const int* __restrict__ rowIds, const int* __restrict__ IC,
                                                          int* __restrict__ JC, double* __restrict__ C,
                                                          int* __restrict__ cnt, int lmin) {
  __shared__ double fred[2][4];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int first = binPtr[binLo], count = binPtr[binHi] - first;
  for (int q = blockIdx.x; q < count; q += gridDim.x) {
    const int row = rowIds[first + q];
    const int s = IC[row], e = IC[row + 1];
    if (e - s <= lmin) continue;                       // block-uniform: the fused epilogue took this row
    double mx = 0.0, sum = 0.0;
    for (int p = s + tid; p < e; p += 256) { const double c = C[p], v = c * c; mx = fmax(mx, v); sum += v; }
    mx = rowL_max<64>(mx);
    sum = rowL_sum<64>(sum);
    if (lane == 0) { fred[0][w] = mx; fred[1][w] = sum; }
    __syncthreads();
    mx = fmax(fmax(fred[0][0], fred[0][1]), fmax(fred[0][2], fred[0][3]));
    sum = ((fred[1][0] + fred[1][1]) + fred[1][2]) + fred[1][3];
    __syncthreads();
    const double th = rmcl_threshold(sum / (double)(e - s), mx);
    double ks = 0.0;
    for (int p = s + tid; p < e; p += 256) { const double c = C[p], v = c * c; ks += v >= th ? v : 0.0; }
    ks = rowL_sum<64>(ks);
    if (lane == 0) fred[0][w] = ks;
    __syncthreads();
    ks = ((fred[0][0] + fred[0][1]) + fred[0][2]) + fred[0][3];
    int out = 0;                                       // kept so far (block-uniform)
    for (int p0 = s; p0 < e; p0 += 256) {
      const int p = p0 + tid;
      const double c = p < e ? C[p] : 0.0;
      const int j = p < e ? JC[p] : 0;
      asm volatile("" :: "v"(c), "v"(j));              // both loads have landed before the barrier: the writes below may
      const double v = c * c;                          // hit positions other lanes of this step read
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

// the kept entries sit at the front of every row's scratch range [IC[row], ...), newPtr is the scan of their counts
template <int L>
__global__ __launch_bounds__(256) void k_rmcl_move64(int m, const int* __restrict__ IC, const int* __restrict__ newPtr,
                                                      const int* __restrict__ JC, const double* __restrict__ C,
                                                      int* __restrict__ JN, double* __restrict__ CN) {
  constexpr int RPB = 256 / L;
  const int gl = threadIdx.x & (L - 1);
  for (int row = blockIdx.x * RPB + threadIdx.x / L; row < m; row += gridDim.x * RPB) {
    const int src = IC[row], dst = newPtr[row], n = newPtr[row + 1] - dst;
    for (int i = gl; i < n; i += L) { JN[dst + i] = JC[src + i]; CN[dst + i] = C[src + i]; }
  }
}

// ---- the rule on a C in HBM (hip_rmcl_prune_f64): L lanes per row, two passes
// pass 1: per-row threshold, kept sum and kept count -> cnt[row]
template <int L>
__global__ __launch_bounds__(256) void k_rmcl_stats64(int m, const int* __restrict__ IC, const double* __restrict__ C,
                                                       int* __restrict__ cnt, double* __restrict__ thresh,
                                                       double* __restrict__ ksum) {
  constexpr int RPB = 256 / L;
  const int gl = threadIdx.x & (L - 1);
  const int nrowsL = (m + RPB - 1) / RPB * RPB;
  for (int row = blockIdx.x * RPB + threadIdx.x / L; row < nrowsL; row += gridDim.x * RPB) {
    const bool live = row < m;
    const int s = live ? IC[row] : 0, e = live ? IC[row + 1] : 0;
    double mx = 0.0, sum = 0.0;
    for (int p = s + gl; p < e; p += 4 * L) {
      double c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = p + i * L < e ? C[p + i * L] : 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) { const double v = c[i] * c[i]; mx = fmax(mx, v); sum += v; }
    }
    mx = rowL_max<L>(mx);
    sum = rowL_sum<L>(sum);
    const double th = rmcl_threshold(sum / (double)(e - s), mx);
    double ks = 0.0;
    int kc = 0;
    for (int p = s + gl; p < e; p += 4 * L) {          // the row was just read: L2
      double c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = p + i * L < e ? C[p + i * L] : 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double v = c[i] * c[i];
        if (p + i * L < e && v >= th) { ks += v; ++kc; }
      }
    }
    ks = rowL_sum<L>(ks);
    kc = (int)rowL_sum<L>((double)kc);                 // (exact: integers below 2^53)
    if (live && gl == 0) { cnt[row] = kc; thresh[row] = th; ksum[row] = ks; }
  }
}

// pass 2: stable compaction of the kept entries, normalised, into the new arrays at newPtr[row]
template <int L>
__global__ __launch_bounds__(256) void k_rmcl_compact64(int m, const int* __restrict__ IC, const int* __restrict__ JC,
                                                         const double* __restrict__ C, const int* __restrict__ newPtr,
                                                         const double* __restrict__ thresh, const double* __restrict__ ksum,
                                                         int* __restrict__ JN, double* __restrict__ CN) {
  constexpr int RPB = 256 / L;
  const int gl = threadIdx.x & (L - 1);
  const int lane = lane_id();
  const int nrowsL = (m + RPB - 1) / RPB * RPB;
  for (int row = blockIdx.x * RPB + threadIdx.x / L; row < nrowsL; row += gridDim.x * RPB) {
    const bool live = row < m;
    const int s = live ? IC[row] : 0, e = live ? IC[row + 1] : 0;
    const double th = live ? thresh[row] : 0.0, ks = live ? ksum[row] : 1.0;
    int out = live ? newPtr[row] : 0;
    const int lim = live ? newPtr[row + 1] : 0;
    for (int p0 = s; p0 < e; p0 += 2 * L) {
      double c[2];
      int j[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int p = p0 + i * L + gl;
        c[i] = p < e ? C[p] : 0.0;
        j[i] = p < e ? JC[p] : 0;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const double v = c[i] * c[i];
        const bool keep = p0 + i * L + gl < e && v >= th;
        const unsigned long long mk = ballot64(keep);
        const unsigned long long gm = L == 64 ? mk : ((mk >> (lane - gl)) & ((1ull << L) - 1ull));
        if (keep) { const int o = out + __popcll(gm & ((1ull << gl) - 1ull)); if (o < lim) { JN[o] = j[i]; CN[o] = v / ks; } }
        out += __popcll(gm);
      }
    }
  }
}

}  // namespace smf
