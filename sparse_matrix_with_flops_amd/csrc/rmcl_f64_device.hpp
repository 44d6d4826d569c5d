// rmcl_f64_device.hpp — what the R-MCL row rule needs for double values only (the reference's FDOUBLE build of
// nlibs/tools/util.cc:4-69 and nlibs/qrmcl.cc:96-117): inflate v*v, row max and row sum, thresh = clamp(0.90*avg*(1 -
// 2*(max - avg)), 1e-7, max) with avg = sum / stored entries, keep v*v >= thresh, divide the kept squares by their sum.
// Every operation in double.
//
//   rmcl_threshold(double, double)  the threshold without the float overload's promotions
//   rowL_sum / rowL_max (double)    the cross-lane reductions below
//   prune_emit_group64 / _block64   the rule on a finished row that still sits in the split LDS table (int keys, double
//                                   values) of the f64 numeric kernels (spgemm_f64_device.hpp, PRUNE = true): only the
//                                   kept, normalised entries reach the scratch C, at the front of the row's range
// The kernels that apply the rule to rows in HBM (k_rmcl_stats / _compact / _move / _fix_rows) are templates on the value
// type in rmcl_rows_device.hpp and pick these overloads for V = double.
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

}  // namespace smf
