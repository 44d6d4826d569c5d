// spgemm_f64_device.hpp — numeric phase of C = A*B with double values (the reference's FDOUBLE build:
// QValue = double, nlibs/tools/macro.h:3-6; cusparseDcsrgemm, gpus/cusparse_spmm.cc:73).
//
// Everything before the numeric phase depends on the structure only, so the float pipeline's classification, symbolic
// pass and scan are reused as they are: these kernels start from the row bins (rowIds / binPtr) and the exact row
// pointers IC, i.e. every row i knows its output length L_i = IC[i+1] - IC[i].  The float kernels pack (column, float)
// into one 64-bit slot and CAS it; a (column, double) pair does not fit one CAS, so the tables here are split: int keys
// claimed by CAS, double values accumulated by atomicAdd (ds_add_f64 in LDS, global_atomic_add_f64 in device memory under
// -munsafe-fp-atomics): RowTab<double> of spgemm_device.hpp.  Tables are sized from L_i, not from the product count.
//
//   bins 1-4 (1-64 products)      k_num_g16<double>  the float pipeline's 16-lane kernel (spgemm_device.hpp) on the
//                                                split table; rows whose products all hit different columns
//                                                (L_i == products) write them straight to their place, no table
//   bins 5-7 (65-4096 products)   k_num64_rows   one block per row, LDS table of up to 8192 slots (96 KB)
//   bin 8, L_i <= F64_LDS_MAXL    k_num64_rows   the same with 1024 threads, table of 8192 slots loaded up to 3/4
//   bin 8, L_i <= F64_PASS_MAXL   k_num64_rows   the same in ceil(L_i / F64_PASS_L) passes over the row: pass p keeps the
//                                                columns of hash class p (about 4096 of them), compacts them, clears
//   bin 8, wider                  k_num64_rows<GLOBAL>  a table of 2*L_i slots (power of two) in device memory, one region
//                                                per block, compacted into the output row
// Rows come out column-unsorted (the float path's contract).  A full table or an emitted count != L_i raises the error
// word, and the call fails with SPGEMM_ERR_INTERNAL.
// The fused R-MCL step (PRUNE) is the float path's: prune_emit_block of spgemm_device.hpp over RowTab<double>, with the
// table swept NT slots a step (BlockStrided<NT>) where the float kernels give each wave a segment.
#pragma once
#include "spgemm_device.hpp"

namespace smf {

constexpr int F64_LDS_TBL = 8192;          // slots of the bin-7 / bin-8 LDS table: 8192 * 12 B = 96 KB
constexpr int F64_LDS_MAXL = 6144;         // bin-8 rows up to this many entries use it in one pass (load <= 3/4)
constexpr int F64_PASS_L = 4096;           // wider rows: entries per pass (expected load 1/2; a class that overflows the
constexpr int F64_PASS_MAXL = 16 * F64_PASS_L;   // table raises ERRF_TABLE_FULL) -- up to 16 passes, beyond that device memory

// hash class of a column for the multi-pass rows: a mixer independent of the table's multiplicative hash
__device__ __forceinline__ int col_class(int c, int npass) {
  unsigned x = (unsigned)c;
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return (int)(((unsigned long long)x * (unsigned)npass) >> 32);
}
constexpr int F64_BIG_THREADS = 1024;

// ---- bins 5-8: one block per row ------------------------------------------------------------------------------------
template <int NT> struct Row64Stage { int incl[NT]; int off[NT]; double aval[NT]; int wsum[NT / WAVE]; int cnt; };

// the products of one row by a block of NT threads: A entries staged NT at a time (block scan of their B-row lengths),
// every product finds its entry by a binary search of the staged prefix sums; f(col, jb, a, b) for each product (jb = its
// position in B; b = VB[jb] when LOADV, else 0: the multi-pass rows load the value only for the columns of the pass)
template <int NT, bool LOADV, class F>
__device__ __forceinline__ void row64_walk(Row64Stage<NT>& st, int as, int ae, const int2* __restrict__ SBL,
                                           const double* __restrict__ VA, const int* __restrict__ JB,
                                           const double* __restrict__ VB, F&& f) {
  constexpr int U = 2;
  const int tid = threadIdx.x, lane = lane_id(), w = tid / WAVE;
  for (int chunk = as; chunk < ae; chunk += NT) {
    const int ap = chunk + tid;
    int len = 0, bs = 0;
    double a = 0.0;
    if (ap < ae) {
      const int2 sbl = SBL[ap];
      bs = sbl.x;
      len = sbl.y;
      a = VA[ap];
    }
    int incl = wave_incl_add(len);
    if (lane == WAVE - 1) st.wsum[w] = incl;
    __syncthreads();
    for (int i = 0; i < w; ++i) incl += st.wsum[i];
    st.incl[tid] = incl;
    st.off[tid] = bs - (incl - len);
    st.aval[tid] = a;
    __syncthreads();
    const int T = st.incl[NT - 1];
    for (int p0 = 0; p0 < T; p0 += NT * U) {
      int p[U], e[U], col[U], jbs[U];
      double vb[U], av[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { p[u] = min(p0 + u * NT + tid, T - 1); e[u] = 0; }
#pragma unroll
      for (int sft = NT / 2; sft >= 1; sft >>= 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int c = e[u] + sft;
          e[u] = st.incl[c - 1] <= p[u] ? c : e[u];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jb = st.off[e[u]] + p[u];
        jbs[u] = jb;
        col[u] = JB[jb];
        vb[u] = LOADV ? VB[jb] : 0.0;
        av[u] = st.aval[e[u]];
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (p0 + u * NT + tid < T) f(col[u], jbs[u], av[u], vb[u]);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);                  // lgkmcnt(0): no return-less LDS atomic of f in flight at the barrier
    __syncthreads();
  }
}

// GLOBAL = false: rows of the bin with lmin <= L_i <= lmax, LDS table of TBL slots.
// GLOBAL = true: the same in a table of gslots slots per block at gkeys/gvals + blockIdx.x * gslots (device memory).
// PRUNE: rows that finish in one LDS pass get the R-MCL row rule in the epilogue (kept entries to the front of the row's
// range, their count to pcnt[row]); multi-pass and device-memory rows are written in full (k_rmcl_fix_rows<double> of
// rmcl_rows_device.hpp takes them).
template <int NT, int TBL, bool GLOBAL, bool PRUNE = false>
__global__ __launch_bounds__(NT) void k_num64_rows(const int* __restrict__ binPtr, int bin, const int* __restrict__ rowIds,
                                                   const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                   const double* __restrict__ VA, const int* __restrict__ JB,
                                                   const double* __restrict__ VB, const int* __restrict__ IC,
                                                   int* __restrict__ JC, double* __restrict__ C, int* __restrict__ err,
                                                   int lmin, int lmax, int* gkeys, double* gvals, int gslots,
                                                   int* __restrict__ pcnt) {
  __shared__ PruneShared<double, PRUNE ? NT / WAVE : 1> ps;
  __shared__ int skeys[GLOBAL ? 1 : TBL];
  __shared__ double svals[GLOBAL ? 1 : TBL];
  __shared__ Row64Stage<NT> st;
  int* keys = GLOBAL ? gkeys + (size_t)blockIdx.x * gslots : skeys;
  double* vals = GLOBAL ? gvals + (size_t)blockIdx.x * gslots : svals;
  const RowTab<double> tab{keys, vals};
  const int tid = threadIdx.x;
  const int first = binPtr[bin], count = binPtr[bin + 1] - first;
  for (int q = blockIdx.x; q < count; q += gridDim.x) {
    const int row = rowIds[first + q];
    const int off = IC[row];
    const int want = IC[row + 1] - off;
    if (want < lmin || want > lmax || want == 0) continue;             // block-uniform
    const int npass = GLOBAL || want <= F64_LDS_MAXL ? 1 : (want + F64_PASS_L - 1) / F64_PASS_L;
    // power of two >= 2 * want (LDS: capped at TBL, loaded up to 3/4 by the largest one-pass rows)
    const int size = GLOBAL ? next_pow2_clamped(2 * want, 64, 1 << 30) : table_size(want, 64, TBL);
    const int shift = 32 - log2_pow2(size);
    if (tid == 0) st.cnt = 0;
    for (int pass = 0; pass < npass; ++pass) {
      for (int i = tid; i < size; i += NT) tab.clear(i);
      if (GLOBAL) __threadfence();
      __syncthreads();
      auto accum = [&](int col, double v) { tab.accum(size, shift, col, v, err); };
      if (npass == 1)
        row64_walk<NT, true>(st, IA[row], IA[row + 1], SBL, VA, JB, VB, [&](int col, int, double a, double b) { accum(col, a * b); });
      else
        row64_walk<NT, false>(st, IA[row], IA[row + 1], SBL, VA, JB, VB, [&](int col, int jb, double a, double) {
          if (col_class(col, npass) == pass) accum(col, a * VB[jb]);
        });
      if (GLOBAL) __threadfence();                       // the block's atomics are done before any lane reads the table
      __syncthreads();
      if constexpr (PRUNE && !GLOBAL) {
        if (npass == 1) {                                  // block-uniform
          prune_emit_block<NT / WAVE, (TBL + NT - 1) / NT>(tab, BlockStrided<NT>{size}, want, ps, JC + off, C + off, pcnt + row, err);
          if (tid == 0) st.cnt = want;                     // (the epilogue has checked the count itself)
          break;
        }
      }
      for (int i0 = 0; i0 < size; i0 += NT) {
        const int i = i0 + tid;
        const int k = i < size ? keys[i] : EMPTY_KEY;
        const bool occ = k != EMPTY_KEY;
        const unsigned long long mk = ballot64(occ);
        int base = 0;
        if (lane_id() == 0 && mk) base = atomicAdd(&st.cnt, __popcll(mk));
        base = __shfl(base, 0, WAVE);
        const int pos = base + mask_rank(mk);
        if (occ && pos < want) { st_out(JC + off + pos, k); st_out(C + off + pos, vals[i]); }
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);                // lgkmcnt(0)
      __syncthreads();
    }
    if (tid == 0 && st.cnt != want) atomicOr(err, ERRF_COUNT_MISMATCH);
    __syncthreads();
  }
}

// largest L_i among the rows of `bin` with L_i > lmin, and their number: sizes the device-memory tables
__global__ __launch_bounds__(256) void k_num64_wide_rows(const int* __restrict__ binPtr, int bin,
                                                          const int* __restrict__ rowIds, const int* __restrict__ IC,
                                                          int lmin, int* __restrict__ out2) {
  const int first = binPtr[bin], count = binPtr[bin + 1] - first;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < count; q += gridDim.x * 256) {
    const int row = rowIds[first + q];
    const int L = IC[row + 1] - IC[row];
    if (L > lmin) { atomicMax(&out2[0], L); atomicAdd(&out2[1], 1); }
  }
}

}  // namespace smf
