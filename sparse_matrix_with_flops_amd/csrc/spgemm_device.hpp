// spgemm_device.hpp — hand-written HIP kernels for CSR x CSR SpGEMM on MI355X (gfx950, wave64).
//
// Pipeline:   flops+bin  ->  bin scan  ->  scatter rows  ->  symbolic per bin
//                            ->  exclusive scan of IC  ->  numeric per bin
// Reference counterparts (read as text only; nothing is translated line by line):
//   k_row_flops            gcomputeFlops + gcomputeBinId     mindex2-cuda/flops.cu:66-94
//                          dynamic_omp_CSR_flops             nlibs/flops_csr_kernel.cc:14-31
//   k_bin_scan/k_scatter   thrust::stable_sort_by_key + computeHistogram   flops.cu:96-107,131
//                          group_CSR_flops counting sort     nlibs/group_csr_kernel.cc:24-51
//   k_sym_*                sgpu_CSR_IC_nnzC_mid*             mindex2-cuda/tryOutBins.cuh:5-131
//                          gpu_CSR_IC_nnzC                   nlibs/gpus/gpu_csr_kernel.cu:44-82
//   k_num_g16/k_num_hash   sgpu_SpGEMM_mid / fp1 / fp2 / fpl4 mindex2-cuda/gspgemm.cuh:2-293
//                          hashCASAdd2                       mindex2-cuda/casHash.cuh:34-43
//   k_num_big*             sgpu_SpGEMM_olarge (dense map)    "mindex2-cuda/\":143-213
//
// CDNA4 choices: 64-lane ballots / DPP scans instead of __syncthreads()-stepped sub-warp scans;
// products of one C row are flattened over all lanes (B rows of a power-law graph are short: a
// "lanes stride one B row" mapping leaves >90% of a wave idle); several rounds of products are kept
// in flight per wave (the path is latency-bound, not issue-bound); LDS tables sized per row; rows with
// more than 4096 products use either an LDS column bitmap + popcount ranks (n <= 262144: sorted output,
// no probing) or a multi-pass 128 KB LDS hash (any n) — 160 KB LDS per CU is what makes both possible.
// No MFMA: this is index/scatter work.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace smf {

#ifdef SMF_ABLATE
// diagnostic build only (make ablate): pieces of the wave-per-row numeric kernel can be switched off at run time
// (SPGEMM_ABLATE bit mask: 1 no insert, 2 no gathers, 4 no compaction, 8 no walk) to see what its time is made of.
// The results are wrong by construction; never the product.
__device__ int g_ablate = 0;
#define ABL(bit) (g_ablate & (bit))
// error flags (int*) are not raised in this build: with pieces switched off every row "fails" and the flag word serialises
__device__ __forceinline__ void smf_or(int*, int) {}
__device__ __forceinline__ unsigned smf_or(unsigned* p, unsigned v) { return atomicOr(p, v); }   // (k_sym_big<true> reads the old word)
#define atomicOr(p, v) smf_or((p), (v))
#else
#define ABL(bit) 0
#endif

constexpr int WAVE = 64;

// C is written once and not read again by this call: its stores carry the non-temporal hint so that the output stream
// does not push B out of the caches the gathers live on
template <class T> __device__ __forceinline__ void st_out(T* p, T v) {
#ifdef SMF_PLAIN_STORES
  *p = v;
#else
  __builtin_nontemporal_store(v, p);
#endif
}
constexpr int NBINS = 9;  // {0 | 1 | 2-4 | 5-16 | 17-64 | 65-512 | 513-2048 | 2049-4096 | >4096}
constexpr int EMPTY_KEY = -1;

__host__ __device__ __forceinline__ int bin_of(unsigned long long f) {
  if (f == 0) return 0;
  if (f == 1) return 1;
  if (f <= 4) return 2;
  if (f <= 16) return 3;
  if (f <= 64) return 4;
  if (f <= 512) return 5;
  if (f <= 2048) return 6;
  if (f <= 4096) return 7;
  return 8;
}

// Layout slots of the row-id array (finer than the bins; a bin is one or more consecutive slots):
//   slots 0..4  = bins 0..4
//   slots 5, 6  = bin 5 split at 256 products: rows up to 256 products need a 512-slot table, so their wave-per-row
//                 kernel fits 24 blocks per CU instead of 16 (measured on the symbolic kernel: 16 -> 24 waves/CU is
//                 17 % faster, 32 is slower again)
//   slots 7, 8  = bin 6 split at 1024 products: a 2048-slot table lets 7 four-wave blocks share a CU instead of 4 (these
//                 kernels are bound by the serial chain of a row times the rows in flight, not by any unit's throughput)
//   slot  9     = bin 7
//   slots 10..15 = the last bin split into NSUB size classes (4097-8191, 8192-16383, ... by powers of two) laid out
//                 LARGEST FIRST, so that the work queue of the block-per-row kernels hands out the heavy rows first
//                 and the kernel does not end on one of them (measured: k_num_bighash 1.58 -> 1.48 ms at 1 M rows)
constexpr int NSUB = 6;
constexpr int SLOT_H1A = 5, SLOT_H1B = 6, SLOT_H4A = 7, SLOT_H4B = 8, SLOT_H8 = 9, SLOT_BIG0 = 10;
constexpr int NSLOTS = SLOT_BIG0 + NSUB;
constexpr int H1A_MAX = 256, H4A_MAX = 1024;
__host__ __device__ __forceinline__ int slot_of(unsigned long long f) {
  const int b = bin_of(f);
  if (b < 5) return b;
  if (b == 5) return f <= (unsigned)H1A_MAX ? SLOT_H1A : SLOT_H1B;
  if (b == 6) return f <= (unsigned)H4A_MAX ? SLOT_H4A : SLOT_H4B;
  if (b == 7) return SLOT_H8;
  int lg = 12;                                        // f >= 4097
  while (lg < 12 + NSUB - 1 && (f >> (lg + 1)) != 0) ++lg;
  return SLOT_BIG0 + (NSUB - 1 - (lg - 12));
}
// last slot of a bin
__host__ __device__ __forceinline__ int last_slot_of_bin(int b) {
  return b < 5 ? b : b == 5 ? SLOT_H1B : b == 6 ? SLOT_H4B : b == 7 ? SLOT_H8 : NSLOTS - 1;
}

// error flag bits written by kernels into Workspace::d_err
constexpr int ERRF_TABLE_FULL = 1;
constexpr int ERRF_COUNT_MISMATCH = 2;

// ------------------------------------------------------------------------------------------------
// wave64 primitives
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }

// lane mask of a predicate, straight from the compare (HIP's __ballot(int) goes through a 0/1 VGPR and back)
__device__ __forceinline__ unsigned long long ballot64(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }

// number of set bits of `mask` strictly below this lane
__device__ __forceinline__ int mask_rank(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

#define SMF_DPP(v, ctrl, rowmask, ident) __builtin_amdgcn_update_dpp((ident), (v), (ctrl), (rowmask), 0xf, false)

// inclusive +-scan over the 64 lanes; all lanes must be active
__device__ __forceinline__ int wave_incl_add(int v) {
  v += SMF_DPP(v, 0x111, 0xf, 0);  // row_shr:1
  v += SMF_DPP(v, 0x112, 0xf, 0);  // row_shr:2
  v += SMF_DPP(v, 0x114, 0xf, 0);  // row_shr:4
  v += SMF_DPP(v, 0x118, 0xf, 0);  // row_shr:8
  v += SMF_DPP(v, 0x142, 0xa, 0);  // row_bcast:15 -> rows 1,3
  v += SMF_DPP(v, 0x143, 0xc, 0);  // row_bcast:31 -> rows 2,3
  return v;
}

// inclusive max-scan of non-negative ints over the 64 lanes
__device__ __forceinline__ int wave_incl_max(int v) {
  v = max(v, SMF_DPP(v, 0x111, 0xf, 0));
  v = max(v, SMF_DPP(v, 0x112, 0xf, 0));
  v = max(v, SMF_DPP(v, 0x114, 0xf, 0));
  v = max(v, SMF_DPP(v, 0x118, 0xf, 0));
  v = max(v, SMF_DPP(v, 0x142, 0xa, 0));
  v = max(v, SMF_DPP(v, 0x143, 0xc, 0));
  return v;
}

__device__ __forceinline__ int wave_sum(int v) { return __builtin_amdgcn_readlane(wave_incl_add(v), 63); }

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// LDS traffic between lanes of ONE wave: the LDS executes a wave's DS ops in order, so only the
// compiler must be kept from reordering.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // compiler ordering only: no vmcnt drain
  __builtin_amdgcn_s_waitcnt(0xc07f);                       // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int next_pow2_clamped(int x, int lo, int hi) {
  int p = lo;
  while (p < x && p < hi) p <<= 1;
  return p;
}

__device__ __forceinline__ int log2_pow2(int p) { return 31 - __clz(p); }

// power-of-two table for `items` distinct keys at load <= 1/2, clamped to [lo, hi]; `items` may be INT_MAX (saturated flops)
// MULT = 4 (the wave-per-row and multi-wave hash kernels since round 4): a row that leaves room in its kernel's table gets
// four slots per item instead of two.  In the lock-step insert loops every lane pays for the longest probe chain of the
// trip, and the chains shorten with the load faster than the sweep of the larger table grows (measured: hash kernels -1 to
// -4 % each; the 16-lane kernels, which sweep 16 slots at a time, lose with it and stay at 2; R-MCL tables at HALF the
// size: +27 %).
template <int MULT = 2>
__device__ __forceinline__ int table_size(int items, int lo, int hi) {
  return items >= hi / MULT ? hi : next_pow2_clamped(MULT * items, lo, hi);
}

// ------------------------------------------------------------------------------------------------
// LDS open-addressing hash (keys >= 0, EMPTY_KEY = -1), multiplicative hash, linear probing.
// hash_insert: one key per lane (small-row kernels).  Returns the slot of `c`; *is_new is set when this call
// claimed the slot.  `size` is a power of two >= 2 * (number of distinct keys), so a probe sequence always
// terminates; a bounded loop and an error flag guard against corrupt inputs instead of hanging the GPU.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int hash_insert(int* keys, int size, int shift, int c, bool* is_new, int* err) {
  unsigned h = ((unsigned)c * 2654435761u) >> shift;
  const unsigned mask = (unsigned)size - 1u;
  *is_new = false;
  for (int probe = 0; probe < size; ++probe) {
    const int old = atomicCAS(&keys[h], EMPTY_KEY, c);
    if (old == EMPTY_KEY) { *is_new = true; return (int)h; }
    if (old == c) return (int)h;
    h = (h + 1u) & mask;
  }
  atomicOr(err, ERRF_TABLE_FULL);
  return 0;
}

// U keys per lane at once, straight-line code: predication is done through the ADDRESS (a lane with nothing to
// insert aims its CAS / add at a private dummy word), never through a branch, so the U LDS atomics of a probe
// step issue back to back and their latencies overlap; hipcc otherwise wraps every conditional atomic in its
// own exec-mask branch with an s_waitcnt right behind it.  CAS first: most products of a SpGEMM row touch their
// column for the first time, so the claim usually succeeds in one LDS round trip.
// vals == nullptr: symbolic (count only).  `dummy` = one private int per lane.  Returns the slots this lane claimed.
// POW2: size is a power of two (slot = top bits of the multiplicative hash); otherwise any size
// (slot = mulhi(hash, size)), which lets the big-row kernel use every byte of LDS it can get.
// The loop-carried state of the multi-insert loops is integers only: the byte offset of the slot a lane probes next,
// with the lane's private dummy word standing for "done".  (Carried bools live in VGPRs as 0/1 and cost two VALU
// instructions each per round to turn back into lane masks; these kernels are VALU-bound.)  Conditions used inside
// one round stay lane masks in SGPRs and combine on the scalar unit.
// Returns the number of new keys THIS LANE claimed (the caller reduces over the wave once per row).
// The dummy words are initialised to DUMMY_KEY (never EMPTY_KEY, never a column), so a CAS that lands there fails
// and a parked lane needs no masking when the new keys of a round are counted.
// RH (the logging symbolic kernels): (*rehit)[u] says whether product u ended on its own key ALREADY PRESENT -- a re-hit of its
// column -- instead of claiming an empty slot.  The LDS serialises the CAS of a wave instruction lane by lane, so of several
// lanes that bring the same new column in one round exactly one claims it and the others are re-hits: a row's re-hits are
// its products minus its distinct columns.  (A parked lane reads DUMMY_KEY, never a column.)
constexpr int DUMMY_KEY = (int)0x80000000;

template <bool POW2 = true, bool RH = false, int U>
__device__ __forceinline__ int hash_insert_multi(int* keys, int size, int shift, const bool (&act)[U],
                                                 const int (&col)[U], int* dummy, int* err, bool (*rehit)[U] = nullptr) {
  char* const base = reinterpret_cast<char*>(keys);
  const int dumB = (int)(reinterpret_cast<char*>(dummy) - base);
  const int maskB = size * 4 - 1;
  int hB[U];
  int claimed = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const unsigned hv = (unsigned)col[u] * 2654435761u;
    const unsigned h = POW2 ? hv >> shift : __umulhi(hv, (unsigned)size);
    hB[u] = act[u] ? (int)(h * 4u) : dumB;
    if constexpr (RH) (*rehit)[u] = false;
  }
  int probe = 0;
  // Bookkeeping on the vector side (round 3; these kernels fill ~55 % of the SCALAR issue slots too): `claimed` is a
  // per-LANE count of the keys this lane claimed -- a compare and an add instead of ballot + s_bcnt1 + s_add per product
  // and probe round; the caller sums over the wave once per row.  "Any lane still probing" comes from one OR-ed word and
  // one compare instead of a ballot per product.  (k_sym_hash<4,4096> 0.264 -> 0.249 ms, <1,*> 0.223 -> 0.210 ms.)
  for (;;) {                                        // first round unconditional: nothing between the gathers and their use
    int old[U];
#pragma unroll
    for (int u = 0; u < U; ++u) old[u] = atomicCAS(reinterpret_cast<int*>(base + hB[u]), EMPTY_KEY, col[u]);
    ++probe;
    int pendBits = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      claimed += old[u] == EMPTY_KEY ? 1 : 0;                               // the dummy is never EMPTY_KEY
      if constexpr (RH) (*rehit)[u] = (*rehit)[u] || old[u] == col[u];
      const bool adv = hB[u] != dumB && old[u] != EMPTY_KEY && old[u] != col[u];
      // power-of-two tables: triangular steps (+1, +2, +3, ...) visit every slot once and break up probe clusters
      const int nh = POW2 ? ((hB[u] + probe * 4) & maskB) : (hB[u] + 4 == size * 4 ? 0 : hB[u] + 4);
      hB[u] = adv ? nh : dumB;
      pendBits |= hB[u] ^ dumB;
    }
    if (ballot64(pendBits != 0) == 0ull) break;
    if (probe >= size) { atomicOr(err, ERRF_TABLE_FULL); break; }
  }
  return claimed;
}

// ------------------------------------------------------------------------------------------------
// Numeric accumulation.  Measured on gfx950 (tools/micro/lds_atomics.hip): ds_add_f32 costs ~3 cycles PER ACTIVE LANE
// (195 cycles for a full wave, and lanes parked on a dummy address count as active), while ds_cmpst b32/b64 and plain
// reads cost <= 26 cycles per wave instruction.  So the tables of the numeric kernels hold (key, value) PAIRS in one
// 64-bit word and a product that meets an empty slot deposits key AND value with a single 64-bit CAS -- on these
// matrices 9 out of 10 products are the first of their column.  Only a product that finds its key already present
// needs a float add, issued under the EXEC mask (cost = 3 cycles x the few lanes that need it).
// ------------------------------------------------------------------------------------------------
typedef unsigned long long slot_t;                       // low half: key (column), high half: value bits
constexpr slot_t EMPTY_SLOT = 0x00000000FFFFFFFFull;      // {EMPTY_KEY, 0.0f}
constexpr slot_t DUMMY_SLOT = 0x0000000080000000ull;      // {DUMMY_KEY, 0.0f}: what the dummy words hold
__device__ __forceinline__ slot_t make_slot(int col, float v) {
  return (slot_t)(unsigned)col | ((slot_t)__float_as_uint(v) << 32);
}
__device__ __forceinline__ int slot_key(slot_t sl) { return (int)(unsigned)sl; }
__device__ __forceinline__ float slot_val(slot_t sl) { return __uint_as_float((unsigned)(sl >> 32)); }
__device__ __forceinline__ float* slot_val_ptr(slot_t* tab, unsigned i) { return reinterpret_cast<float*>(tab + i) + 1; }

// one product per lane, divergent callers (small-row kernels)
__device__ __forceinline__ void hash_accum(slot_t* tab, int size, int shift, int c, float v, int* err) {
  unsigned h = ((unsigned)c * 2654435761u) >> shift;
  const unsigned mask = (unsigned)size - 1u;
  const slot_t mine = make_slot(c, v);
  for (int probe = 0; probe < size; ++probe) {
    const slot_t old = atomicCAS(&tab[h], EMPTY_SLOT, mine);
    if (old == EMPTY_SLOT) return;
    if (slot_key(old) == c) { atomicAdd(slot_val_ptr(tab, h), v); return; }
    h = (h + 1u) & mask;
  }
  atomicOr(err, ERRF_TABLE_FULL);
}

// U products per lane in lock step, wave-uniform control flow.  Lanes without work aim their CAS at a private
// 8-byte dummy (a CAS costs the same with any lane count; the float add below does not, hence its EXEC mask).
// (Round 3, measured and kept out: adding the repeated columns by a 64-bit CAS on the whole slot {key, value + v} instead of
// ds_add_f32 -- 3 cycles per active lane -- for rounds where most products repeat a column (nnz(C)/P ~ 0.5).  The slot
// content the insert CAS returned has to be carried per product: +2U VGPRs in every numeric kernel.  Web-graph surrogate:
// k_num_hash<1,*> 0.308 -> 0.478 ms; headline matrix 0.293 -> 0.366 ms.  profiles/README.md, round 3.)
template <bool POW2 = true, int U>
__device__ __forceinline__ void hash_accum_multi(slot_t* tab, int size, int shift, const bool (&act)[U],
                                                 const int (&col)[U], const float (&val)[U], slot_t* dummy, int* err) {
  char* const base = reinterpret_cast<char*>(tab);
  const int dumB = (int)(reinterpret_cast<char*>(dummy) - base);
  const int maskB = size * 8 - 1, sizeB = size * 8;
  int hB[U], stepB[U], dupB[U];                   // byte offsets; dumB = "done" / "no repeated column"
  slot_t mine[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const unsigned hv = (unsigned)col[u] * 2654435761u;
    const unsigned h = POW2 ? hv >> shift : __umulhi(hv, (unsigned)size);
    // tables of 1024*k slots (k <= 17): double hashing with a prime step > 17, coprime with every such size
    stepB[u] = POW2 ? 0 : (int)((0x2f2b29251f1d1713ull >> (((hv >> 7) & 7u) * 8u)) & 0xffu) * 8;
    hB[u] = act[u] ? (int)(h * 8u) : dumB;
    dupB[u] = dumB;
    mine[u] = make_slot(col[u], val[u]);
  }
  int probe = 0;
  for (;;) {                                        // first round unconditional: the col and value gathers stay together
    slot_t old[U];
#pragma unroll
    for (int u = 0; u < U; ++u) old[u] = atomicCAS(reinterpret_cast<slot_t*>(base + hB[u]), EMPTY_SLOT, mine[u]);
    ++probe;
    int pendBits = 0;                               // (one OR-ed word and one compare instead of a ballot per product)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool pend = hB[u] != dumB;
      const bool same = pend && slot_key(old[u]) == col[u];
      const bool adv = pend && old[u] != EMPTY_SLOT && slot_key(old[u]) != col[u];
      dupB[u] = same ? hB[u] : dupB[u];
      int nh;
      if (POW2) nh = (hB[u] + probe * 8) & maskB;            // triangular steps
      else { nh = hB[u] + stepB[u]; nh = nh >= sizeB ? nh - sizeB : nh; }
      hB[u] = adv ? nh : dumB;
      pendBits |= hB[u] ^ dumB;
    }
    if (ballot64(pendBits != 0) == 0ull) break;
    if (probe >= size) { atomicOr(err, ERRF_TABLE_FULL); break; }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (dupB[u] != dumB) atomicAdd(reinterpret_cast<float*>(base + dupB[u] + 4), val[u]);
}

// float add into an LDS word by read + 32-bit CAS (retry on interference): ~2 cheap LDS ops instead of a
// ds_add_f32 over a full wave.  U per lane in lock step; lanes without work aim at a private dummy.
template <int U>
__device__ __forceinline__ void lds_fadd_multi(float* acc, const int (&idx)[U], const bool (&ok)[U], const float (&v)[U],
                                               int* dummy) {
  int* ia = reinterpret_cast<int*>(acc);
  int old[U];
  bool pend[U];
#pragma unroll
  for (int u = 0; u < U; ++u) { pend[u] = ok[u]; old[u] = ia[ok[u] ? idx[u] : 0]; }
  for (;;) {
    int got[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      got[u] = atomicCAS(pend[u] ? &ia[idx[u]] : dummy, old[u], __float_as_int(__int_as_float(old[u]) + v[u]));
    bool more = false;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      pend[u] = pend[u] && got[u] != old[u];
      old[u] = got[u];
      more = more || pend[u];
    }
    if (ballot64(more) == 0ull) break;
  }
}

// The R rounds of a trip (gathered together: one memory round trip) are INSERTED CH rounds at a time: in a lock-step probe
// loop every round of the trip issues its CAS in every iteration until the longest chain among ALL its products has ended
// (R = 8: the longest of 512 chains), so R/CH short loops issue fewer instructions than one long one, and the first of
// them starts as soon as ITS gathers have landed.  Round 4, medians of 4 processes per arm: the wave-per-row kernels (R up
// to 8) with CH = 4 / 2 / 1: symbolic 0.195 -> 0.189 / 0.177 / 0.172 ms, numeric 0.304 -> 0.298 / 0.289 / 0.284 (web
// surrogate numeric 0.296 -> 0.280 at CH = 1); the multi-wave kernels (trips of 2 rounds) LOSE 2-4 % with CH = 1 and
// keep their one loop.  CH <= 0: the whole trip in one loop.
// (trips of 4 rounds inserted 2 at a time in the multi-wave kernels: no change; of 8: slower.)
template <int NW> struct InsChunk { static constexpr int value = NW == 1 ? 1 : 0; };
template <int CH, bool RH = false, int R>
__device__ __forceinline__ int hash_insert_chunked(int* keys, int size, int shift, const bool (&act)[R], const int (&col)[R],
                                                   int* dummy, int* err, bool (*rehit)[R] = nullptr) {
  if constexpr (CH <= 0 || CH >= R) return hash_insert_multi<true, RH>(keys, size, shift, act, col, dummy, err, rehit);
  else {
    int claimed = 0;
#pragma unroll
    for (int c0 = 0; c0 < R; c0 += CH) {
      bool a_[CH]; int c_[CH]; bool r_[CH];
#pragma unroll
      for (int u = 0; u < CH; ++u) { a_[u] = c0 + u < R ? act[c0 + u < R ? c0 + u : 0] : false; c_[u] = col[c0 + u < R ? c0 + u : 0]; r_[u] = false; }
      if (!(CH == 1 && ballot64(a_[0]) == 0ull))                 // (else: a round past the end of the group -- 5 rounds run as 6, 7 as 8)
        claimed += hash_insert_multi<true, RH>(keys, size, shift, a_, c_, dummy, err, RH ? &r_ : nullptr);
      if constexpr (RH) {
#pragma unroll
        for (int u = 0; u < CH; ++u) if (c0 + u < R) (*rehit)[c0 + u] = r_[u];
      }
    }
    return claimed;
  }
}
template <int CH, int R>
__device__ __forceinline__ void hash_accum_chunked(slot_t* tab, int size, int shift, const bool (&act)[R], const int (&col)[R],
                                                   const float (&val)[R], slot_t* dummy, int* err) {
  if constexpr (CH <= 0 || CH >= R) hash_accum_multi(tab, size, shift, act, col, val, dummy, err);
  else {
#pragma unroll
    for (int c0 = 0; c0 < R; c0 += CH) {
      bool a_[CH]; int c_[CH]; float v_[CH];
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const int i = c0 + u < R ? c0 + u : 0;
        a_[u] = c0 + u < R ? act[i] : false; c_[u] = col[i]; v_[u] = val[i];
      }
      if (CH == 1 && ballot64(a_[0]) == 0ull) continue;
      hash_accum_multi(tab, size, shift, a_, c_, v_, dummy, err);
    }
  }
}

// slot-table clear, two slots per lane and instruction
__device__ __forceinline__ void clear_slots(slot_t* tab, int size, int tid, int nthreads) {
  for (int i = tid * 2; i < size; i += nthreads * 2) *reinterpret_cast<ulonglong2*>(tab + i) = make_ulonglong2(EMPTY_SLOT, EMPTY_SLOT);
}

// table clear, four slots per lane and instruction (sizes are multiples of 4; arrays 16-byte aligned)
__device__ __forceinline__ void clear_table(int* keys, float* vals, int size, int tid, int nthreads) {
  const int4 ek = make_int4(EMPTY_KEY, EMPTY_KEY, EMPTY_KEY, EMPTY_KEY);
  const float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = tid * 4; i < size; i += nthreads * 4) {
    *reinterpret_cast<int4*>(keys + i) = ek;
    if (vals) *reinterpret_cast<float4*>(vals + i) = zv;
  }
}

// One wave emits the occupied slots [base, base+per) of a finished table: slots into registers, one LDS atomic for
// the wave's share of the output range [outLo, outHi), stores from the registers (64 consecutive positions a step).
template <int MAXSTEPS>
__device__ __forceinline__ void emit_claimed(const slot_t* tab, int base, int per, int* emitted,
                                             int outLo, int outHi, int* __restrict__ JC, float* __restrict__ C) {
  const int lane = lane_id();
  slot_t sl[MAXSTEPS];
  int cnt = 0;
#pragma unroll
  for (int sidx = 0; sidx < MAXSTEPS; ++sidx) {
    sl[sidx] = sidx * WAVE < per ? tab[base + sidx * WAVE + lane] : EMPTY_SLOT;
    cnt += __popcll(ballot64(slot_key(sl[sidx]) != EMPTY_KEY));
  }
  int pos = 0;
  if (lane == 0) pos = atomicAdd(emitted, cnt);
  pos = __builtin_amdgcn_readfirstlane(pos);
  // positions relative to the row: one small 32-bit offset serves both output arrays (uniform base + offset stores)
  int* const JCrow = JC + outLo;
  float* const Crow = C + outLo;
  const unsigned lim = (unsigned)(outHi - outLo);
#pragma unroll
  for (int sidx = 0; sidx < MAXSTEPS; ++sidx) {
    const bool occ = slot_key(sl[sidx]) != EMPTY_KEY;
    const unsigned long long mk = ballot64(occ);
    const unsigned o = (unsigned)(pos + mask_rank(mk));
    if (occ && o < lim) { st_out(JCrow + o, slot_key(sl[sidx])); st_out(Crow + o, slot_val(sl[sidx])); }
    pos += __popcll(mk);
  }
}

// ------------------------------------------------------------------------------------------------
// R-MCL row rule (CPU: nlibs/tools/util.cc:4-69; reference GPU: nlibs/gpus/dutil.cuh:8-80): inflate (square), max,
// sum, thresh = clamp(0.9*avg*(1-2(max-avg)), 1e-7, max), keep v >= thresh, divide the kept values by their sum.
// Written once for both value types V = float, double (the reference's QValue); what differs by type is the threshold's
// arithmetic, how one value crosses lanes, and how a row's table is laid out in LDS (RowTab<V>).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rmcl_threshold(float avg, float mx) {
  float ret = (float)(0.90 * avg * (1 - 2 * (mx - avg)));       // same promotions as computeThreshold (util.cc:4-9)
  ret = (float)((ret > 1.0e-7) ? ret : 1.0e-7);
  ret = (ret > mx) ? mx : ret;
  return ret;
}
__device__ __forceinline__ double rmcl_threshold(double avg, double mx) {
  double ret = 0.90 * avg * (1 - 2 * (mx - avg));               // computeThreshold with QValue = double: nothing to promote
  ret = (ret > 1.0e-7) ? ret : 1.0e-7;
  ret = (ret > mx) ? mx : ret;
  return ret;
}
__device__ __forceinline__ float rmcl_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double rmcl_max(double a, double b) { return fmax(a, b); }

// one value across lanes: by DPP control CTRL inside a 16-lane row, or read from lane l.  A float is one 32-bit move; a
// double travels as its two halves (gfx950 has no 64-bit DPP operand for these controls, and __shfl_xor of a double is two
// ds_bpermute_b32 plus the address VALU and a wait on the LDS queue, which the fused epilogues read their tables through).
template <int CTRL> __device__ __forceinline__ float lane_dpp(float v) {
  return __int_as_float(SMF_DPP(__float_as_int(v), CTRL, 0xf, 0));
}
template <int CTRL> __device__ __forceinline__ double lane_dpp(double v) {
  const int lo = SMF_DPP(__double2loint(v), CTRL, 0xf, 0), hi = SMF_DPP(__double2hiint(v), CTRL, 0xf, 0);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float lane_read(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ double lane_read(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// all-reduce inside the L lanes that share a row (L = 16: one DPP row; L = 64: the wave).  DPP butterflies (xor 1, xor 2,
// half-row mirror, row mirror): four VALU steps for 16 lanes and no LDS round trip -- a ds_bpermute chain here costs more
// than the whole product walk of a 100-product row.  64 lanes: the four row results are combined in a fixed order.
template <int L, class V, class Op>
__device__ __forceinline__ V rowL_allreduce(V v, Op op) {
  static_assert(L == 16 || L == 64, "16-lane groups or whole waves");
  v = op(v, lane_dpp<0xB1>(v));                       // quad_perm [1,0,3,2]
  v = op(v, lane_dpp<0x4E>(v));                       // quad_perm [2,3,0,1]
  v = op(v, lane_dpp<0x141>(v));                      // row_half_mirror
  v = op(v, lane_dpp<0x140>(v));                      // row_mirror
  if (L == 64) {
    const V r0 = lane_read(v, 0), r1 = lane_read(v, 16), r2 = lane_read(v, 32), r3 = lane_read(v, 48);
    v = op(op(r0, r1), op(r2, r3));
  }
  return v;
}
template <int L, class V> __device__ __forceinline__ V rowL_sum(V v) { return rowL_allreduce<L>(v, [](V a, V b) { return a + b; }); }
template <int L, class V> __device__ __forceinline__ V rowL_max(V v) { return rowL_allreduce<L>(v, [](V a, V b) { return rmcl_max(a, b); }); }
// this group's 16 (or all 64) bits of a wave-wide lane mask
template <int L>
__device__ __forceinline__ unsigned long long group_mask(unsigned long long mk, int gl) {
  return L == 64 ? mk : ((mk >> (lane_id() - gl)) & 0xffffull);
}

// A finished row's slots in LDS, by value type: a view of pointers only, everything inlines to what the kernels did by hand.
//   float   one packed 64-bit slot per entry (make_slot): a product that meets an empty slot deposits both with one CAS
//   double  int keys claimed by CAS + double values accumulated by atomicAdd: (column, double) does not fit one CAS
// at(i) reads slot i once for key() and val(), empty() is what a cleared slot reads as; put() writes entry i of a plain
// list; accum() adds a product to the hash table.
// BOUND: a store that takes an entry from the row's swept slots to C is checked against the row's length (store_ok).
// Nothing is stored past it in a correct run (the symbolic pass counted the same columns); the check only keeps a count
// mismatch, which raises ERRF_COUNT_MISMATCH either way, from touching the next row.  On for double.  Off for float: with
// it, nine of the sixteen fused float kernels take 2 more VGPRs and all of them, the headline path's k_num_g16 included,
// more code, and the fused float kernels of the R-MCL loop measured about 2 % slower, for a case the error word already
// reports (the same split as k_rmcl_compact's BOUND; figures in profiles/README.md).
template <class V> struct RowTab;
template <> struct RowTab<float> {
  typedef float value_type;
  static constexpr bool BOUND = false;
  struct Entry {                                      // the slot as loaded: one 64-bit read serves key and value
    slot_t sv;
    __device__ __forceinline__ int key() const { return slot_key(sv); }
    __device__ __forceinline__ float val() const { return slot_val(sv); }
  };
  slot_t* tab;
  __device__ __forceinline__ Entry at(int i) const { return {tab[i]}; }
  __device__ __forceinline__ static Entry empty() { return {EMPTY_SLOT}; }
  __device__ __forceinline__ void clear(int i) const { tab[i] = EMPTY_SLOT; }
  __device__ __forceinline__ void put(int i, int col, float v) const { tab[i] = make_slot(col, v); }
  __device__ __forceinline__ void accum(int size, int shift, int col, float v, int* err) const {
    hash_accum(tab, size, shift, col, v, err);
  }
};
template <> struct RowTab<double> {
  typedef double value_type;
  static constexpr bool BOUND = true;
  struct Entry {
    int k;
    double v;
    __device__ __forceinline__ int key() const { return k; }
    __device__ __forceinline__ double val() const { return v; }
  };
  int* keys;
  double* vals;
  __device__ __forceinline__ Entry at(int i) const { return {keys[i], vals[i]}; }
  __device__ __forceinline__ static Entry empty() { return {EMPTY_KEY, 0.0}; }
  __device__ __forceinline__ void clear(int i) const { keys[i] = EMPTY_KEY; vals[i] = 0.0; }
  __device__ __forceinline__ void put(int i, int col, double v) const { keys[i] = col; vals[i] = v; }
  __device__ __forceinline__ void accum(int size, int shift, int col, double v, int* err) const {
    bool isnew;
    atomicAdd(&vals[hash_insert(keys, size, shift, col, &isnew, err)], v);
  }
};
// the LDS behind a view of N slots
template <class V, int N> struct RowTabMem;
template <int N> struct RowTabMem<float, N> {
  slot_t tab[N];
  __device__ __forceinline__ RowTab<float> view() { return {tab}; }
};
template <int N> struct RowTabMem<double, N> {
  double vals[N];
  int keys[N];
  __device__ __forceinline__ RowTab<double> view() { return {keys, vals}; }
};
// may entry `o` of a row of `want` entries be stored?  want < 0 (length unknown, see prune_emit_group) bounds nothing.
template <class Tab>
__device__ __forceinline__ bool store_ok(int o, int want) { return !Tab::BOUND || (unsigned)o < (unsigned)want; }
// ... and how many of `kept` entries were stored
template <class Tab>
__device__ __forceinline__ int stored_count(int kept, int want) { return Tab::BOUND && want >= 0 ? min(kept, want) : kept; }

// Fused expansion + prune (hip_rmcl_expand_prune): the row rule applied to a finished row that still sits in LDS, so
// that only the KEPT entries (about a quarter of an R-MCL product) ever reach HBM.  They are written, normalised, to
// the FRONT of the row's range of the scratch arrays, their count to cnt[row]; k_rmcl_move then packs the rows.
// The slots hold either a hash table (occupied = key set) or the plain list of the row's `want` products (expanded rows).
// L lanes share the row (a 16-lane group or a whole wave) and sweep slots [0, per), per a multiple of L.
// want < 0: the number of distinct columns is not known beforehand (no symbolic pass ran), the occupied slots are counted;
// the row's range then holds all its products, so no store needs a bound (store_ok).
// Returns the count of kept entries stored; *nocc = occupied slots.
template <int L, class Tab>
__device__ __forceinline__ int prune_emit_group(Tab t, int per, int want, bool byKey, bool live, int gl, int* __restrict__ JCrow,
                                                typename Tab::value_type* __restrict__ Crow, int* nocc) {
  typedef typename Tab::value_type V;
  V mx = V(0), sum = V(0);
  int n = 0;
  for (int i0 = 0; i0 < per; i0 += L) {
    const auto sv = t.at(i0 + gl);
    const bool occ = live && (byKey ? sv.key() != EMPTY_KEY : i0 + gl < want);
    const V c = sv.val(), v = occ ? c * c : V(0);
    mx = rmcl_max(mx, v);
    sum += v;
    n += __popcll(group_mask<L>(ballot64(occ), gl));
  }
  mx = rowL_max<L>(mx);
  sum = rowL_sum<L>(sum);
  *nocc = n;
  const V th = rmcl_threshold(sum / (V)(want >= 0 ? want : n), mx);
  V ks = V(0);
  for (int i0 = 0; i0 < per; i0 += L) {
    const auto sv = t.at(i0 + gl);
    const bool occ = live && (byKey ? sv.key() != EMPTY_KEY : i0 + gl < want);
    const V c = sv.val(), v = c * c;
    ks += (occ && v >= th) ? v : V(0);
  }
  ks = rowL_sum<L>(ks);
  const V inv = V(1) / ks;                            // one division per row; v*inv is within an ulp of v/ks,
  int pos = 0;                                        // except v == ks (the row keeps one entry): v/ks is 1.0, stored as such
  for (int i0 = 0; i0 < per; i0 += L) {
    const auto sv = t.at(i0 + gl);
    const bool occ = live && (byKey ? sv.key() != EMPTY_KEY : i0 + gl < want);
    const V c = sv.val(), v = c * c;
    const bool keep = occ && v >= th;
    const unsigned long long gm = group_mask<L>(ballot64(keep), gl);
    if (keep) {
      const int o = pos + __popcll(gm & ((1ull << gl) - 1ull));
      if (store_ok<Tab>(o, want)) { st_out(JCrow + o, sv.key()); st_out(Crow + o, v == ks ? V(1) : v * inv); }
    }
    pos += __popcll(gm);
  }
  return stored_count<Tab>(pos, want);
}

// The same for a block of NW waves on a hash table.  One sweep of the table: every thread takes its MAXSTEPS slots in one
// unrolled loop (the loads overlap; three dependent sweeps of a 4096-slot table cost more than the product walk of its row)
// and keeps key and squared value in registers, -1 marking an empty slot (never >= a threshold).  Partials are combined in wave
// order by every thread, so the threshold, the kept sum and the places of the kept entries (wave by wave, step by step,
// lane by lane) do not depend on timing.
// Which slot a thread holds at a step is the layout's: slot(s), has(s) = that slot lies inside the table, live(s) = step s is
// worth running at all (uniform over the block; a step that is not live is skipped throughout).
//   WaveSegments     wave w owns slots [w*per, w*per+per), per a multiple of 64: a wave's kept entries are neighbours in
//                    the table (k_num_hash, whose table is at most twice its steps: the empty steps are swept like the rest)
//   BlockStrided<NT> step s is slots [s*NT, s*NT+NT) of a table of `size` slots, any power of two from 64 on
//                    (k_num64_rows, whose table is sized by the row: most rows need few of the steps)
struct WaveSegments {
  int per;
  __device__ __forceinline__ int slot(int s) const { return (threadIdx.x >> 6) * per + s * WAVE + lane_id(); }
  __device__ __forceinline__ bool has(int s) const { return s * WAVE < per; }
  __device__ __forceinline__ bool live(int) const { return true; }
};
template <int NT> struct BlockStrided {
  int size;
  __device__ __forceinline__ int slot(int s) const { return s * NT + threadIdx.x; }
  __device__ __forceinline__ bool has(int s) const { return slot(s) < size; }
  __device__ __forceinline__ bool live(int s) const { return s * NT < size; }
};
template <class V, int NW> struct PruneShared { V mx[NW], sum[NW], ks[NW]; int occ[NW], kc[NW]; };

template <int NW, int MAXSTEPS, class Tab, class Lay>
__device__ __forceinline__ void prune_emit_block(Tab t, Lay lay, int want, PruneShared<typename Tab::value_type, NW>& ps,
                                                 int* __restrict__ JCrow, typename Tab::value_type* __restrict__ Crow,
                                                 int* __restrict__ cntRow, int* __restrict__ err) {
  typedef typename Tab::value_type V;
  const int lane = lane_id(), w = threadIdx.x >> 6;
  int k[MAXSTEPS];
  V v[MAXSTEPS];                                      // squared value; -1 marks an empty slot (never >= a threshold)
  V mx = V(0), sum = V(0);
  int n = 0;
#pragma unroll
  for (int sidx = 0; sidx < MAXSTEPS; ++sidx) {
    const typename Tab::Entry sv = lay.has(sidx) ? t.at(lay.slot(sidx)) : Tab::empty();
    k[sidx] = sv.key();
    v[sidx] = V(-1);                                  // (a step that is not live holds nothing)
    if (lay.live(sidx)) {
      const bool occ = sv.key() != EMPTY_KEY;
      v[sidx] = occ ? sv.val() * sv.val() : V(-1);
      mx = rmcl_max(mx, v[sidx]);
      sum += occ ? v[sidx] : V(0);
      n += __popcll(ballot64(occ));
    }
  }
  mx = rowL_max<64>(mx);
  sum = rowL_sum<64>(sum);
  if (lane == 0) { ps.mx[w] = mx; ps.sum[w] = sum; ps.occ[w] = n; }
  __syncthreads();
  mx = V(0); sum = V(0); n = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) { mx = rmcl_max(mx, ps.mx[i]); sum += ps.sum[i]; n += ps.occ[i]; }
  const V th = rmcl_threshold(sum / (V)(want >= 0 ? want : n), mx);
  V ks = V(0);
  int kc = 0;                                         // kept by this wave (wave-uniform)
#pragma unroll
  for (int sidx = 0; sidx < MAXSTEPS; ++sidx) {
    if (lay.live(sidx)) {
      const bool keep = v[sidx] >= th;
      ks += keep ? v[sidx] : V(0);
      kc += __popcll(ballot64(keep));
    }
  }
  ks = rowL_sum<64>(ks);
  if (lane == 0) { ps.ks[w] = ks; ps.kc[w] = kc; }
  __syncthreads();
  ks = V(0);
  int pos = 0, total = 0;                             // this wave's first place: the waves before it, in wave order
#pragma unroll
  for (int i = 0; i < NW; ++i) { ks += ps.ks[i]; pos += i < w ? ps.kc[i] : 0; total += ps.kc[i]; }
  const V inv = V(1) / ks;                            // one division per row; v*inv is within an ulp of v/ks (v == ks: 1.0, as above)
#pragma unroll
  for (int sidx = 0; sidx < MAXSTEPS; ++sidx) {
    if (lay.live(sidx)) {
      const bool keep = v[sidx] >= th;
      const unsigned long long mk = ballot64(keep);
      if (keep) {
        const int o = pos + mask_rank(mk);
        if (store_ok<Tab>(o, want)) { st_out(JCrow + o, k[sidx]); st_out(Crow + o, v[sidx] == ks ? V(1) : v[sidx] * inv); }
      }
      pos += __popcll(mk);
    }
  }
  if (threadIdx.x == 0) {
    *cntRow = stored_count<Tab>(total, want);
    if (want >= 0 && n != want) atomicOr(err, ERRF_COUNT_MISMATCH);
  }
}

// ------------------------------------------------------------------------------------------------
// K1  per-row product count + bin id + per-block bin histogram            (mindex2: gcomputeFlops)
// One wave owns 64 consecutive rows.  Phase 1: every lane walks the first FL_SHORT entries of its own
// row (87% of the rows of a power-law matrix end there).  Phase 2: rows that are longer are finished by
// the whole wave, 64 entries per step, so a 4095-entry row costs 64 steps, not 4095.
// ------------------------------------------------------------------------------------------------
constexpr int K1_THREADS = 256;
constexpr int FL_SHORT = 8;

// K1a: per A entry, where its B row starts and how long it is -- ONE coalesced record per entry.  Every later kernel
// stages a row from these records instead of walking the dependent chain JA -> IB (two memory round trips per row in
// every symbolic and numeric kernel, and three random IB gathers per entry over the whole pipeline instead of one).
__global__ __launch_bounds__(256) void k_entry_lens(int nnzA, const int* __restrict__ JA, const int* __restrict__ IB,
                                                     int2* __restrict__ SBL) {
  for (int p = blockIdx.x * 256 + threadIdx.x; p < nnzA; p += gridDim.x * 256) {
    const int j = JA[p];
    const int2 be = make_int2(IB[j], IB[j + 1]);
    SBL[p] = make_int2(be.x, max(be.y - be.x, 0));
  }
}

// inclusive +-scan of 64-bit values over the wave (both halves travel through the same DPP moves)
__device__ __forceinline__ unsigned long long wave_incl_add_u64(unsigned long long v) {
#define SMF_DPP64_STEP(ctrl, rowmask)                                                                          \
  {                                                                                                             \
    const unsigned lo = (unsigned)SMF_DPP((int)(unsigned)v, ctrl, rowmask, 0);                                   \
    const unsigned hi = (unsigned)SMF_DPP((int)(unsigned)(v >> 32), ctrl, rowmask, 0);                           \
    v += ((unsigned long long)hi << 32) | lo;                                                                   \
  }
  SMF_DPP64_STEP(0x111, 0xf) SMF_DPP64_STEP(0x112, 0xf) SMF_DPP64_STEP(0x114, 0xf) SMF_DPP64_STEP(0x118, 0xf)
  SMF_DPP64_STEP(0x142, 0xa) SMF_DPP64_STEP(0x143, 0xc)
#undef SMF_DPP64_STEP
  return v;
}

// K1: one wave owns 64 consecutive rows = ONE contiguous range of A entries.  The wave walks that range 64 entries at a
// time, fully coalesced: entry -> column -> {B-row start, length} (the record of K1a, written here when SBL != nullptr:
// the two kernels are one), an inclusive scan of the 64 lengths, and every row takes the difference of the scan values
// at its two ends (two cross-lane reads).  No per-lane walk of its own row (64 different lines per load) and no serial
// finishing of long rows.  CHK chunks are in flight together (their JA -> IB chains are independent).
// EXTENTS: B is NOT packed -- row j is [IBse[j].x, IBse[j].y) (the pruned matrix of the previous R-MCL
// iteration, left where the epilogues wrote it: hip_gpuRmclIter_device; k_zip_extents makes the pairs so that the
// gather stays ONE 8-byte load per entry).  Everything downstream reads the records.
template <bool EXTENTS>
__global__ __launch_bounds__(K1_THREADS) void k_row_flops(
    int m, const int* __restrict__ IA, const int* __restrict__ JA, const int* __restrict__ IB,
    const int2* __restrict__ IBse, int2* __restrict__ SBL, int sblCap,
    int* __restrict__ rowFlops, unsigned char* __restrict__ binId, int* __restrict__ blockHist,
    unsigned long long* __restrict__ blockP, int* __restrict__ IC) {
  __shared__ int hist[NSLOTS];
  __shared__ unsigned long long psum;
  const int tid = threadIdx.x, lane = lane_id();
  if (tid < NSLOTS) hist[tid] = 0;
  if (tid == 0) psum = 0;
  __syncthreads();
  const int r = blockIdx.x * K1_THREADS + tid;
  const int rs = IA[min(r, m)], re = IA[min(r + 1, m)];      // rows past the end: empty, at the end of the range
  const int s = __builtin_amdgcn_readlane(rs, 0), e = __builtin_amdgcn_readlane(re, 63);
  unsigned long long f = 0;
  constexpr int CHK = 4;
  for (int c0 = s; c0 < e; c0 += CHK * WAVE) {
    int j[CHK];
    int2 be[CHK];
#pragma unroll
    for (int i = 0; i < CHK; ++i) { const int p = c0 + i * WAVE + lane; j[i] = p < e ? JA[p] : -1; }
#pragma unroll
    for (int i = 0; i < CHK; ++i) {
      if (EXTENTS) be[i] = j[i] >= 0 ? IBse[j[i]] : make_int2(0, 0);
      else be[i] = j[i] >= 0 ? make_int2(IB[j[i]], IB[j[i] + 1]) : make_int2(0, 0);
    }
#pragma unroll
    for (int i = 0; i < CHK; ++i) {
      const int cb = c0 + i * WAVE;                           // wave-uniform
      if (cb >= e) break;
      const int len = max(be[i].y - be[i].x, 0);
      if (SBL && j[i] >= 0 && cb + lane < sblCap) SBL[cb + lane] = make_int2(be[i].x, len);
      const unsigned long long incl = wave_incl_add_u64((unsigned long long)(unsigned)len);
      const int a = min(max(rs - cb, 0), WAVE), b = min(max(re - cb, 0), WAVE);   // this row's part of the chunk: [a, b)
      const unsigned long long hiP = __shfl(incl, max(b - 1, 0), WAVE);
      const unsigned long long loP = __shfl(incl, max(a - 1, 0), WAVE);
      if (b > a) f += hiP - (a > 0 ? loP : 0ull);
    }
  }
  int b = -1;
  if (r < m) {
    rowFlops[r] = f > 0x7fffffffULL ? 0x7fffffff : (int)f;
    b = slot_of(f);
    binId[r] = (unsigned char)b;
    if (b <= 1) IC[r] = b;                           // 0 products -> 0 entries, 1 product -> 1 entry
  }
#pragma unroll
  for (int q = 0; q < SLOT_BIG0; ++q) {
    const unsigned long long mk = ballot64(b == q);
    if (lane == 0 && mk) atomicAdd(&hist[q], __popcll(mk));
  }
  if (ballot64(b >= SLOT_BIG0)) {                    // big rows are rare: most waves skip their size classes
    for (int q = SLOT_BIG0; q < NSLOTS; ++q) {
      const unsigned long long mk = ballot64(b == q);
      if (lane == 0 && mk) atomicAdd(&hist[q], __popcll(mk));
    }
  }
  const unsigned long long wsum = wave_sum_u64(f);
  if (lane == 0 && wsum) atomicAdd(&psum, wsum);
  __syncthreads();
  if (tid < NSLOTS) blockHist[(size_t)tid * gridDim.x + blockIdx.x] = hist[tid];   // slot-major
  if (tid == 0) blockP[blockIdx.x] = psum;      // no same-address global atomics: k_bin_scan sums these
}

// ------------------------------------------------------------------------------------------------
// K2  exclusive scan of the per-block histograms, one layout slot per block: blockOff[slot][block] = rows of the slot in
//     the blocks before this one, slotTot[slot] = rows of the slot.  Block 0 also sums blockP into totalP.  A thread
//     holds K2_ITEMS consecutive counts; a tile of 1024 x K2_ITEMS counts is loaded before its first use and scanned
//     with one block scan (16 x nblk counts in NSLOTS blocks, where one block used to walk them wave by wave).
//     The running sums over the slots (slotBase, binPtr) are 16 adds: K3 makes them in its prologue.
// ------------------------------------------------------------------------------------------------
constexpr int K2_THREADS = 1024;
constexpr int K2_ITEMS = 4;
constexpr int K2_TILE = K2_THREADS * K2_ITEMS;

__global__ __launch_bounds__(K2_THREADS) void k_bin_scan(int nblk, const int* __restrict__ blockHist,
                                                          int* __restrict__ blockOff, int* __restrict__ slotTot,
                                                          const unsigned long long* __restrict__ blockP,
                                                          unsigned long long* __restrict__ totalP) {
  __shared__ int wsum[2][K2_THREADS / WAVE];            // (two sets: one barrier per tile)
  __shared__ unsigned long long psum[K2_THREADS / WAVE];
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6, sl = blockIdx.x;
  const int* src = blockHist + (size_t)sl * nblk;
  int* dst = blockOff + (size_t)sl * nblk;
  int run = 0;                                           // rows of the slot in the tiles before this one (block-uniform)
  for (int t0 = 0, it = 0; t0 < nblk; t0 += K2_TILE, it ^= 1) {
    const int base = t0 + tid * K2_ITEMS;
    int v[K2_ITEMS];
    int s = 0;
#pragma unroll
    for (int i = 0; i < K2_ITEMS; ++i) { v[i] = base + i < nblk ? src[base + i] : 0; s += v[i]; }
    const int incl = wave_incl_add(s);
    if (lane == 63) wsum[it][w] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < K2_THREADS / WAVE; ++i) { const int x = wsum[it][i]; tot += x; if (i < w) woff += x; }
    int o = run + woff + incl - s;
#pragma unroll
    for (int i = 0; i < K2_ITEMS; ++i) { if (base + i < nblk) dst[base + i] = o; o += v[i]; }
    run += tot;
  }
  if (tid == 0) slotTot[sl] = run;
  if (sl == 0) {
    unsigned long long p = 0;
    for (int b = tid; b < nblk; b += K2_THREADS) p += blockP[b];
    p = wave_sum_u64(p);
    if (lane == 0) psum[w] = p;
    __syncthreads();
    if (tid == 0) {
      unsigned long long t = 0;
      for (int i = 0; i < K2_THREADS / WAVE; ++i) t += psum[i];
      *totalP = t;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// K3  stable scatter of row ids into their layout slots (rows ascend inside a bin / a size class of the last bin).
//     Prologue: every block turns K2's NSLOTS slot totals into the slots' first positions; block 0 leaves them, and the
//     bins' (binPtr), in the device block for the kernels of the later phases.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(K1_THREADS) void k_scatter_rows(int m, const unsigned char* __restrict__ binId,
                                                             const int* __restrict__ blockOff,
                                                             const int* __restrict__ slotTot,
                                                             int* __restrict__ slotBase, int* __restrict__ binPtr,
                                                             int* __restrict__ rowIds) {
  static_assert(NSLOTS <= WAVE, "one wave scans the slot totals");
  __shared__ int wcnt[K1_THREADS / WAVE][NSLOTS];
  __shared__ int sbase[NSLOTS + 1];
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  if (w == 0) {
    const int incl = wave_incl_add(lane < NSLOTS ? slotTot[lane] : 0);
    if (lane < NSLOTS) sbase[lane + 1] = incl;
    if (lane == 0) sbase[0] = 0;
  }
  const int r = blockIdx.x * K1_THREADS + tid;
  const int b = r < m ? (int)binId[r] : -1;
  int myrank = 0;
#pragma unroll
  for (int q = 0; q < NSLOTS; ++q) {
    const unsigned long long mk = ballot64(b == q);
    if (b == q) myrank = mask_rank(mk);
    if (lane == 0) wcnt[w][q] = __popcll(mk);
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    if (tid <= NSLOTS) slotBase[tid] = sbase[tid];
    if (tid <= NBINS) binPtr[tid] = tid ? sbase[last_slot_of_bin(tid - 1) + 1] : 0;
  }
  if (b >= 0) {
    int off = sbase[b] + blockOff[(size_t)b * gridDim.x + blockIdx.x];
    for (int i = 0; i < w; ++i) off += wcnt[i][b];
    rowIds[off + myrank] = r;
  }
}

// Launch grids of the statically scheduled kernels are multiples of 8 (host: grid8()).
struct XcdRange { int lo, hi, bi, nb; };
__device__ __forceinline__ XcdRange xcd_range(int count) {
  const int x = blockIdx.x & 7;
  XcdRange r;
  r.bi = blockIdx.x >> 3;
  r.nb = gridDim.x >> 3;
  r.lo = (int)((long long)count * x >> 3);
  r.hi = (int)((long long)count * (x + 1) >> 3);
  return r;
}

// ------------------------------------------------------------------------------------------------
// Rows with 1..64 products: 16 lanes per row (4 rows per wave), products flattened over the 16 lanes.
// The old "A entries one after the other" walk costs three dependent memory round trips per A entry;
// here a row costs three in total (JA -> IB -> JB/VB): the row's A entries are staged 16 at a time with a
// 16-lane DPP scan of their B-row lengths, then 16-product rounds find their entry by a 4-step search.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int row16_incl_add(int v) {   // inclusive scan inside each 16-lane DPP row
  v += SMF_DPP(v, 0x111, 0xf, 0);
  v += SMF_DPP(v, 0x112, 0xf, 0);
  v += SMF_DPP(v, 0x114, 0xf, 0);
  v += SMF_DPP(v, 0x118, 0xf, 0);
  return v;
}

template <class V> struct G16Stage { int incl[16]; int off[16]; V aval[16]; };

// the products of one row, 16 A entries staged at a time; f(active, col, a*b, position of the product in the row).
// NEED_VAL = false (the symbolic pass): no value is loaded, staged or multiplied.
template <class V, int U, bool NEED_VAL, class F>
__device__ __forceinline__ void g16_walk(G16Stage<V>& st, int gl, int as, int ae, const int2* __restrict__ SBL,
                                         const V* __restrict__ VA,
                                         const int* __restrict__ JB, const V* __restrict__ VB, F&& f) {
  int rowBase = 0;                                  // products of the chunks before this one
  for (int chunk = as; chunk < ae; chunk += 16) {
    const int ap = chunk + gl;
    int len = 0, bs = 0;
    V a = V(0);
    if (ap < ae) {
      const int2 sbl = SBL[ap];
      bs = sbl.x;
      len = sbl.y;
      if (NEED_VAL) a = VA[ap];
    }
    const int incl = row16_incl_add(len);
    st.incl[gl] = incl;
    st.off[gl] = bs - (incl - len);
    if (NEED_VAL) st.aval[gl] = a;
    wave_lds_sync();
    const int T = st.incl[15];
    for (int r0 = 0; r0 * 16 < T; r0 += U) {
      int p[U], e[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { p[u] = min((r0 + u) * 16 + gl, T - 1); e[u] = 0; }   // past the end: shadow the last product
#pragma unroll
      for (int sft = 8; sft >= 1; sft >>= 1) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int c = e[u] + sft;
          e[u] = st.incl[c - 1] <= p[u] ? c : e[u];
        }
      }
      int col[U];
      V val[U], av[U], vb[U];
      bool act[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {                // straight-line, no branches around the gathers
        act[u] = (r0 + u) * 16 + gl < T;
        const int jb = st.off[e[u]] + p[u];
        col[u] = JB[jb];
        vb[u] = NEED_VAL ? VB[jb] : V(0);
        av[u] = NEED_VAL ? st.aval[e[u]] : V(0);
      }
      __builtin_amdgcn_sched_barrier(0);           // all gathers issued before the first wait
#pragma unroll
      for (int u = 0; u < U; ++u) val[u] = av[u] * vb[u];
#pragma unroll
      for (int u = 0; u < U; ++u) f(act[u], col[u], val[u], rowBase + (r0 + u) * 16 + gl);
    }
    rowBase += T;
    wave_lds_sync();
  }
}

template <int TBL, int U>
__global__ __launch_bounds__(256) void k_sym_g16(const int* __restrict__ binPtr, int bin, int binHi,
                                                  const int* __restrict__ rowIds,
                                                  const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                  const int* __restrict__ JB,
                                                  const int* __restrict__ rowFlops, int* __restrict__ IC,
                                                  int* __restrict__ err) {
  __shared__ int keys[16][TBL];
  __shared__ G16Stage<float> st[16];               // (no value is staged: the type only sizes the unused array)
  const int tid = threadIdx.x, g = tid >> 4, gl = tid & 15;
  const int first = binPtr[bin], count = binPtr[binHi] - first;
  const int iters = (count + 15) / 16;
  // XCD-contiguous schedule: the blocks that share an XCD (blockIdx % 8, guide "Workgroup dispatch") walk ONE contiguous
  // eighth of the bin, so that the B rows its A rows have in common are fetched into that XCD's L2 once, not into all eight
  const XcdRange xr = xcd_range(iters);
  for (int it = xr.lo + xr.bi; it < xr.hi; it += xr.nb) {
    const int q = it * 16 + g;
    const bool live = q < count;
    const int row = live ? rowIds[first + q] : 0;
    const int F = live ? rowFlops[row] : 1;
    const int size = table_size(F, 16, TBL);
    const int shift = 32 - log2_pow2(size);
    for (int i = gl; i < size; i += 16) keys[g][i] = EMPTY_KEY;
    wave_lds_sync();
    int mine = 0;
    if (live) {
      g16_walk<float, U, false>(st[g], gl, IA[row], IA[row + 1], SBL, nullptr, JB, nullptr, [&](bool active, int col, float, int) {
        if (active) {
          bool isnew;
          hash_insert(keys[g], size, shift, col, &isnew, err);
          mine += isnew ? 1 : 0;
        }
      });
    }
    mine = row16_incl_add(mine);
    if (live && gl == 15) IC[row] = mine;
    wave_lds_sync();
  }
}

// PRUNE: 0 plain product; 1 fused R-MCL prune, IC = exact row pointers of the product (symbolic pass ran); 2 fused prune
// WITHOUT a symbolic pass: IC = prefix sums of the rows' product counts (an upper bound of every row; rows of bin 8, which
// these kernels do not see, contribute their exact counts), every row is hashed
// in a table sized by its products and the distinct columns are counted by the epilogue itself (float only).
// V: float or double; the double pipeline (spgemm_f64_device.hpp) launches this kernel for its bins 1-4 with the exact row
// pointers of the float pipeline's symbolic pass.  Two rules hold for both types:
//   * a row kept as a plain list that is longer than the table (cannot happen for rows of these bins: at most 64 products,
//     TBL >= 64 where they go) is cut at the table and raises ERRF_TABLE_FULL;
//   * the stores of the compaction sweeps are bounded by the row's length where the view says so (RowTab<V>::BOUND).
template <class V, int TBL, int U, int PRUNE = 0>
__global__ __launch_bounds__(256) void k_num_g16(const int* __restrict__ binPtr, int bin, int binHi,
                                                  const int* __restrict__ rowIds,
                                                  const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                  const V* __restrict__ VA,
                                                  const int* __restrict__ JB,
                                                  const V* __restrict__ VB,
                                                  const int* __restrict__ IC, int* __restrict__ JC,
                                                  V* __restrict__ C, int* __restrict__ err,
                                                  const int* __restrict__ rowFlops, int* __restrict__ pcnt) {
  static_assert(PRUNE != 2 || std::is_same<V, float>::value, "the fused prune without a symbolic pass is float only");
  typedef RowTab<V> Tab;
  __shared__ RowTabMem<V, TBL> mem[16];        // one table (or plain list) per row of the block
  __shared__ G16Stage<V> st[16];
  const int tid = threadIdx.x, g = tid >> 4, gl = tid & 15;
  const Tab t = mem[g].view();
  const int first = binPtr[bin], count = binPtr[binHi] - first;
  const int iters = (count + 15) / 16;
  // XCD-contiguous schedule: the blocks that share an XCD (blockIdx % 8, guide "Workgroup dispatch") walk ONE contiguous
  // eighth of the bin, so that the B rows its A rows have in common are fetched into that XCD's L2 once, not into all eight
  const XcdRange xr = xcd_range(iters);
  for (int it = xr.lo + xr.bi; it < xr.hi; it += xr.nb) {
    const int q = it * 16 + g;
    const bool live = q < count;
    const int row = live ? rowIds[first + q] : 0;
    const int off = live ? IC[row] : 0;
    const int want = live ? IC[row + 1] - off : 0;
    // rows whose products all hit different columns (want == flops: 93-99 % of the rows this small on a power-law
    // matrix) are EXPANDED: products go straight to their position in the row, no table, no compaction.  The four
    // rows of a wave take the same path (wave-uniform control flow).
    const bool hashRow = live && (PRUNE == 2 || want != rowFlops[row]);
    if (ballot64(hashRow) == 0ull) {
      if (PRUNE) {                                   // the row's products as a plain list in LDS, then the row rule
        if (live) {
          g16_walk<V, U, true>(st[g], gl, IA[row], IA[row + 1], SBL, VA, JB, VB, [&](bool active, int col, V v, int pos) {
            if (active && (unsigned)pos < (unsigned)min(want, TBL)) t.put(pos, col, v);
          });
        }
        wave_lds_sync();
        int nocc;
        const int kept = prune_emit_group<16>(t, (min(want, TBL) + 15) & ~15, min(want, TBL), false, live, gl,
                                              JC + off, C + off, &nocc);
        if (live && gl == 0) { pcnt[row] = kept; if (want > TBL) atomicOr(err, ERRF_TABLE_FULL); }
        wave_lds_sync();
        continue;
      }
      if (live) {
        g16_walk<V, U, true>(st[g], gl, IA[row], IA[row + 1], SBL, VA, JB, VB, [&](bool active, int col, V v, int pos) {
          if (active && (unsigned)pos < (unsigned)want) { st_out(JC + off + pos, col); st_out(C + off + pos, v); }
        });
      }
      continue;
    }
    const int size = table_size(want, 16, TBL);
    const int shift = 32 - log2_pow2(size);
    for (int i = gl; i < size; i += 16) t.clear(i);
    wave_lds_sync();
    if (live) {
      g16_walk<V, U, true>(st[g], gl, IA[row], IA[row + 1], SBL, VA, JB, VB, [&](bool active, int col, V v, int) {
        if (active) t.accum(size, shift, col, v, err);
      });
    }
    wave_lds_sync();
    if (PRUNE) {
      int nocc;
      const int kept = prune_emit_group<16>(t, size, PRUNE == 2 ? -1 : want, true, live, gl, JC + off, C + off, &nocc);
      if (live && gl == 0) { pcnt[row] = kept; if (PRUNE == 1 && nocc != want) atomicOr(err, ERRF_COUNT_MISMATCH); }
      wave_lds_sync();
      continue;
    }
    int written = 0;
    for (int i0 = 0; i0 < size; i0 += 16) {
      const auto sv = t.at(i0 + gl);
      const bool occ = live && sv.key() != EMPTY_KEY;
      const unsigned long long mk = ballot64(occ);
      const unsigned gm = (unsigned)(mk >> (lane_id() - gl)) & 0xffffu;
      const int rank = __popc(gm & ((1u << gl) - 1u));
      if (occ && store_ok<Tab>(written + rank, want)) { st_out(JC + off + written + rank, sv.key()); st_out(C + off + written + rank, sv.val()); }
      written += __popc(gm);
    }
    if (live && gl == 0 && written != want) atomicOr(err, ERRF_COUNT_MISMATCH);
    wave_lds_sync();
  }
}

// ------------------------------------------------------------------------------------------------
// Product walk of ONE C row by a block of NW waves.
//
// The row's A entries are staged in groups of 64 (one per lane of the staging wave).  A group splits in two:
//   * entries whose B row has >= LONG_LEN entries ("long": 3 % of the entries, 55-65 % of the products of a power-law
//     matrix) are walked directly: a unit of 64*U consecutive products of ONE B row per wave -- no search, the A value
//     and the B-row base are wave-uniform, the gathers are fully coalesced;
//   * the other entries are flattened: the group's <= 64*63 products are numbered consecutively, a lane finds the entry
//     that owns its product from OWNERSHIP MARKS: bit p of the group's mark words is set when product p is the last one
//     of its entry, so owner(p) = (entries that end before this 64-product round) + popcount(marks below the lane)
//     -- one v_mbcnt pair instead of a six-step binary search through LDS.
// NW > 1: every wave stages one group (no cross-wave scan), one barrier, then the waves take UNITS (a trip of U rounds of
// some group's short products, or 64*U products of a long entry) from one list: the first NW units are dealt, the rest
// claimed from an LDS counter (probe chains make unit times uneven).  f(act[U], col[U], val[U]) is called in wave-uniform
// control flow (val = a*b).
// ------------------------------------------------------------------------------------------------
constexpr int LONG_LEN = WAVE;           // B rows of at least this length are walked by whole waves

// first chunk of A entries fetched ahead of time (wave-per-row kernels prefetch the next row's while they work)
struct PreA { int bs, len; float a; bool valid; };

struct WalkStage1 {                      // one wave per row
  unsigned long long marks[WAVE];        // ownership marks of the staged group (64 entries x <= 63 products)
  int2 rec[WAVE];                        // short entries, compacted: {JB offset of product 0 of the group's numbering, a}
  slot_t dummy[WAVE];                    // one 8-byte word per lane: target of predicated-off atomics
};
template <int NW>
struct WalkStageN {
  unsigned long long marks[NW][WAVE];
  int4 rec[NW][WAVE];                    // short entries from the bottom {off, a, -, -}; long ones from the top {bs, a, len, unit offset}
  unsigned char wpre[NW][WAVE];          // entries of the group that end before round r
  int gT[NW], gNS[NW], gNL[NW], gLU[NW]; // per group: short products, short entries, long entries, long units
  int claim;                             // next unclaimed unit of the chunk
  slot_t dummy[WAVE];                    // shared by the waves: whatever lands there is never read
};
template <int NW> struct WalkSel { typedef WalkStageN<NW> type; };
template <> struct WalkSel<1> { typedef WalkStage1 type; };

struct GroupLanes {                      // what the staging wave keeps in registers about its group
  int bs, len;                           // this lane's entry: B-row start and length
  float a;
  int T, ns;                             // short products / short entries of the group (uniform)
  unsigned long long lmask;              // lanes holding a long entry
  unsigned long long mw;                 // mark word `lane`
  int pexcl;                             // short entries that end before round `lane`
};

template <bool NEED_VAL, int RS, int LONGLEN>
__device__ __forceinline__ GroupLanes stage_group(unsigned long long* marks, char* rec, int ap, int ae,
                                                  const int2* __restrict__ SBL, const float* __restrict__ VA, PreA pre) {
  const int lane = lane_id();
  GroupLanes g;
  g.bs = 0; g.len = 0; g.a = 0.f;
  if (ap < ae) {
    if (pre.valid) { g.bs = pre.bs; g.len = pre.len; g.a = pre.a; }
    else {
      const int2 sbl = SBL[ap];
      g.bs = sbl.x; g.len = sbl.y;
      if (NEED_VAL) g.a = VA[ap];
    }
  }
  const bool isLong = g.len >= LONGLEN;
  const int slen = isLong ? 0 : g.len;
  const bool keep = slen > 0;
  const unsigned long long km = ballot64(keep);
  g.lmask = ballot64(isLong);
  const int incl = wave_incl_add(slen);
  g.T = __builtin_amdgcn_readlane(incl, 63);
  g.ns = __popcll(km);
  marks[lane] = 0ull;
  wave_lds_sync();
  if (keep) {
    *reinterpret_cast<int2*>(rec + mask_rank(km) * RS) = make_int2(g.bs - (incl - slen), __float_as_int(g.a));
    const int q = incl - 1;                              // last product of this entry
    if (q < WAVE * WAVE) atomicOr(reinterpret_cast<unsigned*>(marks) + (q >> 5), 1u << (q & 31));
  }
  wave_lds_sync();
  g.mw = marks[lane];
  const int pc = __popcll(g.mw);
  g.pexcl = wave_incl_add(pc) - pc;
  return g;
}

// U rounds of 64 short products of one staged group.  W[u] / base[u]: mark word and entries-before of round r0+u
// (wave-uniform values, in SGPRs or broadcast VGPRs).
template <int U, bool NEED_VAL, int RS, class F>
__device__ __forceinline__ void short_trip(const char* rec, int T, int ns, int r0, const unsigned long long (&W)[U],
                                           const int (&base)[U], const int* __restrict__ JB,
                                           const float* __restrict__ VB, F&& f, int p0row = -1) {
  const int lane = lane_id();
  int col[U];
  float av[U], vb[U], val[U];
  bool act[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {                          // straight-line, no branches around the gathers
    const int p0 = (r0 + u) * WAVE + lane;
    act[u] = p0 < T;
    const int p = min(p0, T - 1);                        // lanes past the end shadow the last product: valid, nearby reads
    int e = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(W[u] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)W[u], (unsigned)base[u]));
    e = min(e, ns - 1);
    const int2 ra = *reinterpret_cast<const int2*>(rec + e * RS);
    const int jb = ra.x + p;
    if (ABL(2)) { col[u] = jb; vb[u] = 1.f; }
    else {
    col[u] = JB[jb];
    vb[u] = NEED_VAL ? VB[jb] : 0.f;
    }
    av[u] = __int_as_float(ra.y);
  }
  __builtin_amdgcn_sched_barrier(0);                     // all 2U gathers are issued before the first of them is waited for
#pragma unroll
  for (int u = 0; u < U; ++u) val[u] = av[u] * vb[u];
  f(act, col, val, p0row);                              // p0row: index of the trip's first product in the row's own
}                                                        // numbering (wave-per-row walk), -1 where there is none

// 64*U consecutive products [s0, s0 + 64U) of one long B row: base, length and A value are wave-uniform
template <int U, bool NEED_VAL, class F>
__device__ __forceinline__ void long_trip(int kb, int kl, float ka, int s0, const int* __restrict__ JB,
                                          const float* __restrict__ VB, F&& f, int p0row = -1) {
  const int lane = lane_id();
  int col[U];
  float vb[U], val[U];
  bool act[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p0 = s0 + u * WAVE + lane;
    act[u] = p0 < kl;
    const int jb = kb + min(p0, kl - 1);
    if (ABL(2)) { col[u] = jb; vb[u] = 1.f; }
    else {
    col[u] = JB[jb];
    vb[u] = NEED_VAL ? VB[jb] : 0.f;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < U; ++u) val[u] = ka * vb[u];
  f(act, col, val, p0row);
}

// wave-uniform R in 1..8 -> compile-time round count (5 runs as 6, 7 as 8): a trip costs what its rounds cost
template <class G>
__device__ __forceinline__ void with_rounds(int R, G&& g) {
  switch (R) {
    case 1: g(std::integral_constant<int, 1>{}); break;
    case 2: g(std::integral_constant<int, 2>{}); break;
    case 3: g(std::integral_constant<int, 3>{}); break;
    case 4: g(std::integral_constant<int, 4>{}); break;
    case 5: case 6: g(std::integral_constant<int, 6>{}); break;
    default: g(std::integral_constant<int, 8>{}); break;
  }
}

// ---- one wave per row (rows of at most 512 products): no long path, the whole group is flattened and ALL its rounds
// are gathered before the first insert -- one memory round trip and one probe sequence per group instead of one per
// pair of rounds (these kernels are bound by the chain of dependent waits of a wave, not by any unit's throughput).
// f is a generic callable: f(act[R], col[R], val[R]) for R in {1,2,3,4,6,8}.
template <int NW, int U, bool NEED_VAL, class F>
__device__ __forceinline__ typename std::enable_if<NW == 1>::type
for_each_product(WalkStage1& st, int as, int ae, const int2* __restrict__ SBL, const float* __restrict__ VA,
                 const int* __restrict__ JB, const float* __restrict__ VB, F&& f,
                 PreA pre = PreA{0, 0, 0.f, false}, int* err = nullptr) {
  const int lane = lane_id();
  int rowBase = 0;                                     // products of the groups before this one
  for (int gb = as; gb < ae; gb += WAVE) {
    const GroupLanes g = stage_group<NEED_VAL, 8, 0x40000000>(st.marks, reinterpret_cast<char*>(st.rec), gb + lane, ae, SBL, VA,
                                                              gb == as ? pre : PreA{0, 0, 0.f, false});
    if (g.T > WAVE * WAVE) {                             // cannot happen for rows of this bin (<= 512 products)
      if (err && lane == 0) atomicOr(err, ERRF_TABLE_FULL);
      continue;
    }
    const int nr = (g.T + WAVE - 1) >> 6;
    const unsigned mlo = (unsigned)g.mw, mhi = (unsigned)(g.mw >> 32);
    for (int r0 = 0; r0 < nr; r0 += 8) {
      with_rounds(min(8, nr - r0), [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        unsigned long long W[R];
        int base[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
          const int r = min(r0 + u, WAVE - 1);
          W[u] = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)mlo, r) |
                 ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)mhi, r) << 32);
          base[u] = __builtin_amdgcn_readlane(g.pexcl, r);
        }
        short_trip<R, NEED_VAL, 8>(reinterpret_cast<const char*>(st.rec), g.T, g.ns, r0, W, base, JB, VB, f, rowBase + r0 * WAVE);
      });
    }
    rowBase += g.T;
  }
}

// ---- NW waves per row
// num != nullptr: every product gets its index in a dense numbering of the ROW (chunk by chunk: the short products of the
// chunk's groups first, then its long entries one after the other) and the callback receives the index of the unit's
// first product -- what the expansion of duplicate-free rows needs to store products without a table.
template <int NW>
struct WalkNumber { int lpro[NW][WAVE]; int gLP[NW]; };   // per long entry: products of the group's earlier long entries; their sum
static_assert(sizeof(WalkNumber<8>) <= 4096 * sizeof(unsigned long long), "lives in the (idle) hash table of an expanded row");

template <int NW, int U, bool NEED_VAL, class F>
__device__ __forceinline__ typename std::enable_if<(NW > 1)>::type
for_each_product(WalkStageN<NW>& st, int as, int ae, const int2* __restrict__ SBL, const float* __restrict__ VA,
                 const int* __restrict__ JB, const float* __restrict__ VB, F&& f,
                 PreA pre = PreA{0, 0, 0.f, false}, int* err = nullptr, WalkNumber<NW>* num = nullptr) {
  (void)err;
  int chunkBase = 0;                                     // products of the chunks before this one (numbering only)
  static_assert(NW <= 16, "the unit table of a chunk lives in the first 16 lanes");
  constexpr int K = WAVE * NW;
  constexpr int UP = WAVE * U;                           // products per unit
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  (void)pre;
  for (int chunk = as; chunk < ae; chunk += K) {
    // ---- wave w stages group w of the chunk
    {
      const GroupLanes g = stage_group<NEED_VAL, 16, LONG_LEN>(st.marks[w], reinterpret_cast<char*>(st.rec[w]), chunk + tid, ae, SBL, VA,
                                                     PreA{0, 0, 0.f, false});
      const bool isLong = (g.lmask >> lane) & 1ull;
      const int units = isLong ? (g.len + UP - 1) / UP : 0;
      const int uincl = wave_incl_add(units);
      if (isLong) st.rec[w][WAVE - 1 - mask_rank(g.lmask)] = make_int4(g.bs, __float_as_int(g.a), g.len, uincl - units);
      if (num) {
        const int lincl = wave_incl_add(isLong ? g.len : 0);
        if (isLong) num->lpro[w][mask_rank(g.lmask)] = lincl - g.len;
        if (lane == 63) num->gLP[w] = lincl;
      }
      st.wpre[w][lane] = (unsigned char)g.pexcl;
      if (lane == 0) { st.gT[w] = g.T; st.gNS[w] = g.ns; st.gNL[w] = __popcll(g.lmask); }
      if (lane == 63) st.gLU[w] = uincl;
      if (tid == 0) st.claim = NW;
    }
    __syncthreads();
    // ---- the chunk's unit list: short trips of the groups first, then the long units (lane g < NW holds group g)
    const int gT = lane < NW ? st.gT[lane] : 0;
    const int gNS = lane < NW ? st.gNS[lane] : 0;
    const int gNL = lane < NW ? st.gNL[lane] : 0;
    const int lug = lane < NW ? st.gLU[lane] : 0;
    const int ntg = (((gT + WAVE - 1) >> 6) + U - 1) / U;
    const int sIncl = wave_incl_add(ntg), lIncl = wave_incl_add(lug);
    const int S = __builtin_amdgcn_readlane(sIncl, 63);
    const int total = S + __builtin_amdgcn_readlane(lIncl, 63);
    int tIncl = 0, lpIncl = 0, gLPv = 0, shortSum = 0;
    if (num) {
      gLPv = lane < NW ? num->gLP[lane] : 0;
      tIncl = wave_incl_add(gT);
      lpIncl = wave_incl_add(gLPv);
      shortSum = __builtin_amdgcn_readlane(tIncl, 63);
    }
    for (int u = __builtin_amdgcn_readfirstlane(w); u < total;) {
      int unext = 0;
      if (lane == 0) unext = atomicAdd(&st.claim, 1);
      if (u < S) {
        const int g = __popcll(ballot64(sIncl <= u));                       // group of this trip (< NW: sIncl[63] = S > u)
        const int t = u - (__builtin_amdgcn_readlane(sIncl, g) - __builtin_amdgcn_readlane(ntg, g));
        const int T = __builtin_amdgcn_readlane(gT, g), ns = __builtin_amdgcn_readlane(gNS, g);
        unsigned long long W[U];
        int base[U];
#pragma unroll
        for (int uu = 0; uu < U; ++uu) {
          const int r = min(t * U + uu, WAVE - 1);
          W[uu] = st.marks[g][r];                                          // uniform address: broadcast reads
          base[uu] = st.wpre[g][r];
        }
        const int p0 = num ? chunkBase + (__builtin_amdgcn_readlane(tIncl, g) - T) + t * U * WAVE : -1;
        short_trip<U, NEED_VAL, 16>(reinterpret_cast<const char*>(st.rec[g]), T, ns, t * U, W, base, JB, VB, f, p0);
      } else {
        const int ul = u - S;
        const int g = __popcll(ballot64(lIncl <= ul));
        const int ug = ul - (__builtin_amdgcn_readlane(lIncl, g) - __builtin_amdgcn_readlane(lug, g));
        const int nl = __builtin_amdgcn_readlane(gNL, g);
        const int uex = lane < nl ? st.rec[g][WAVE - 1 - lane].w : 0x7fffffff;   // unit offsets of the group's long entries
        const int k = __popcll(ballot64(uex <= ug)) - 1;
        const int4 r4 = st.rec[g][WAVE - 1 - k];
        const int p0 = num ? chunkBase + shortSum + (__builtin_amdgcn_readlane(lpIncl, g) - __builtin_amdgcn_readlane(gLPv, g)) +
                                 num->lpro[g][k] + (ug - r4.w) * UP
                           : -1;
        long_trip<U, NEED_VAL>(r4.x, r4.z, __int_as_float(r4.y), (ug - r4.w) * UP, JB, VB, f, p0);
      }
      u = __builtin_amdgcn_readfirstlane(unext);
    }
    // the callback's last LDS atomics return nothing (ds_or / ds_add_f32): nothing else waits for them, and a wave
    // that leaves the barrier may read their target before they have landed (seen as lost bitmap bits)
    __builtin_amdgcn_s_waitcnt(0xc07f);                  // lgkmcnt(0)
    if (num) chunkBase += shortSum + __builtin_amdgcn_readlane(lpIncl, 63);
    __syncthreads();
  }
}

// dynamic row scheduling for block-per-row kernels: rows of a bin differ by up to 8x in work, a static
// round-robin leaves the CUs with the light rows idle.  One agent-scope atomic per row (guide: "dequeue",
// ~0.3-1 us, overlapped with the previous row's tail by fetching one row ahead).
// A single queue word saturates near 88 dequeues/us (guide, "dequeue"): kernels whose rows are short take R
// rows per atomic.
template <int R>
__device__ __forceinline__ int next_row(int* ctr, int* slot, int prev) {
  if (R > 1 && prev >= 0 && (prev + 1) % R != 0) return prev + 1;      // still inside the batch (block-uniform)
  if (threadIdx.x == 0) *slot = atomicAdd(ctr, R);
  __syncthreads();
  const int q = *slot;
  __syncthreads();
  return q;
}
__device__ __forceinline__ int next_row(int* ctr, int* slot) { return next_row<1>(ctr, slot, -1); }
// A queue of `count` rows handed out R at a time has ceil(count / R) batches, so blocks beyond that many can never all be
// needed: they leave before their first dequeue.  The launches over a fallback list are sized by the bin (the list's length is
// on the device only) and the list is short or empty most of the time: a thousand blocks that each spend one atomic on the
// queue word to learn that took 0.035 ms per launch on the headline matrix (profiles/README.md, "Mid rows: one wave per row").
__device__ __forceinline__ bool surplus_block(int count, int R) { return (long long)blockIdx.x * R >= (long long)count; }

// per-row metadata, fetched one row ahead of use so that the dependent rowIds -> IA/IC loads of the
// next row overlap the current row's work
struct RowMeta { int row, as, ae, x0, x1, x2; };

__device__ __forceinline__ RowMeta load_meta_sym(const int* rows, int q, int count, const int* IA, const int* rowFlops) {
  RowMeta mtd{0, 0, 0, 0, 0, 0};
  if (q < count) { mtd.row = rows[q]; mtd.as = IA[mtd.row]; mtd.ae = IA[mtd.row + 1]; mtd.x0 = rowFlops[mtd.row]; }
  return mtd;
}
template <class Rows>
__device__ __forceinline__ RowMeta load_meta_num(const Rows& rows, int q, int count, const int* IA, const int* IC,
                                                 const int* rowFlops = nullptr) {
  RowMeta mtd{0, 0, 0, 0, 0, 0};
  if (q < count) {
    mtd.row = rows[q]; mtd.as = IA[mtd.row]; mtd.ae = IA[mtd.row + 1]; mtd.x0 = IC[mtd.row]; mtd.x1 = IC[mtd.row + 1];
    if (rowFlops) mtd.x2 = rowFlops[mtd.row];
  }
  return mtd;
}

// wave-per-row kernels: this lane's A entry of the row's first chunk, fetched one row ahead
__device__ __forceinline__ PreA load_pre(const RowMeta& mtd, const int2* SBL, const float* VA, bool needVal) {
  PreA p{0, 0, 0.f, true};
  const int ap = mtd.as + lane_id();
  if (ap < mtd.ae) { const int2 sbl = SBL[ap]; p.bs = sbl.x; p.len = sbl.y; if (needVal) p.a = VA[ap]; }
  return p;
}

// ------------------------------------------------------------------------------------------------
// The re-hit log kit: "log the repeats, store the rest direct", the default path of a float product's rows of 513 products
// and more.  The scheme, once:
// SYMBOLIC pass (k_sym_hash<.., true>, k_sym_midpair, k_sym_big<true>): the insert says which products are RE-HITS of a
// column the row already has.  Every wave compacts the re-hit columns of a trip (ballot + rank + one LDS counter add) and
// appends them to the row's stretch of a log in HBM (rehit_log_append); nothing is deduplicated, a column hit k times is
// logged k-1 times, so a row logs exactly products - IC[row] entries.  The row's metadata is {first log entry, re-hits};
// the count is -1 when the row logged more than `cap` entries or found no room -- such a row leaves the log as it found
// it and goes on a fallback list for the kernel with the full table.  Where the log space comes from is the kernel's:
// chunks off one global cursor for the mid rows (LogChunk), a region per block for the big ones.
// NUMERIC pass (k_num_bigdirect, k_num_middirect, k_num_midwave): a table of at most S (key, value) slots that holds ONLY
// the row's repeated columns.  The log is inserted first (fill_from_log), every key with the value bits of -0.0f (the
// additive identity: a column hit twice ends as exactly a + b, as in the full-table kernels).  Then the products are
// walked once and probe READ-ONLY (probe_rounds): a hit adds its value under EXEC; a miss -- the probe meets an empty
// slot -- is a product whose column occurs once in the row, and goes straight to JC/C at the next free position of the
// row's range (ballot rank; where the position comes from is the kernel's policy).  The table sweep then emits the
// repeated columns behind them.  A row is taken only with 0 <= re-hits <= cap <= bd_cap(S) (load_meta_logged), so the
// table can never fill up and every probe ends at an empty slot; the other rows are skipped, they are in the fallback
// list.  A row without any repeated column (IC range = products) is EXPANDED (expanded_store): no table at all.
// ------------------------------------------------------------------------------------------------
// re-hits a row may log and still take a direct kernel with a table of S slots: the distinct repeated columns are at most
// the re-hits, so the table is never more than 7/8 full
__host__ __device__ constexpr int bd_cap(int S) { return S / 8 * 7; }

// ---- symbolic side
// The re-hit columns of one trip of a wave, appended to the row's log stretch of `room` ints from myLog[first] on.  *logCnt:
// the row's re-hits so far (LDS); *logOvf: set when the row passes `room` -- then nothing more is stored, the row falls back.
// (`first` is k_sym_big's place in its block's region, an index apart from the pointer: folded into it, that kernel comes
// out with two more VGPRs; the chunk kernels pass their row's own pointer and 0.)
template <int R>
__device__ __forceinline__ void rehit_log_append(const bool (&rehit)[R], const int (&col)[R], int* logCnt, int* logOvf,
                                                 int* myLog, int first, int room) {
  unsigned long long mk[R];
  int tot = 0;
#pragma unroll
  for (int u = 0; u < R; ++u) { mk[u] = ballot64(rehit[u]); tot += __popcll(mk[u]); }
  if (tot) {                                             // wave-uniform
    int base = 0;
    if (lane_id() == 0) base = atomicAdd(logCnt, tot);
    base = __builtin_amdgcn_readfirstlane(base);
    if (base + tot > room) {                             // wave-uniform: a row for the fallback kernel
      if (lane_id() == 0) *logOvf = 1;
    } else {
#pragma unroll
      for (int u = 0; u < R; ++u) {                      // base + tot <= room: inside the stretch
        if (rehit[u]) myLog[first + base + mask_rank(mk[u])] = col[u];
        base += __popcll(mk[u]);
      }
    }
  }
}

// Log space of the mid rows (bins 6-7): CHUNKS of MD_CHUNK ints reserved from one global cursor (one global atomic per
// chunk, not per row) and filled front to back over the rows of a block (k_sym_midpair's light rows: of a half).  A row
// starts only with `cap` ints left in the chunk, so it can run out of room only by passing the cap.  A chunk that lies
// beyond the log's capacity logs nothing (the cursor keeps counting there: its final value is the space the call would
// have used, which sizes the log of the handle's next call); its rows fall back, *fbCount counts them.
constexpr int MD_CHUNK = 4096;                 // log ints per reservation: at least two rows at the largest cap (bd_cap(2048) = 1792),
                                               // about 50 rows of the headline matrix (60 re-hits per row on average)
struct MidLogArgs {
  int2* meta;                                  // per ROW ID: {first log entry, re-hits or -1}
  int* log;
  long long logCap;                            // ints of `log` (0: none yet -- every row falls back, the demand is still counted)
  int cap;                                     // re-hits a row may log
  unsigned long long* cursor;                  // next unreserved int of the log
  int* fbList;
  int* fbCount;
  unsigned long long* logged;                  // sum of the re-hits of the rows that stay direct (test hook)
};
// The chunk in use, uniform over the threads that share a row.  A row: is_full() -> one thread reserve()s into an LDS word,
// barrier, take(word); the walk appends to log() within room(); behind the barrier after the walk, finish().
struct LogChunk {
  unsigned long long start = 0ull;             // first int of the chunk
  int used = MD_CHUNK;                         // ints of it in use (MD_CHUNK: none reserved yet)
  unsigned long long directSum = 0ull;         // re-hits of the rows that stayed direct (test hook), kept by the threads that `sums`
  __device__ __forceinline__ bool is_full(const MidLogArgs& ml) const { return used + ml.cap > MD_CHUNK; }   // may not hold another row
  __device__ __forceinline__ static unsigned long long reserve(const MidLogArgs& ml) {
    return atomicAdd(ml.cursor, (unsigned long long)MD_CHUNK);
  }
  __device__ __forceinline__ void take(unsigned long long s) { start = s; used = 0; }
  __device__ __forceinline__ bool logging(const MidLogArgs& ml) const {
    return start + (unsigned long long)MD_CHUNK <= (unsigned long long)ml.logCap;
  }
  __device__ __forceinline__ int* log(const MidLogArgs& ml) const { return ml.log + start + used; }
  __device__ __forceinline__ int room(const MidLogArgs& ml) const { return min(ml.cap, MD_CHUNK - used); }   // (= cap; the chunk bounds every store whatever cap is)
  // The row is done (logging: what logging() said before its walk): `products` of them on `cnt` distinct columns, `logged`
  // re-hits counted, ovf: it passed room().  The `leader` thread writes the row's count and metadata.  A row that stays
  // direct has logged <= room <= cap.  (The sum is kept in here and the flag handed in: with finish() returning `direct`
  // to a sum of the caller's, k_sym_midpair spills nine more SGPRs.)
  __device__ __forceinline__ void finish(const MidLogArgs& ml, bool logging, bool leader, bool sums, int row, int products,
                                         int cnt, int logged, bool ovf, int* __restrict__ IC) {
    const int rehits = products - cnt;                   // what the row logs when it has room
    const bool direct = logging && !ovf;
    if (leader) {
      IC[row] = cnt;
      ml.meta[row] = make_int2((int)start + used, direct ? logged : -1);
      if (!direct) ml.fbList[atomicAdd(ml.fbCount, 1)] = row;
    }
    if (direct) { used += logged; if (sums) directSum += (unsigned long long)logged; }
    else if (!logging && rehits >= 0 && rehits <= ml.cap) used += rehits;   // no log yet: count the demand
  }
};

// ---- numeric side
// A row's log into its cleared table: distinct keys <= lc <= cap < S, or size >= 4 * lc
__device__ __forceinline__ void fill_from_log(slot_t* tab, int size, int shift, const int* __restrict__ lg, int lc, int tid,
                                              int nthreads) {
  const unsigned mask = (unsigned)size - 1u;
  for (int i = tid; i < lc; i += nthreads) {
    const int c = lg[i];
    const slot_t own = make_slot(c, -0.0f);
    unsigned h = ((unsigned)c * 2654435761u) >> shift;
    for (int probe = 0; probe < size; ++probe) {
      const slot_t old = atomicCAS(&tab[h], EMPTY_SLOT, own);
      if (old == EMPTY_SLOT || slot_key(old) == c) break;
      h = (h + 1u) & mask;
    }
  }
}

// U rounds of products against the table of the row's repeated columns (`base`; dumB: this lane's dummy word, as a byte
// offset from it), keys read-only: a hit adds under EXEC, missOut[u] says that the product met an empty slot.  (The misses
// are gathered in an array of the helper's own and copied out once: gathered through the reference, or handed on to a
// functor, the compiler keeps them packed in bytes -- 16 to 116 more instructions per kernel, and a lower occupancy.)
template <int U>
__device__ __forceinline__ void probe_rounds(char* base, int dumB, int size, int shift, const bool (&act)[U],
                                             const int (&col)[U], const float (&val)[U], int* __restrict__ err,
                                             bool (&missOut)[U]) {
  const int maskB = size * 8 - 1;
  int hB[U], hitB[U];                                  // byte offsets; dumB = "done" / "no hit"
  bool miss[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const unsigned h = ((unsigned)col[u] * 2654435761u) >> shift;
    hB[u] = act[u] ? (int)(h * 8u) : dumB;
    hitB[u] = dumB;
    miss[u] = false;
  }
  for (int probe = 0;;) {                              // the keys do not change during the walk: plain reads
    int key[U];
#pragma unroll
    for (int u = 0; u < U; ++u) key[u] = *reinterpret_cast<const int*>(base + hB[u]);
    ++probe;
    int pendBits = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool pend = hB[u] != dumB;
      const bool hit = pend && key[u] == col[u];
      const bool emp = pend && key[u] == EMPTY_KEY;
      hitB[u] = hit ? hB[u] : hitB[u];
      miss[u] = miss[u] || emp;
      hB[u] = (pend && !hit && !emp) ? ((hB[u] + 8) & maskB) : dumB;   // linear, like fill_from_log
      pendBits |= hB[u] ^ dumB;
    }
    if (ballot64(pendBits != 0) == 0ull) break;
    if (probe >= size) { atomicOr(err, ERRF_TABLE_FULL); break; }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (hitB[u] != dumB) atomicAdd(reinterpret_cast<float*>(base + hitB[u] + 4), val[u]);
#pragma unroll
  for (int u = 0; u < U; ++u) missOut[u] = miss[u];
}
// The misses of U rounds go to the next free positions of the row's range of `lim` entries, in ballot rank order.  Where
// the position comes from is the kernel's: a register of the wave kernel -- returns the position behind the misses --
template <int U>
__device__ __forceinline__ int store_misses(const bool (&miss)[U], const int (&col)[U], const float (&val)[U], int pos,
                                            unsigned lim, int* __restrict__ JCrow, float* __restrict__ Crow) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const unsigned long long mk = ballot64(miss[u]);
    const unsigned o = (unsigned)(pos + mask_rank(mk));
    if (miss[u] && o < lim) { st_out(JCrow + o, col[u]); st_out(Crow + o, val[u]); }
    pos += __popcll(mk);
  }
  return pos;
}
// ... or the row's LDS counter of the block kernels, drawn from once per trip for all U rounds together
template <int U>
__device__ __forceinline__ void store_misses_claimed(const bool (&miss)[U], const int (&col)[U], const float (&val)[U],
                                                     int* emitted, unsigned lim, int* JCrow, float* Crow) {
  unsigned long long mk[U];
  int tot = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) { mk[u] = ballot64(miss[u]); tot += __popcll(mk[u]); }
  if (tot) {                                           // wave-uniform
    int pos = 0;
    if (lane_id() == 0) pos = atomicAdd(emitted, tot);
    pos = __builtin_amdgcn_readfirstlane(pos);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned o = (unsigned)(pos + mask_rank(mk[u]));
      if (miss[u] && o < lim) { st_out(JCrow + o, col[u]); st_out(Crow + o, val[u]); }
      pos += __popcll(mk[u]);
    }
  }
}

// An expanded row: no repeated column, so every product goes to its number in the walk.  The walk's functor for such a
// row, over the caller's own variables (`lane`: its lane id) like the lambdas it stands for: as a helper called from a
// lambda, or with copies of them, k_num_middirect and k_num_midwave come out with three to five VGPRs fewer -- another
// occupancy figure than the kernels were measured with, which is not this code's to change.
__device__ __forceinline__ auto expanded_store(const int& lane, const unsigned& lim, int* const& JCrow, float* const& Crow) {
  return [&](const auto& act, const auto& col, const auto& val, int p0) {
    constexpr int R = (int)(sizeof(col) / sizeof(col[0]));
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const unsigned o = (unsigned)(p0 + u * WAVE + lane);
      if (act[u] && o < lim) { st_out(JCrow + o, col[u]); st_out(Crow + o, val[u]); }
    }
  };
}

// Bin 6 has two direct kernels: k_num_midwave (one wave per row, a table of MW_SLOTS slots) and k_num_middirect.  THE rule
// for which of the two takes a row, read by both: the wave kernel takes the rows that logged (lm = the row's {first log
// entry, re-hits}) at most waveCap <= bd_cap(MW_SLOTS) re-hits and whose log lies inside the log; k_num_middirect keeps the
// other rows up to its own cap.  waveCap < 0: no wave kernel in this call (bin 7, SPGEMM_MD_WAVE=0, a bin below the row
// threshold).
constexpr int MW_SLOTS = 512;
__device__ __forceinline__ bool midwave_takes(int2 lm, long long logCap, int waveCap) {
  return lm.y >= 0 && lm.y <= waveCap && lm.x >= 0 && (long long)lm.x + lm.y <= logCap;
}
// Row q of `rows` (rows[q], q < count) with its log, fetched one row ahead like RowMeta: ls = first log entry, lc = re-hits,
// or -1 for a row that is not this kernel's.  lm = meta[q] (byRow: meta[row id]); take(lm) is the kernel's rule: > 0 the
// row is taken, 0 it is skipped, < 0 (k_num_midwave) it is left to another list: lc = -1, ls = 1 and the row id.
struct LoggedMeta { RowMeta m; int ls, lc; };
template <class Rows, class Take>
__device__ __forceinline__ LoggedMeta load_meta_logged(const Rows& rows, int q, int count, const int* IA, const int* IC,
                                                       const int* rowFlops, const int2* meta, bool byRow, Take take) {
  LoggedMeta d{{0, 0, 0, 0, 0, 0}, 0, -1};
  if (q < count) {
    const int row = rows[q];
    const int2 lm = meta[byRow ? row : q];
    const int t = take(lm);
    if (t > 0) {
      d.ls = lm.x; d.lc = lm.y; d.m = load_meta_num(rows, q, count, IA, IC, rowFlops);
    } else if (t < 0) { d.ls = 1; d.m.row = row; }
  }
  return d;
}

// ------------------------------------------------------------------------------------------------
// Medium rows (65..4096 products): one block of NW waves per row, LDS key table (symbolic) or
// key+value table compacted by a table sweep (numeric).
// ------------------------------------------------------------------------------------------------
// LOG (NW > 1, bins 6-7 of a float product, for k_num_middirect): the logging symbolic pass of the kit above, log space in
// chunks (LogChunk).

template <int NW, int TBL, int U, bool LOG = false>
__global__ __launch_bounds__(WAVE * NW) void k_sym_hash(const int* __restrict__ binPtr, int bin,
                                                         const int* __restrict__ rowIds,
                                                         const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                         const int* __restrict__ JB,
                                                         const int* __restrict__ rowFlops, int* __restrict__ IC,
                                                         int* __restrict__ err, int* __restrict__ qctr, MidLogArgs ml) {
  static_assert(!LOG || NW > 1, "only the multi-wave kernels log");
  __shared__ __attribute__((aligned(16))) int keys[TBL];
  __shared__ typename WalkSel<NW>::type st;
  __shared__ int cnt_s;
  __shared__ int qslot;
  __shared__ int logCnt_s, logOvf_s;             // LOG: re-hits of the current row so far; the row passed the cap
  __shared__ unsigned long long chunk_s;         // LOG: the chunk reserved last
  LogChunk chunk;                                // LOG, block-uniform: the block's chunk
  const int tid = threadIdx.x, lane = lane_id();
  if (tid < WAVE) st.dummy[tid] = DUMMY_SLOT;    // (ordered before the first insert by the barrier / wave order below)
  int first = binPtr[bin], count = binPtr[bin + 1] - first;
  constexpr int QB = NW >= 8 ? 2 : 4;            // rows per dequeue
  int stride = (int)gridDim.x;
  if (NW == 1) {                                 // static schedule: XCD-contiguous (see xcd_range)
    const XcdRange xr = xcd_range(count);
    first += xr.lo; count = xr.hi - xr.lo; stride = xr.nb;
  }
  const int* rows = rowIds + first;
  int q = NW > 1 ? next_row<QB>(qctr, &qslot, -1) : (int)(blockIdx.x >> 3);
  RowMeta cur = load_meta_sym(rows, q, count, IA, rowFlops);
  // NW == 1: two rows of metadata and one row of A entries are in flight ahead of the row being processed
  RowMeta nxt = NW == 1 ? load_meta_sym(rows, q + stride, count, IA, rowFlops) : RowMeta{0, 0, 0, 0, 0, 0};
  PreA pc = NW == 1 ? load_pre(cur, SBL, nullptr, false) : PreA{0, 0, 0.f, false};
  while (q < count) {
    int qn;
    PreA pn{0, 0, 0.f, false};
    RowMeta nn{0, 0, 0, 0, 0};
    if (NW == 1) {
      qn = q + stride;
      nn = load_meta_sym(rows, qn + stride, count, IA, rowFlops);
      pn = load_pre(nxt, SBL, nullptr, false);
    } else {
      qn = next_row<QB>(qctr, &qslot, q);
      nxt = load_meta_sym(rows, qn, count, IA, rowFlops);
    }
    const int size = table_size<4>(cur.x0, 64, TBL);
    const int shift = 32 - log2_pow2(size);
    clear_table(keys, nullptr, size, tid, WAVE * NW);
    if (tid == 0) cnt_s = 0;
    const bool newChunk = LOG && chunk.is_full(ml);   // block-uniform
    if constexpr (LOG) if (tid == 0) {
      logCnt_s = 0; logOvf_s = 0;
      if (newChunk) chunk_s = LogChunk::reserve(ml);
    }
    __syncthreads();
    if constexpr (LOG) if (newChunk) chunk.take(chunk_s);
    // (chunk_s is written again at the start of a later row, behind this row's barriers)
    const bool logging = LOG && chunk.logging(ml);
    int* const myLog = LOG && logging ? chunk.log(ml) : nullptr;
    const int room = LOG ? chunk.room(ml) : 0;
    int mine = 0;
    for_each_product<NW, U, false>(st, cur.as, cur.ae, SBL, nullptr, JB, nullptr,
                                   [&](const auto& act, const auto& col, const auto& val, int) {
      if constexpr (!LOG)
      mine += hash_insert_chunked<InsChunk<NW>::value>(keys, size, shift, act, col, reinterpret_cast<int*>(&st.dummy[lane_id()]), err);
      else {
        constexpr int R = (int)(sizeof(col) / sizeof(col[0]));
        bool rehit[R];
        mine += hash_insert_chunked<InsChunk<NW>::value, true>(keys, size, shift, act, col,
                                                               reinterpret_cast<int*>(&st.dummy[lane_id()]), err, &rehit);
        if (logging) rehit_log_append(rehit, col, &logCnt_s, &logOvf_s, myLog, 0, room);   // block-uniform
      }
    }, pc, err);
    const int ws = wave_sum(mine);                           // hash_insert_multi counts per lane
    if (NW == 1) {
      if (lane == 0) IC[cur.row] = ws;
    } else {
      if (lane == 0 && ws) atomicAdd(&cnt_s, ws);
      __syncthreads();
      if constexpr (LOG) {
        const int logged = logCnt_s;                     // (reset at the start of the next row, behind the barrier below)
        chunk.finish(ml, logging, tid == 0, true, cur.row, cur.x0, cnt_s, logged, logOvf_s, IC);
      } else if (tid == 0) IC[cur.row] = cnt_s;
    }
    __syncthreads();
    cur = nxt;
    if (NW == 1) { nxt = nn; pc = pn; }
    q = qn;
  }
  if constexpr (LOG) if (tid == 0 && chunk.directSum) atomicAdd(ml.logged, chunk.directSum);
}

// ---- bin 6 of a logging symbolic pass: k_sym_midpair.  k_sym_hash<4,4096,2,true> gives every row of 513-2048 products four
// waves, a dequeue and seven block barriers, and a row has 49 A entries on average: one staged group, three waves waiting
// for it.  Here a block of HW waves has ONE table of 4096 keys, and one launch runs over both layout slots on the static
// schedule of k_num_midwave (each XCD's eighth of the heavy slot first, then its eighth of the light one; no queue word):
//   heavy rows (1025-2048 products): all HW waves on one row, the whole table (two slots per product);
//   light rows (513-1024 products): TWO rows at a time, HW/2 waves and HALF of the table each (two slots per product,
//     load <= 0.5 where the four-wave kernel gives them four).
// The walk is the wave-per-row one and needs no barrier: EVERY wave of a row stages every group of 64 A entries for itself
// (one load and one scan, the same for all of them) and takes the rounds k, k + K, ... of the group's products, up to 8
// gathered before the first insert.  So a row costs two block barriers whatever its shape -- behind the table clear and
// behind the count -- which is what lets two light rows share a block: both halves pass the same barriers (a half without
// a row on the last trip passes them idle).  The row's counters alternate between two sets, so the next row's reset needs
// no third barrier.  The next two rows' metadata and the next row's first A entries are in flight as in k_sym_hash<1, ..>.
// HW = 2: 19.5 KB of LDS (a light row has one wave: no barrier in that mode).  HW = 4: 22.5 KB.  The compiler's occupancy
// figures are 8 and 7 blocks per CU; measured, six of either are resident, and the host launches six (spPerCU).
// Measured on the headline matrix (profiles/README.md, "Mid rows, symbolic"): HW = 4 equals the four-wave kernel's time, HW = 2
// is 12 % behind it -- so the launch is opt-in (SPGEMM_SYM_PAIR=1).
// The log is k_sym_hash<.., true>'s in meaning: IC exact, a row logs products - IC columns, meta / fbList / cursor / logged
// as there (the kit).  Chunks are reserved by the block for heavy rows and by each half for light ones (half 0 goes on in
// the block's chunk).  `took`: rows this launch processed (test hook).
#ifndef SMF_SP_CH
#define SMF_SP_CH 1
#endif
constexpr int SP_CH = SMF_SP_CH;                  // rounds of a trip inserted per probe loop, as in the wave-per-row kernels
struct MidPairCtr { int cnt, logCnt, logOvf; };
template <int HW>
struct MidPairShared {
  int keys[4096];
  WalkStage1 st[HW];                             // every wave stages for itself
  MidPairCtr ctr[2][2];                          // [half][row parity]: distinct columns, re-hits logged, "passed the cap" (heavy rows: half 0's)
  unsigned long long chunk[2];                   // the chunk a half (heavy rows: the block) reserved last
};
static_assert(sizeof(MidPairShared<4>) <= 24 * 1024, "k_sym_midpair: six blocks per CU with room to spare");

// U rounds of 64 short products of one staged group, the rounds given one by one (short_trip takes consecutive ones)
template <int U, class F>
__device__ __forceinline__ void short_trip_at(const char* rec, int T, int ns, const int (&rnd)[U], const unsigned long long (&W)[U],
                                              const int (&base)[U], const int* __restrict__ JB, F&& f) {
  const int lane = lane_id();
  int col[U];
  bool act[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {                          // straight-line, no branches around the gathers
    const int p0 = rnd[u] * WAVE + lane;
    act[u] = p0 < T;
    const int p = min(p0, T - 1);                        // lanes past the end shadow the last product: valid, nearby reads
    int e = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(W[u] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)W[u], (unsigned)base[u]));
    e = min(e, ns - 1);
    const int2 ra = *reinterpret_cast<const int2*>(rec + e * 8);
    col[u] = JB[ra.x + p];
  }
  __builtin_amdgcn_sched_barrier(0);                     // all U gathers are issued before the first of them is waited for
  f(act, col);
}

// the wave-per-row walk (for_each_product<1>, symbolic) of wave k of the K that share a row: all groups staged, the rounds
// k, k + K, ... of each walked.  f(act[R], col[R]) for R in {1,2,3,4,6,8}, in wave-uniform control flow.
template <int K, class F>
__device__ __forceinline__ void for_each_column_dealt(WalkStage1& st, int k, int as, int ae, const int2* __restrict__ SBL,
                                                      const int* __restrict__ JB, F&& f, PreA pre, int* err) {
  const int lane = lane_id();
  for (int gb = as; gb < ae; gb += WAVE) {
    const GroupLanes g = stage_group<false, 8, 0x40000000>(st.marks, reinterpret_cast<char*>(st.rec), gb + lane, ae, SBL, nullptr,
                                                           gb == as ? pre : PreA{0, 0, 0.f, false});
    if (g.T > WAVE * WAVE || g.T <= 0) {                 // more than a row of this bin has / nothing but empty B rows
      if (g.T > 0 && err && lane == 0) atomicOr(err, ERRF_TABLE_FULL);
      continue;
    }
    const int nr = (g.T + WAVE - 1) >> 6;
    const int nj = nr > k ? (nr - k + K - 1) / K : 0;    // this wave's rounds of the group: k + j K, j < nj
    const unsigned mlo = (unsigned)g.mw, mhi = (unsigned)(g.mw >> 32);
    for (int j0 = 0; j0 < nj; j0 += 8) {
      with_rounds(min(8, nj - j0), [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        unsigned long long W[R];
        int base[R], rnd[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
          rnd[u] = k + (j0 + u) * K;                     // (past the group's end for the rounds that pad 5 to 6 and 7 to 8: no lane active)
          const int r = min(rnd[u], WAVE - 1);
          W[u] = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)mlo, r) |
                 ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)mhi, r) << 32);
          base[u] = __builtin_amdgcn_readlane(g.pexcl, r);
        }
        short_trip_at<R>(reinterpret_cast<const char*>(st.rec), g.T, g.ns, rnd, W, base, JB, f);
      });
    }
  }
}

template <int HW>
__global__ __launch_bounds__(HW * WAVE) void k_sym_midpair(const int* __restrict__ slotBase, int slotLo, int slotHi,
                                                           const int* __restrict__ rowIds,
                                                           const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                           const int* __restrict__ JB,
                                                           const int* __restrict__ rowFlops, int* __restrict__ IC,
                                                           int* __restrict__ err, MidLogArgs ml,
                                                           unsigned long long* __restrict__ took) {
  static_assert(HW == 2 || HW == 4, "two halves of HW/2 waves");
  constexpr int TBL = 4096, LW = HW / 2;
  __shared__ __attribute__((aligned(16))) MidPairShared<HW> sh;
  const int tid = threadIdx.x, lane = lane_id(), w = __builtin_amdgcn_readfirstlane(tid >> 6);
  WalkStage1& st = sh.st[w];
  int* const dummy = reinterpret_cast<int*>(&st.dummy[lane]);
  st.dummy[lane] = DUMMY_SLOT;
  wave_lds_sync();
  // the chunk in use: uniform over the waves of a row; its sum and the rows processed: kept by the first wave of a row
  LogChunk chunk;
  int tookRows = 0;
  int par = 0;
  const XcdRange xh = xcd_range(slotBase[slotHi + 1] - slotBase[slotHi]);
  const XcdRange xl = xcd_range(slotBase[slotLo + 1] - slotBase[slotLo]);
  const int* const hiRows = rowIds + slotBase[slotHi] + xh.lo;
  const int* const loRows = rowIds + slotBase[slotLo] + xl.lo;
  const int nhi = xh.hi - xh.lo, nlo = xl.hi - xl.lo;
  const int nb = xh.nb;
  // one row by the K waves that share it; this wave is number k of them and this thread number gt.  have = false: a half
  // without a row, which only passes the barriers
  auto do_row = [&](auto kc, bool have, const RowMeta& cur, const PreA& pc, int* keys, int tblMax, int k, int gt,
                    MidPairCtr* sets, unsigned long long* chunkSlot) {
    constexpr int K = decltype(kc)::value;
    auto sync = [] { if constexpr (K == HW) __syncthreads(); else if constexpr (K == 1) wave_lds_sync(); else __syncthreads(); };
    MidPairCtr& rc = sets[par];
    const int size = table_size<2>(cur.x0, 64, tblMax);
    const int shift = 32 - log2_pow2(size);
    const bool newChunk = have && chunk.is_full(ml);     // row-uniform
    if (have) {
      clear_table(keys, nullptr, size, gt, K * WAVE);
      if (gt == 0) {
        rc.cnt = 0; rc.logCnt = 0; rc.logOvf = 0;
        if (newChunk) *chunkSlot = LogChunk::reserve(ml);
      }
    }
    sync();
    if (newChunk) chunk.take(*chunkSlot);                // (written again at the start of a later row, behind this row's barriers)
    const bool logging = chunk.logging(ml);
    if (have) {
      int* const myLog = logging ? chunk.log(ml) : nullptr;
      const int room = chunk.room(ml);
      int mine = 0;
      for_each_column_dealt<K>(st, k, cur.as, cur.ae, SBL, JB, [&](const auto& act, const auto& col) {
        constexpr int R = (int)(sizeof(col) / sizeof(col[0]));
        bool rehit[R];
        mine += hash_insert_chunked<SP_CH, true>(keys, size, shift, act, col, dummy, err, &rehit);
        if (logging) rehit_log_append(rehit, col, &rc.logCnt, &rc.logOvf, myLog, 0, room);   // row-uniform
      }, pc, err);
      const int ws = wave_sum(mine);                     // hash_insert_multi counts per lane
      if (lane == 0 && ws) atomicAdd(&rc.cnt, ws);
      __builtin_amdgcn_s_waitcnt(0xc07f);                // lgkmcnt(0): the adds that return nothing have landed
    }
    sync();                                              // (every wave's inserts are behind it: the table is free, too)
    if (have) {
      const int cnt = rc.cnt, logged = rc.logCnt;        // (this set is reset two rows on, behind the next row's barrier)
      chunk.finish(ml, logging, gt == 0, k == 0, cur.row, cur.x0, cnt, logged, rc.logOvf, IC);
      if (k == 0) ++tookRows;
    }
    par ^= 1;
  };
  // ---- heavy rows: the block strides over the XCD's share
  {
    int q = xh.bi;
    RowMeta cur = load_meta_sym(hiRows, q, nhi, IA, rowFlops);
    RowMeta nxt = load_meta_sym(hiRows, q + nb, nhi, IA, rowFlops);
    PreA pc = load_pre(cur, SBL, nullptr, false);
    while (q < nhi) {
      const int qn = q + nb;
      const RowMeta nn = load_meta_sym(hiRows, qn + nb, nhi, IA, rowFlops);
      const PreA pn = load_pre(nxt, SBL, nullptr, false);
      do_row(std::integral_constant<int, HW>{}, true, cur, pc, sh.keys, TBL, w, tid, sh.ctr[0], &sh.chunk[0]);
      cur = nxt; nxt = nn; pc = pn;
      q = qn;
    }
  }
  // ---- light rows: half h of block b takes rows 2b + h, 2b + h + 2 nb, ... of the XCD's share
  {
    const int h = w / LW, k = w % LW;
    if (h != 0) chunk = LogChunk();                      // (half 0 keeps the block's chunk; the others have summed nothing yet)
    const int stride = 2 * nb;
    int q0 = 2 * xl.bi;
    RowMeta cur = load_meta_sym(loRows, q0 + h, nlo, IA, rowFlops);
    RowMeta nxt = load_meta_sym(loRows, q0 + h + stride, nlo, IA, rowFlops);
    PreA pc = load_pre(cur, SBL, nullptr, false);
    while (q0 < nlo) {                                   // block-uniform: both halves pass the same barriers
      const int qn = q0 + stride;
      const RowMeta nn = load_meta_sym(loRows, qn + h + stride, nlo, IA, rowFlops);
      const PreA pn = load_pre(nxt, SBL, nullptr, false);
      do_row(std::integral_constant<int, LW>{}, q0 + h < nlo, cur, pc, sh.keys + h * (TBL / 2), TBL / 2, k, tid - h * LW * WAVE,
             sh.ctr[h], &sh.chunk[h]);
      cur = nxt; nxt = nn; pc = pn;
      q0 = qn;
    }
  }
  if (lane == 0) {
    if (chunk.directSum) atomicAdd(ml.logged, chunk.directSum);
    if (tookRows) atomicAdd(took, (unsigned long long)tookRows);
  }
}

template <int NW, int TBL, int U, int PRUNE = 0>      // PRUNE: see k_num_g16
__global__ __launch_bounds__(WAVE * NW) void k_num_hash(const int* __restrict__ binPtr, int bin,
                                                         const int* __restrict__ rowIds,
                                                         const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                         const float* __restrict__ VA,
                                                         const int* __restrict__ JB,
                                                         const float* __restrict__ VB,
                                                         const int* __restrict__ IC, int* __restrict__ JC,
                                                         float* __restrict__ C, int* __restrict__ err,
                                                         int* __restrict__ qctr, const int* __restrict__ rowFlops,
                                                         int* __restrict__ pcnt) {
  __shared__ __attribute__((aligned(16))) slot_t tab[TBL];   // (column, value) pairs
  __shared__ PruneShared<float, NW> ps;               // (fused prune, several waves: the block reductions)
  __shared__ typename WalkSel<NW>::type st;
  __shared__ int qslot;
  __shared__ int emitted;                        // output positions handed out so far in this row (NW > 1)
  const int tid = threadIdx.x;
  if (tid < WAVE) st.dummy[tid] = DUMMY_SLOT;
  constexpr int T = WAVE * NW;
  int first = binPtr[bin], count = binPtr[bin + 1] - first;
  constexpr int QB = NW >= 8 ? 2 : 4;            // rows per dequeue
  if (NW > 1 && surplus_block(count, QB)) return;
  int stride = (int)gridDim.x;
  if (NW == 1) {                                 // static schedule: XCD-contiguous (see xcd_range)
    const XcdRange xr = xcd_range(count);
    first += xr.lo; count = xr.hi - xr.lo; stride = xr.nb;
  }
  const int* rows = rowIds + first;
  int q = NW > 1 ? next_row<QB>(qctr, &qslot, -1) : (int)(blockIdx.x >> 3);
  const int* const rf = rowFlops;                        // the product count decides hash vs expansion
  RowMeta cur = load_meta_num(rows, q, count, IA, IC, rf);
  RowMeta nxt = NW == 1 ? load_meta_num(rows, q + stride, count, IA, IC, rf) : RowMeta{0, 0, 0, 0, 0, 0};
  PreA pc = NW == 1 ? load_pre(cur, SBL, VA, true) : PreA{0, 0, 0.f, false};
  while (q < count) {
    int qn;
    PreA pn{0, 0, 0.f, false};
    RowMeta nn{0, 0, 0, 0, 0};
    if (NW == 1) {
      qn = q + stride;
      nn = load_meta_num(rows, qn + stride, count, IA, IC, rf);
      pn = load_pre(nxt, SBL, VA, true);
    } else {
      qn = next_row<QB>(qctr, &qslot, q);
      nxt = load_meta_num(rows, qn, count, IA, IC, rf);
    }
    const int off = cur.x0;
    const int want = cur.x1 - off;                      // exact distinct count from the symbolic pass
    if (NW == 1 && PRUNE == 1 && want == cur.x2 && want <= TBL) {
      // fused prune of an expanded row: its products as a plain list in LDS (no clear, no probing), then the row rule
      for_each_product<NW, U, true>(st, cur.as, cur.ae, SBL, VA, JB, VB,
                                    [&](const auto& act, const auto& col, const auto& val, int p0) {
        constexpr int R = (int)(sizeof(col) / sizeof(col[0]));
#pragma unroll
        for (int u = 0; u < R; ++u) {
          const unsigned o = (unsigned)(p0 + u * WAVE + lane_id());
          if (act[u] && o < (unsigned)want) tab[o] = make_slot(col[u], val[u]);
        }
      }, pc, err);
      wave_lds_sync();
      int nocc;
      const int kept = prune_emit_group<64>(RowTab<float>{tab}, (want + 63) & ~63, want, false, true, lane_id(), JC + off, C + off, &nocc);
      if (lane_id() == 0) pcnt[cur.row] = kept;
      wave_lds_sync();
      cur = nxt;
      nxt = nn; pc = pn;
      q = qn;
      continue;
    }
    if (NW == 1 && PRUNE == 0 && want == cur.x2) {
      // As many distinct columns as products: no two products of this row meet, nothing to accumulate.  The row is
      // EXPANDED: every product goes straight to the position it has in the row's own numbering -- coalesced stores,
      // no table, no clear, no compaction sweep (more than half of the products of rows up to 256 products on a
      // power-law matrix sit in such rows).
      int* const JCrow = JC + off;
      float* const Crow = C + off;
      for_each_product<NW, U, true>(st, cur.as, cur.ae, SBL, VA, JB, VB,
                                    [&](const auto& act, const auto& col, const auto& val, int p0) {
        constexpr int R = (int)(sizeof(col) / sizeof(col[0]));
#pragma unroll
        for (int u = 0; u < R; ++u) {
          const unsigned o = (unsigned)(p0 + u * WAVE + lane_id());
          if (act[u] && o < (unsigned)want) { st_out(JCrow + o, col[u]); st_out(Crow + o, val[u]); }
        }
      }, pc, err);
      cur = nxt;
      if (NW == 1) { nxt = nn; pc = pn; }
      q = qn;
      continue;
    }
    if constexpr (NW > 1 && PRUNE == 0) if (want == cur.x2) {
      // several waves per row, no repeated column (16 % of the rows of 513-1024 products on the headline power-law matrix,
      // 13 % and 6 % of the two classes above): expanded
      // like the wave-per-row case, positions from the walk's dense product numbering
      int* const JCrow = JC + off;
      float* const Crow = C + off;
      for_each_product<NW, U, true>(st, cur.as, cur.ae, SBL, VA, JB, VB,
                                    [&](const auto& act, const auto& col, const auto& val, int p0) {
        constexpr int R = (int)(sizeof(col) / sizeof(col[0]));
#pragma unroll
        for (int u = 0; u < R; ++u) {
          const unsigned o = (unsigned)(p0 + u * WAVE + lane_id());
          if (act[u] && o < (unsigned)want) { st_out(JCrow + o, col[u]); st_out(Crow + o, val[u]); }
        }
      }, pc, err, reinterpret_cast<WalkNumber<NW>*>(tab));   // the table is idle in an expanded row: its memory holds the numbering
      cur = nxt;
      q = qn;
      continue;
    }
    const int size = table_size<4>(want, T > 64 ? T : 64, TBL);
    const int shift = 32 - log2_pow2(size);
    clear_slots(tab, size, tid, T);
    if (NW > 1 && tid == 0) emitted = 0;
    __syncthreads();
    if (!ABL(8))
    for_each_product<NW, U, true>(st, cur.as, cur.ae, SBL, VA, JB, VB,
                                  [&](const auto& act, const auto& col, const auto& val, int) {
      if (ABL(1)) {
#pragma unroll
        for (int u = 0; u < (int)(sizeof(col) / sizeof(col[0])); ++u) asm volatile("" :: "v"(col[u]), "v"(val[u]));
      } else
      hash_accum_chunked<InsChunk<NW>::value>(tab, size, shift, act, col, val, &st.dummy[lane_id()], err);
    }, pc, err);
    // compaction: wave w sweeps the contiguous slots [w*per, w*per+per) 64 at a time, so that a wave's stores
    // land on consecutive output positions.  One wave: a single pass.  Several waves: a wave reads its slots into
    // registers, claims its share of the row's output range with ONE LDS atomic (any order inside a row is a valid
    // CSR row) and emits from the registers: no counting sweep, no block scan, no barrier.
    const int per = size / NW;
    const int lane = lane_id(), w = tid >> 6;
    if (ABL(4)) { __syncthreads(); }
    else if (PRUNE && NW == 1) {
      int nocc;
      const int kept = prune_emit_group<64>(RowTab<float>{tab}, per, PRUNE == 2 ? -1 : want, true, true, lane, JC + off, C + off, &nocc);
      if (tid == 0) { pcnt[cur.row] = kept; if (PRUNE == 1 && nocc != want) atomicOr(err, ERRF_COUNT_MISMATCH); }
      __syncthreads();
    } else if (PRUNE) {
      prune_emit_block<NW, TBL / NW / WAVE>(RowTab<float>{tab}, WaveSegments{per}, PRUNE == 2 ? -1 : want, ps, JC + off, C + off, pcnt + cur.row, err);
      __syncthreads();
    } else if (NW == 1) {
      int pos = 0;                                    // relative to the row: small 32-bit offsets for both stores
      int* const JCrow = JC + off;
      float* const Crow = C + off;
      for (int i0 = 0; i0 < per; i0 += WAVE) {
        const slot_t sv = tab[i0 + lane];
        const bool occ = slot_key(sv) != EMPTY_KEY;
        const unsigned long long mk = ballot64(occ);
        const unsigned o = (unsigned)(pos + mask_rank(mk));
        if (occ && o < (unsigned)want) { st_out(JCrow + o, slot_key(sv)); st_out(Crow + o, slot_val(sv)); }
        pos += __popcll(mk);
      }
      if (tid == 0 && pos != want) atomicOr(err, ERRF_COUNT_MISMATCH);
      __syncthreads();
    } else {
      emit_claimed<TBL / NW / WAVE>(tab, w * per, per, &emitted, off, off + want, JC, C);
      __syncthreads();
      if (tid == 0 && emitted != want) atomicOr(err, ERRF_COUNT_MISMATCH);
    }
    cur = nxt;
    if (NW == 1) { nxt = nn; pc = pn; }
    q = qn;
  }
}

// ------------------------------------------------------------------------------------------------
// Big rows (> 4096 products): one 1024-thread block per row.
//   symbolic : LDS bitmap over a window of SYM_WC columns, popcount           (any n, 1 window up to 1M cols)
//   numeric A: n <= BIG_WC: bitmap (saved by the symbolic pass when the workspace has room, rebuilt
//              otherwise) + popcount ranks give every column its final position; values accumulate in an
//              LDS float array addressed by rank (no probing, sorted output)
//   numeric B: any n: 128 KB LDS hash table; rows with more distinct columns than one table holds take
//              several passes, each pass owning the columns of one hash class
//   numeric C: n > BIG_WC, rows whose repeated columns the symbolic pass logged: 8 waves per row, a small table for
//              the repeated columns only, every other product stored straight to C (k_num_bigdirect); the rows it
//              cannot take stay with numeric B
// ------------------------------------------------------------------------------------------------
#ifndef SMF_BIG_NW
#define SMF_BIG_NW 16
#endif
constexpr int BIG_NW = SMF_BIG_NW;   // (SMF_BIG_NW: diagnostic builds with fewer waves per big-row block)
constexpr int BIG_THREADS = BIG_NW * WAVE;
constexpr int BIG_U = 4;                        // rounds in flight per wave: bitmap / rank kernels
#ifndef SMF_BH_U
#define SMF_BH_U 2
#endif
constexpr int BH_U = SMF_BH_U;                         // ... and the big-row hash kernel (probe chains: 2 measured better than 4)
constexpr int SYM_WC = 1 << 20;                // columns per symbolic window (128 KB bitmap)
constexpr int SYM_WORDS = SYM_WC / 32;
constexpr int BIG_WC = 262144;                 // columns covered by the rank kernel (32 KB bitmap)
constexpr int BIG_WORDS = BIG_WC / 32;         // 8192
constexpr int BIG_WPT = BIG_WORDS / BIG_THREADS;  // 8 words per thread
constexpr int BIG_CAP = 16384;                 // float accumulators per rank pass (64 KB)
constexpr int BH_SLOTS = 16384;                // hash kernel: 128 KB of (key, value) pairs (what the walk stage leaves of 160 KB)
constexpr int BH_CAP = 11264;                  // distinct columns per hash pass (load <= 0.6 incl. partition skew; measured
                                               // best of 8704/10240/12800 once later passes stream parked products)
constexpr int BH_CAP_MAX = 12288;              // SPGEMM_BHCAP may raise the cap to this (load 0.74)
constexpr int BH_SPILL = 1 << 18;              // (col,val) pairs a multi-pass row may park in HBM per block (2 MB)
constexpr int BH_MAXCLS = 32;                  // hash classes (passes) with their own parking region
// direct big-row kernel (k_num_bigdirect; the scheme: "the re-hit log kit" above)
#ifndef SMF_BD_U
#define SMF_BD_U 4
#endif
constexpr int BD_U = SMF_BD_U;                  // rounds in flight per wave (read-only probes: no CAS chains to keep short)
constexpr int BD_MIN_SLOTS = 1024;             // smallest table of a row (a row without re-hits still sweeps it)
constexpr int RL_ROW_BUDGET = 2048;            // log ints per big row when the workspace is sized (see grow_rehit_log)
constexpr int RL_MIN_REGION = 1 << 15;         // ... and the smallest region of a block

struct BigSymShared {
  unsigned bitmap[SYM_WORDS];
  WalkStageN<BIG_NW> st;
  int red[BIG_NW];
  int logCnt;                    // LOG: re-hits of the current row so far; the row's region ran out (or the row passed rlCap)
  int logOvf;
};
constexpr int BIG_GROUPS = BIG_WORDS / WAVE;   // 128 groups of 64 bitmap words
constexpr int BIG_GPW = BIG_GROUPS / BIG_NW;   // 8 groups per wave, interleaved (dense column ranges spread over all waves)
struct BigNumShared {
  unsigned bitmap[BIG_WORDS];
  int prefix[BIG_WORDS];
  float acc[BIG_CAP];
  WalkStageN<BIG_NW> st;
  int red[BIG_NW];
  int gtot[BIG_GROUPS];
  int gbase[BIG_GROUPS];
  int cnt;
};
struct BigHashShared {
  slot_t tab[BH_SLOTS];          // (column, value) pairs
  WalkStageN<BIG_NW> st;
  int red[BIG_NW];
  int spillCnt[BH_MAXCLS];
  int emitted;
  int ovf;                       // a parking region overflowed: redo the row without parking
  int full;                      // a hash class outgrew the table: redo the row with more, better mixed classes
};
static_assert(sizeof(BigHashShared) <= 160 * 1024, "k_num_bighash: more LDS than a CU has");

__device__ __forceinline__ int block_sum_16(int v, int* red) {
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int ws = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[w] = ws;
  __syncthreads();
  int tot = 0;
  for (int i = 0; i < BIG_NW; ++i) tot += red[i];
  return tot;
}

// saveBitmaps: device buffer of saveCap row slots x BIG_WORDS words (may be null / 0); only used when n <= BIG_WC
// LOG (n > BIG_WC, for k_num_bigdirect): the logging symbolic pass of the kit.  The bitmap update returns the old word, and
// a product whose bit was already set is a re-hit.  Log space: the block's own region of rlLog (rlRegion ints per block,
// filled front to back over the block's rows).  Row q of the bin (queue order) gets rlMeta[q] = {first log entry (index
// into rlLog), re-hits or -1}.  Rows that will not take the direct kernel (count -1, or q >= rlRows: no metadata slot) are
// appended to fbList, *fbCount counts them.  The row's IC entry is the popcount either way.
template <bool LOG>
__global__ __launch_bounds__(BIG_THREADS) void k_sym_big(const int* __restrict__ binPtr, int bin,
                                                         const int* __restrict__ rowIds,
                                                         const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                         const int* __restrict__ JB,
                                                         int n, int* __restrict__ IC,
                                                         unsigned* __restrict__ saveBitmaps, int saveCap,
                                                         int* __restrict__ qctr,
                                                         int2* __restrict__ rlMeta, int rlRows, int* __restrict__ rlLog,
                                                         int rlRegion, int rlCap, int* __restrict__ fbList,
                                                         int* __restrict__ fbCount) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BigSymShared& sh = *reinterpret_cast<BigSymShared*>(smem_raw);
  const int tid = threadIdx.x;
  const int first = binPtr[bin], count = binPtr[bin + 1] - first;
  int cursor = 0;                                      // LOG: ints of this block's region in use (block-uniform)
  int* const myLog = LOG ? rlLog + (size_t)blockIdx.x * (size_t)rlRegion : nullptr;
  // the next row is dequeued and its metadata requested before this row's work starts: the dependent chain
  // queue -> rowIds -> IA (three memory round trips) hides behind the row instead of preceding it
  int q = next_row(qctr, &sh.red[0]);
  RowMeta cur = load_meta_sym(rowIds + first, q, count, IA, IA);
  while (q < count) {
    const int qn = next_row(qctr, &sh.red[0]);
    const RowMeta nxt = load_meta_sym(rowIds + first, qn, count, IA, IA);
    const int row = cur.row;
    const int as = cur.as, ae = cur.ae;
    int total = 0;
    const bool logging = LOG && q < rlRows;            // block-uniform
    const int room = logging ? min(rlCap, rlRegion - cursor) : 0;
    int logged = 0, logOvf = 0;
    // by window index: w0 += SYM_WC would overflow past the last window of an n > 2^31 - SYM_WC (w0 <= 2047 * SYM_WC here)
    for (int wi = 0, nwin = (int)(((unsigned)n + (unsigned)(SYM_WC - 1)) / (unsigned)SYM_WC); wi < nwin; ++wi) {
      const int w0 = wi * SYM_WC;
      const int wc = min(SYM_WC, n - w0);
      const int words = (wc + 31) >> 5;
      const int words4 = (words + 3) & ~3;             // the bitmap is cleared and counted four words at a time
      for (int i = tid * 4; i < words4; i += BIG_THREADS * 4) *reinterpret_cast<uint4*>(&sh.bitmap[i]) = make_uint4(0u, 0u, 0u, 0u);
      if (LOG && w0 == 0 && tid == 0) { sh.logCnt = 0; sh.logOvf = 0; }
      __syncthreads();
      for_each_product<BIG_NW, BIG_U, false>(sh.st, as, ae, SBL, nullptr, JB, nullptr,
                                             [&](const bool (&act)[BIG_U], const int (&col)[BIG_U], const float (&)[BIG_U], int) {
        bool rehit[BIG_U];
#pragma unroll
        for (int u = 0; u < BIG_U; ++u) {            // predicated by value: OR-ing 0 changes nothing
          const int c = col[u] - w0;
          const bool ok = act[u] && (unsigned)c < (unsigned)wc;
          const unsigned bit = ok ? 1u << (c & 31) : 0u;
          if constexpr (LOG) {
            const unsigned old = atomicOr(ok ? &sh.bitmap[c >> 5] : reinterpret_cast<unsigned*>(&sh.st.dummy[lane_id()]), bit);
            rehit[u] = (old & bit) != 0u;              // bit = 0 for a lane without a product
          } else {
            atomicOr(ok ? &sh.bitmap[c >> 5] : reinterpret_cast<unsigned*>(&sh.st.dummy[lane_id()]), bit);
            rehit[u] = false;
          }
        }
        // block-uniform; no room: a row for the fallback kernel anyway
        if constexpr (LOG) if (logging) rehit_log_append(rehit, col, &sh.logCnt, &sh.logOvf, myLog, cursor, room);
      });
      if constexpr (LOG) { logged = sh.logCnt; logOvf = sh.logOvf; }   // after the walk's closing barrier; reset only behind block_sum_16's
      int mine = 0;
      for (int i = tid * 4; i < words4; i += BIG_THREADS * 4) {
        const uint4 v4 = *reinterpret_cast<const uint4*>(&sh.bitmap[i]);
        mine += __popc(v4.x) + __popc(v4.y) + __popc(v4.z) + __popc(v4.w);
      }
      if (n <= BIG_WC && q < saveCap) {
        unsigned* dst = saveBitmaps + (size_t)q * BIG_WORDS;
        for (int i = tid; i < BIG_WORDS; i += BIG_THREADS) dst[i] = i < words ? sh.bitmap[i] : 0u;
      }
      total += block_sum_16(mine, sh.red);
      __syncthreads();
    }
    if (tid == 0) IC[row] = total;
    if constexpr (LOG) {
      const bool direct = logging && !logOvf;          // then logged <= room <= rlCap
      if (tid == 0) {
        if (q < rlRows) rlMeta[q] = make_int2((int)(blockIdx.x * (unsigned)rlRegion) + cursor, direct ? logged : -1);
        if (!direct) fbList[atomicAdd(fbCount, 1)] = row;
      }
      if (direct) cursor += logged;
    }
    cur = nxt;
    q = qn;
  }
}

// numeric A (n <= BIG_WC): rank kernel
__global__ __launch_bounds__(BIG_THREADS) void k_num_big(const int* __restrict__ binPtr, int bin,
                                                         const int* __restrict__ rowIds,
                                                         const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                         const float* __restrict__ VA,
                                                         const int* __restrict__ JB,
                                                         const float* __restrict__ VB, int n,
                                                         const int* __restrict__ IC, int* __restrict__ JC,
                                                         float* __restrict__ C, int* __restrict__ err,
                                                         const unsigned* __restrict__ savedBitmaps, int savedCap,
                                                         int* __restrict__ qctr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BigNumShared& sh = *reinterpret_cast<BigNumShared*>(smem_raw);
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int first = binPtr[bin], count = binPtr[bin + 1] - first;
  for (int q = next_row(qctr, &sh.red[0]); q < count; q = next_row(qctr, &sh.red[0])) {
    const int row = rowIds[first + q];
    const int as = IA[row], ae = IA[row + 1];
    const int outBase = IC[row];
    const int outEnd = IC[row + 1];
    // which columns occur: reload the symbolic pass's bitmap, or rebuild it
    if (q < savedCap) {
      const unsigned* src = savedBitmaps + (size_t)q * BIG_WORDS;
      for (int i = tid; i < BIG_WORDS; i += BIG_THREADS) sh.bitmap[i] = src[i];
      __syncthreads();
    } else {
      for (int i = tid; i < BIG_WORDS; i += BIG_THREADS) sh.bitmap[i] = 0u;
      __syncthreads();
      for_each_product<BIG_NW, BIG_U, false>(sh.st, as, ae, SBL, nullptr, JB, nullptr,
                                             [&](const bool (&act)[BIG_U], const int (&col)[BIG_U], const float (&)[BIG_U], int) {
#pragma unroll
        for (int u = 0; u < BIG_U; ++u) {
          const bool ok = act[u] && (unsigned)col[u] < (unsigned)n;
          atomicOr(&sh.bitmap[ok ? col[u] >> 5 : 0], ok ? 1u << (col[u] & 31) : 0u);
        }
      });
    }
    // exclusive popcount prefix over the words.  Wave w owns the 64-word groups w, w+16, ...: consecutive lanes
    // read consecutive words (no bank conflicts) and a dense column range is shared by all waves.
    int lexcl[BIG_GPW];
#pragma unroll
    for (int si = 0; si < BIG_GPW; ++si) {
      const int g = w + si * BIG_NW;
      const int pc = __popc(sh.bitmap[g * WAVE + lane]);
      const int incl = wave_incl_add(pc);
      lexcl[si] = incl - pc;
      if (lane == 63) sh.gtot[g] = incl;
    }
    __syncthreads();
    if (w == 0) {
      const int s0 = sh.gtot[2 * lane], s1 = sh.gtot[2 * lane + 1];
      const int incl = wave_incl_add(s0 + s1);
      sh.gbase[2 * lane] = incl - s0 - s1;
      sh.gbase[2 * lane + 1] = incl - s1;
      if (lane == 63) sh.cnt = incl;
    }
    __syncthreads();
    int cntw = sh.cnt;
#pragma unroll
    for (int si = 0; si < BIG_GPW; ++si) {
      const int g = w + si * BIG_NW;
      lexcl[si] += sh.gbase[g];
      sh.prefix[g * WAVE + lane] = lexcl[si];
    }
    __syncthreads();
    if (outBase + cntw != outEnd) { if (tid == 0) atomicOr(err, ERRF_COUNT_MISMATCH); cntw = min(cntw, max(0, outEnd - outBase)); }
    // BIG_CAP ranks at a time: column indices first (already sorted; scattered into LDS by rank, then stored
    // coalesced), then the values accumulated by rank
    int* accI = reinterpret_cast<int*>(sh.acc);
    for (int lo = 0; lo < cntw; lo += BIG_CAP) {
      const int span = min(BIG_CAP, cntw - lo);
#pragma unroll
      for (int si = 0; si < BIG_GPW; ++si) {
        const int wd = (w + si * BIG_NW) * WAVE + lane;
        unsigned bits = sh.bitmap[wd];
        int pos = lexcl[si] - lo;
        const int cbase = wd * 32;
        while (bits) {
          const int b = __ffs(bits) - 1;
          bits &= bits - 1;
          if ((unsigned)pos < (unsigned)span) accI[pos] = cbase + b;
          ++pos;
        }
      }
      __syncthreads();
      for (int i = tid; i < span; i += BIG_THREADS) st_out(JC + outBase + lo + i, accI[i]);
      __syncthreads();
      for (int i = tid; i < span; i += BIG_THREADS) sh.acc[i] = 0.f;
      __syncthreads();
      for_each_product<BIG_NW, BIG_U, true>(sh.st, as, ae, SBL, VA, JB, VB,
                                            [&](const bool (&act)[BIG_U], const int (&col)[BIG_U], const float (&val)[BIG_U], int) {
        int rk[BIG_U];
#pragma unroll
        for (int u = 0; u < BIG_U; ++u) {          // the U rank lookups (two LDS reads each) overlap
          const int c = act[u] && (unsigned)col[u] < (unsigned)n ? col[u] : 0;
          const int wi = c >> 5;
          rk[u] = sh.prefix[wi] + __popc(sh.bitmap[wi] & ((1u << (c & 31)) - 1u)) - lo;
        }
        bool ok[BIG_U];
#pragma unroll
        for (int u = 0; u < BIG_U; ++u)
          ok[u] = act[u] && (unsigned)col[u] < (unsigned)n && (unsigned)rk[u] < (unsigned)span;
        lds_fadd_multi(sh.acc, rk, ok, val, reinterpret_cast<int*>(&sh.st.dummy[lane_id()]));
      });
      for (int i = tid; i < span; i += BIG_THREADS) st_out(C + outBase + lo + i, sh.acc[i]);
      __syncthreads();
    }
    __syncthreads();
  }
}

// numeric B (any n): multi-pass LDS hash.  A row with more distinct columns than one table holds takes npass passes,
// pass k owning the columns of hash class k.  Only pass 0 walks the products: what belongs to a later class is
// parked as (col, a*b) pairs in a per-block HBM buffer and the later passes stream that buffer (coalesced, no
// search, no gather).  Rows with more products than the buffer holds fall back to walking once per pass.
__device__ __forceinline__ unsigned bh_class(int col, unsigned npass) {
  return ((((unsigned)col * 0x85ebca6bu) >> 16) * npass) >> 16;     // second hash, independent of the slot hash
}
// One multiplication cannot spread every input: the columns i*s of a banded or grid row are an arithmetic progression, and
// for some strides s (5599 and its small multiples, 509, ...) the products s*0x85ebca6b stay in a narrow range of the top 16
// bits, so that ALL of them land in one class, whatever npass.  A class that outgrows the table is noticed by the block
// (BigHashShared::full) and the row is redone with twice the classes, cut by this full avalanche mixer (murmur3's
// finaliser) salted with the attempt, BH_RETRIES times at most before the call fails.  The first attempt keeps the cheap
// function: it is on the hot path of every multi-pass row, and real rows pass it.
// Cost of a failed attempt: the flag is read at the end of the pass, and until then every trip that brings a column the full
// table cannot take probes all of its slots before it gives up, so a resonant row pays its walk several times over before
// the redo (milliseconds for a row of 300 000 columns; DESIGN.md 2b has the measured test times).  Rows that fit never enter
// that loop.  The state after the last retry has failed too (ERRF_TABLE_FULL, and ERRF_COUNT_MISMATCH because the emitted
// counter was reset) needs an input built against the salted mixer: no test reaches it.
constexpr int BH_RETRIES = 3;
__device__ __forceinline__ unsigned bh_class_mixed(int col, unsigned npass, int attempt) {
  unsigned x = (unsigned)col ^ ((unsigned)attempt * 0x9e3779b9u);
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return __umulhi(x, npass);
}

#ifdef SMF_STAMPS
// diagnostic build: cycles of wave 0 of every block, summed per phase of k_num_bighash (read with spgemm_hip_debug_stamps)
__device__ unsigned long long g_stamps[16];
#define STAMP_DECL unsigned long long st_[12] = {0,0,0,0,0,0,0,0,0,0,0,0}; unsigned long long t_ = __builtin_readcyclecounter(); const unsigned long long t0_ = t_;
#define STAMP(i) { const unsigned long long n_ = __builtin_readcyclecounter(); st_[i] += n_ - t_; t_ = n_; }
#define STAMP_IN(var) const unsigned long long var = __builtin_readcyclecounter();
#define STAMP_OUT(i, var) { st_[i] += __builtin_readcyclecounter() - var; }
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_IN(var)
#define STAMP_OUT(i, var)
#endif
__global__ __launch_bounds__(BIG_THREADS) void k_num_bighash(const int* __restrict__ binPtr, int bin,
                                                             const int* __restrict__ rowIds,
                                                             const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                             const float* __restrict__ VA,
                                                             const int* __restrict__ JB,
                                                             const float* __restrict__ VB,
                                                             const int* __restrict__ IC, int* __restrict__ JC,
                                                             float* __restrict__ C, int* __restrict__ err,
                                                             int* __restrict__ qctr, const int* __restrict__ rowFlops,
                                                             int2* __restrict__ spill, int spillCap, int bhCap, int marginPct) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BigHashShared& sh = *reinterpret_cast<BigHashShared*>(smem_raw);
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int first = binPtr[bin], count = binPtr[bin + 1] - first;
  int2* const park = spill ? spill + (size_t)blockIdx.x * (size_t)spillCap : nullptr;
  if (tid < WAVE) sh.st.dummy[tid] = DUMMY_SLOT;
  STAMP_DECL
  int q = next_row(qctr, &sh.red[0]);                 // one row ahead, as in k_sym_big
  RowMeta cur = load_meta_num(rowIds + first, q, count, IA, IC, rowFlops);
  while (q < count) {
    const int qn = next_row(qctr, &sh.red[0]);
    const RowMeta nxt = load_meta_num(rowIds + first, qn, count, IA, IC, rowFlops);
    const int as = cur.as, ae = cur.ae;
    const int outBase = cur.x0;
    const int outEnd = cur.x1;
    const int want = outEnd - outBase;
    unsigned classes = (unsigned)((want + bhCap - 1) / bhCap);
    const int flops = cur.x2;
    STAMP(0)
    // One attempt at the row with `npass` classes; true when a class held more columns than the table has slots (sh.full).
    // RETRY (a type, so that the first attempt compiles to the code it always was and the redo sits beside it, cold): the
    // classes are cut by bh_class_mixed and the table is used whole.
    auto attempt_row = [&](auto retry, const unsigned npass, const int attempt) -> bool {
      constexpr bool RETRY = decltype(retry)::value;
      // class c >= 1 parks in its own region of `stride` pairs: the expected class size (the classes are a hash of the
      // column, so products/npass) plus a margin.  A class that outgrows its region raises sh.ovf and the row is redone
      // the slow way (one walk per pass) -- rare, and never wrong.
      const int stride = (int)min((long long)flops, (long long)flops * marginPct / (100ll * (long long)npass) + 256ll);
      const bool canSpill = npass > 1 && npass <= (unsigned)BH_MAXCLS && park != nullptr &&
                            (long long)(npass - 1) * stride <= (long long)spillCap;
      const int perPass = (want + (int)npass - 1) / (int)npass;
      // any multiple of 1024 slots: FOUR times the distinct columns of a pass when that fits (2x / 3x / 4x: 0.845 / 0.832 /
      // 0.830 ms -- the lock-step probe loop pays for the longest chain of its 128 products, see table_size); a redone row
      // takes the whole table
      const int size = RETRY ? BH_SLOTS : min(BH_SLOTS, max(BIG_THREADS, (4 * perPass + BIG_THREADS - 1) / BIG_THREADS * BIG_THREADS));
      const int shift = 0;
      const int per = size / BIG_NW;
      bool useSpill = canSpill;
      bool full = false;
      for (unsigned pass = 0; pass < npass;) {
        clear_slots(sh.tab, size, tid, BIG_THREADS);
        if (pass == 0 && tid < BH_MAXCLS) sh.spillCnt[tid] = 0;
        if (pass == 0 && tid == 0) { sh.emitted = 0; sh.ovf = 0; sh.full = 0; }
        __syncthreads();
        STAMP(1)
        if (pass == 0 || !useSpill) {
          for_each_product<BIG_NW, BH_U, true>(sh.st, as, ae, SBL, VA, JB, VB,
                                                [&](const bool (&act)[BH_U], const int (&col)[BH_U], const float (&val)[BH_U], int) {
            STAMP_IN(ti_)
            bool mine[BH_U];
            unsigned cls[BH_U];
#pragma unroll
            for (int u = 0; u < BH_U; ++u) {
              cls[u] = npass == 1 ? 0u : RETRY ? bh_class_mixed(col[u], npass, attempt) : bh_class(col[u], npass);
              mine[u] = act[u] && cls[u] == pass;
            }
            hash_accum_multi<false>(sh.tab, size, shift, mine, col, val, &sh.st.dummy[lane_id()], &sh.full);
            STAMP_OUT(3, ti_)
            STAMP_IN(tp_)
            if (useSpill) {                              // block-uniform; here pass == 0
              for (unsigned c = 1; c < npass; ++c) {
                unsigned long long mk[BH_U];
                int total = 0;
#pragma unroll
                for (int u = 0; u < BH_U; ++u) { mk[u] = ballot64(act[u] && cls[u] == c); total += __popcll(mk[u]); }
                if (total) {                             // wave-uniform
                  int base = 0;
                  if (lane == 0) base = atomicAdd(&sh.spillCnt[c], total);
                  base = __builtin_amdgcn_readfirstlane(base);
                  if (base + total > stride) {           // wave-uniform: region full, the row will be redone
                    if (lane == 0) sh.ovf = 1;
                  } else {
                    int2* const dst = park + (size_t)(c - 1) * (size_t)stride;
#pragma unroll
                    for (int u = 0; u < BH_U; ++u) {
                      if (act[u] && cls[u] == c) dst[base + mask_rank(mk[u])] = make_int2(col[u], __float_as_int(val[u]));
                      base += __popcll(mk[u]);
                    }
                  }
                }
              }
            }
            STAMP_OUT(4, tp_)
          });
          STAMP(2)
          if (pass == 0 && useSpill && sh.ovf) {        // block-uniform (read after the walk's closing barrier)
            __syncthreads();                             // everyone has seen the flag before it is reset
            useSpill = false;
            continue;                                    // pass 0 again, without parking: table and counters are reset
          }
        } else {
          // stream this class's parked pairs; the next batch is in flight while the current one is inserted
          const int cnt = sh.spillCnt[pass];            // written in pass 0, read-only since its closing barrier
          const int2* const src = park + (size_t)(pass - 1) * (size_t)stride;
          int2 nxt[BH_U];
#pragma unroll
          for (int u = 0; u < BH_U; ++u) { const int idx = u * BIG_THREADS + tid; nxt[u] = src[idx < cnt ? idx : 0]; }
          for (int i0 = 0; i0 < cnt; i0 += BIG_THREADS * BH_U) {
            bool mine[BH_U];
            int col[BH_U];
            float val[BH_U];
#pragma unroll
            for (int u = 0; u < BH_U; ++u) {
              col[u] = nxt[u].x;
              val[u] = __int_as_float(nxt[u].y);
              mine[u] = i0 + u * BIG_THREADS + tid < cnt;
            }
#pragma unroll
            for (int u = 0; u < BH_U; ++u) {
              const int idx = i0 + BIG_THREADS * BH_U + u * BIG_THREADS + tid;
              nxt[u] = src[idx < cnt ? idx : 0];
            }
            hash_accum_multi<false>(sh.tab, size, shift, mine, col, val, &sh.st.dummy[lane_id()], &sh.full);
          }
          __syncthreads();
          STAMP(5)
        }
        if (sh.full) {                                   // block-uniform (every insert of the pass is behind a barrier)
          __syncthreads();                               // everyone has seen the flag before the next attempt resets it
          full = true;
          break;
        }
        // compaction: wave w emits the slots [w*per, w*per+per); its share of the row's output range comes from one
        // LDS atomic (the counter runs on across the passes of a row)
        emit_claimed<BH_SLOTS / BIG_NW / WAVE>(sh.tab, w * per, per, &sh.emitted, outBase, outEnd, JC, C);
        __syncthreads();
        STAMP(6)
        ++pass;
      }
      return full;
    };
    // The row as planned; if a class outgrew the table, again with twice the classes and the mixed class function, a few
    // times at most.  The row's output range is its own, so what the passes of a failed attempt wrote is written again.
    bool full = attempt_row(std::false_type{}, classes, 0);
    for (int attempt = 1; full && attempt <= BH_RETRIES; ++attempt) {
      classes *= 2;
      full = attempt_row(std::true_type{}, classes, attempt);
    }
    if (full && tid == 0) atomicOr(err, ERRF_TABLE_FULL);
    if (tid == 0 && sh.emitted != want) atomicOr(err, ERRF_COUNT_MISMATCH);
    __syncthreads();
    cur = nxt;
    q = qn;
    STAMP(7)
  }
#ifdef SMF_STAMPS
  if (tid == 0) {
    for (int i = 0; i < 8; ++i) atomicAdd(&g_stamps[i], st_[i]);
    atomicAdd(&g_stamps[8], __builtin_readcyclecounter() - t0_);
    atomicAdd(&g_stamps[9], 1ull);
  }
#endif
}

// numeric C (n > BIG_WC, rows whose re-hits k_sym_big<true> logged): the kit's numeric pass with one block of NW waves per
// row; the position of a trip's misses is drawn from the row's counter (one LDS atomic per wave and trip).  The rows it
// skips are in the fallback list k_num_bighash runs over.  The queue is the bin's own (largest rows first).
template <int NW, int S>
struct BigDirectShared {
  slot_t tab[S];
  WalkStageN<NW> st;
  int red[NW];
  int emitted;
};

template <int NW, int S>
__global__ __launch_bounds__(WAVE * NW) void k_num_bigdirect(const int* __restrict__ binPtr, int bin,
                                                             const int* __restrict__ rowIds,
                                                             const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                             const float* __restrict__ VA,
                                                             const int* __restrict__ JB,
                                                             const float* __restrict__ VB,
                                                             const int* __restrict__ IC, int* __restrict__ JC,
                                                             float* __restrict__ C, int* __restrict__ err,
                                                             int* __restrict__ qctr, const int2* __restrict__ rlMeta,
                                                             int rlRows, const int* __restrict__ rlLog) {
  static_assert(S % (WAVE * NW) == 0 && BD_MIN_SLOTS % (WAVE * NW) == 0, "every wave sweeps whole 64-slot steps");
  constexpr int T = WAVE * NW;
  constexpr int CAP = bd_cap(S);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  BigDirectShared<NW, S>& sh = *reinterpret_cast<BigDirectShared<NW, S>*>(smem_raw);
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int first = binPtr[bin], count = binPtr[bin + 1] - first;
  if (tid < WAVE) sh.st.dummy[tid] = DUMMY_SLOT;
  // one row ahead, as in k_sym_big; rlMeta goes by the queue position and has rlRows entries
  auto load = [&](int qq) {
    return load_meta_logged(rowIds + first, qq, min(count, rlRows), IA, IC, nullptr, rlMeta, false,
                            [&](int2 lm) { return lm.y >= 0 && lm.y <= CAP; });
  };
  int q = next_row(qctr, &sh.red[0]);
  LoggedMeta cur = load(q);
  while (q < count) {
    const int qn = next_row(qctr, &sh.red[0]);
    const LoggedMeta nxt = load(qn);
    if (cur.lc >= 0) {                                 // block-uniform
      const int as = cur.m.as, ae = cur.m.ae;
      const int outBase = cur.m.x0, outEnd = cur.m.x1;
      const int want = outEnd - outBase;
      const int lc = cur.lc;
      // four slots per logged re-hit when that fits (the clear and the sweep are what a small table saves)
      const int size = table_size<4>(lc, BD_MIN_SLOTS, S);
      const int shift = 32 - log2_pow2(size);
      const int per = size / NW;
      clear_slots(sh.tab, size, tid, T);
      if (tid == 0) sh.emitted = 0;
      __syncthreads();
      fill_from_log(sh.tab, size, shift, rlLog + cur.ls, lc, tid, T);
      __syncthreads();
      int* const JCrow = JC + outBase;
      float* const Crow = C + outBase;
      const unsigned lim = (unsigned)max(want, 0);     // every store stays inside the row's own range
      for_each_product<NW, BD_U, true>(sh.st, as, ae, SBL, VA, JB, VB,
                                       [&](const bool (&act)[BD_U], const int (&col)[BD_U], const float (&val)[BD_U], int) {
        char* const base = reinterpret_cast<char*>(sh.tab);
        const int dumB = (int)(reinterpret_cast<char*>(&sh.st.dummy[lane]) - base);
        bool miss[BD_U];
        probe_rounds(base, dumB, size, shift, act, col, val, err, miss);
        store_misses_claimed(miss, col, val, &sh.emitted, lim, JCrow, Crow);
      });
      // (the walk ends with a barrier behind its last LDS atomics)
      emit_claimed<S / NW / WAVE>(sh.tab, w * per, per, &sh.emitted, outBase, outEnd, JC, C);
      __syncthreads();
      if (tid == 0 && sh.emitted != want) atomicOr(err, ERRF_COUNT_MISMATCH);
      __syncthreads();
    }
    cur = nxt;
    q = qn;
  }
}

// numeric, bins 6-7 (513-4096 products) of a float product whose symbolic pass logged (k_sym_hash<.., true>): the kit's
// numeric pass like k_num_bigdirect, with a table of at most S slots (1024: 8 KB, where k_num_hash clears, fills and sweeps
// 16-64 KB per row).  The rows it skips are in the bin's fallback list that k_num_hash runs over.  An expanded row takes its
// positions from the walk's dense numbering, which lives in the table's memory.
#ifndef SMF_MD_U
#define SMF_MD_U 4
#endif
constexpr int MD_U = SMF_MD_U;                  // rounds in flight per wave, as in k_num_bigdirect (2 measured the same)
template <int NW, int S>
struct MidDirectShared {
  slot_t tab[S];
  WalkStageN<NW> st;
  int qslot;
  int emitted;
};
template <int NW, int S>
__global__ __launch_bounds__(WAVE * NW) void k_num_middirect(const int* __restrict__ binPtr, int bin,
                                                             const int* __restrict__ rowIds,
                                                             const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                             const float* __restrict__ VA,
                                                             const int* __restrict__ JB,
                                                             const float* __restrict__ VB,
                                                             const int* __restrict__ IC, int* __restrict__ JC,
                                                             float* __restrict__ C, int* __restrict__ err,
                                                             int* __restrict__ qctr, const int* __restrict__ rowFlops,
                                                             const int2* __restrict__ meta, const int* __restrict__ mlog,
                                                             long long logCap, int cap, int waveCap,
                                                             unsigned long long* __restrict__ took) {
  constexpr int T = WAVE * NW;
  static_assert(S % T == 0 && S / T <= 8, "every wave sweeps whole 64-slot steps");
  static_assert(sizeof(WalkNumber<NW>) <= S * sizeof(slot_t), "the numbering of an expanded row lives in the table");
  __shared__ __attribute__((aligned(16))) MidDirectShared<NW, S> sh;
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int first = binPtr[bin], count = binPtr[bin + 1] - first;
  const int* rows = rowIds + first;
  cap = min(cap, bd_cap(S));                           // a probe always ends at an empty slot
  constexpr int QB = NW >= 8 ? 2 : 4;                  // rows per dequeue, as in k_num_hash
  if (surplus_block(count, QB)) return;
  if (tid < WAVE) sh.st.dummy[tid] = DUMMY_SLOT;
  auto load = [&](int qq) {                            // the wave kernel's rows are not this one's
    return load_meta_logged(rows, qq, count, IA, IC, rowFlops, meta, true,
                            [&](int2 lm) { return lm.y >= 0 && lm.y <= cap && !midwave_takes(lm, logCap, waveCap); });
  };
  int q = next_row<QB>(qctr, &sh.qslot, -1);
  LoggedMeta cur = load(q);
  int tookRows = 0;                                    // rows of this block that went direct here (test hook)
  while (q < count) {
    const int qn = next_row<QB>(qctr, &sh.qslot, q);
    const LoggedMeta nxt = load(qn);
    const int as = cur.m.as, ae = cur.m.ae;
    const int outBase = cur.m.x0, outEnd = cur.m.x1;
    const int want = outEnd - outBase;
    int* const JCrow = JC + outBase;
    float* const Crow = C + outBase;
    const unsigned lim = (unsigned)max(want, 0);       // every store stays inside the row's own range
    // (block-uniform branches; a row's log must lie inside the log whatever the metadata says)
    const bool mine = cur.lc >= 0 && (long long)cur.ls >= 0 && (long long)cur.ls + cur.lc <= logCap;
    tookRows += __builtin_amdgcn_readfirstlane(mine ? 1 : 0);   // (block-uniform: kept in a scalar register)
    if (mine && want == cur.m.x2) {
      for_each_product<NW, MD_U, true>(sh.st, as, ae, SBL, VA, JB, VB, expanded_store(lane, lim, JCrow, Crow),
                                       PreA{0, 0, 0.f, false}, err, reinterpret_cast<WalkNumber<NW>*>(sh.tab));
    } else if (mine) {
      const int lc = cur.lc;
      // four slots per logged re-hit when that fits (the clear and the sweep are what a small table saves)
      const int size = table_size<4>(lc, T, S);
      const int shift = 32 - log2_pow2(size);
      const int per = size / NW;
      clear_slots(sh.tab, size, tid, T);
      if (tid == 0) sh.emitted = 0;
      __syncthreads();
      fill_from_log(sh.tab, size, shift, mlog + cur.ls, lc, tid, T);
      __syncthreads();
      for_each_product<NW, MD_U, true>(sh.st, as, ae, SBL, VA, JB, VB,
                                       [&](const bool (&act)[MD_U], const int (&col)[MD_U], const float (&val)[MD_U], int) {
        char* const base = reinterpret_cast<char*>(sh.tab);
        const int dumB = (int)(reinterpret_cast<char*>(&sh.st.dummy[lane]) - base);
        bool miss[MD_U];
        probe_rounds(base, dumB, size, shift, act, col, val, err, miss);
        store_misses_claimed(miss, col, val, &sh.emitted, lim, JCrow, Crow);
      });
      // (the walk ends with s_waitcnt lgkmcnt(0) and a barrier behind its last LDS atomics)
      emit_claimed<S / T>(sh.tab, w * per, per, &sh.emitted, outBase, outEnd, JC, C);
      __syncthreads();
      if (tid == 0 && sh.emitted != want) atomicOr(err, ERRF_COUNT_MISMATCH);
      __syncthreads();
    }
    cur = nxt;
    q = qn;
  }
  if (took && tid == 0 && tookRows) atomicAdd(took, (unsigned long long)tookRows);
}

// ---- bin 6, one wave per row (k_num_midwave).  The four waves k_num_middirect<4,1024> gives a row of 513-2048 products
// each run the whole per-row instruction stream -- dequeue, clear, log insert, staging, unit table, claim loop, sweep, twelve
// barriers -- for ONE trip of products.  Here a row has one wave and the wave-per-row walk (for_each_product<1>: no unit
// table, no claim counter, no barrier), in the ways of k_num_hash<1, ..>: static XCD-contiguous schedule, the next row's
// metadata and first A entries in flight one row ahead, up to 8 rounds gathered per trip.  The output position is a
// register of the wave: no LDS counter.  The rounds of a trip are probed MW_CH at a time (registers).
// Measured (profiles/README.md, "Mid rows: one wave per row"): 30 % fewer vector and scalar instructions than the four-wave
// kernel, and with one launch per layout slot the SAME time -- a static schedule of 4-9 rows per wave ends on its slowest
// wave, twice.  What pays is one launch over both slots with every wave's heavy rows first (MidWaveRows).
#ifndef SMF_MW_CH
#define SMF_MW_CH 4
#endif
constexpr int MW_CH = SMF_MW_CH;
struct MidWaveShared {
  slot_t tab[MW_SLOTS];
  WalkStage1 st;
};
// The rows of one launch: this XCD's eighth of the bin's second layout slot (1025-2048 products) FIRST, then its eighth of
// the first slot (513-1024), as one sequence that the waves of the XCD stride over -- a wave's heavy rows come first and the
// launch ends on the light ones (one launch per slot, each with its own tail: 2 x 0.150 ms; profiles/README.md).
struct MidWaveRows {
  const int* hi; int nhi;                              // (second slot)
  const int* lo; int nlo;
  __device__ __forceinline__ int count() const { return nhi + nlo; }
  __device__ __forceinline__ int operator[](int q) const { return q < nhi ? hi[q] : lo[q - nhi]; }
};
__global__ __launch_bounds__(WAVE) void k_num_midwave(const int* __restrict__ slotBase, int slotLo, int slotHi,
                                                      const int* __restrict__ rowIds,
                                                      const int* __restrict__ IA, const int2* __restrict__ SBL,
                                                      const float* __restrict__ VA,
                                                      const int* __restrict__ JB,
                                                      const float* __restrict__ VB,
                                                      const int* __restrict__ IC, int* __restrict__ JC,
                                                      float* __restrict__ C, int* __restrict__ err,
                                                      const int* __restrict__ rowFlops,
                                                      const int2* __restrict__ meta, const int* __restrict__ mlog,
                                                      long long logCap, int waveCap,
                                                      unsigned long long* __restrict__ took,
                                                      int* __restrict__ restList, int* __restrict__ restCount) {
  constexpr int S = MW_SLOTS;
  __shared__ __attribute__((aligned(16))) MidWaveShared sh;
  static_assert(sizeof(MidWaveShared) <= 6 * 1024, "24+ blocks of one wave share a CU");
  const int lane = lane_id();
  waveCap = min(waveCap, bd_cap(S));                   // a probe always ends at an empty slot
  sh.st.dummy[lane] = DUMMY_SLOT;
  MidWaveRows rows;                                    // static schedule: XCD-contiguous (see xcd_range)
  const XcdRange xh = xcd_range(slotBase[slotHi + 1] - slotBase[slotHi]);
  const XcdRange xl = xcd_range(slotBase[slotLo + 1] - slotBase[slotLo]);
  rows.hi = rowIds + slotBase[slotHi] + xh.lo; rows.nhi = xh.hi - xh.lo;
  rows.lo = rowIds + slotBase[slotLo] + xl.lo; rows.nlo = xl.hi - xl.lo;
  const int count = rows.count();
  const int stride = xh.nb;
  int q = xh.bi;
  // two rows of metadata and one row of A entries are in flight ahead of the row being processed
  // (a row with a log that this kernel does not take goes on k_num_middirect's list)
  __builtin_assume(rowFlops != nullptr);
  auto load = [&](int qq) {
    return load_meta_logged(rows, qq, count, IA, IC, rowFlops, meta, true,
                            [&](int2 lm) { return midwave_takes(lm, logCap, waveCap) ? 1 : lm.y >= 0 ? -1 : 0; });
  };
  LoggedMeta cur = load(q);
  LoggedMeta nxt = load(q + stride);
  PreA pc = load_pre(cur.m, SBL, VA, true);            // (a row of the other kernels: as = ae = 0, nothing is read)
  int tookRows = 0;
  while (q < count) {
    const int qn = q + stride;
    const LoggedMeta nn = load(qn + stride);
    const PreA pn = load_pre(nxt.m, SBL, VA, true);
    if (cur.lc >= 0) {                                 // wave-uniform
      ++tookRows;
      const int want = cur.m.x1 - cur.m.x0;
      int* const JCrow = JC + cur.m.x0;
      float* const Crow = C + cur.m.x0;
      const unsigned lim = (unsigned)max(want, 0);     // every store stays inside the row's own range
      if (want == cur.m.x2) {
        // no repeated column: expanded, every product at its place in the walk's numbering of the row
        for_each_product<1, 2, true>(sh.st, cur.m.as, cur.m.ae, SBL, VA, JB, VB, expanded_store(lane, lim, JCrow, Crow), pc, err);
      } else {
        const int lc = cur.lc;
        // four slots per logged re-hit when that fits (the clear and the sweep are what a small table saves)
        const int size = table_size<4>(lc, WAVE, S);
        const int shift = 32 - log2_pow2(size);
        clear_slots(sh.tab, size, lane, WAVE);
        wave_lds_sync();
        fill_from_log(sh.tab, size, shift, mlog + cur.ls, lc, lane, WAVE);
        wave_lds_sync();
        char* const base = reinterpret_cast<char*>(sh.tab);
        const int dumB = (int)(reinterpret_cast<char*>(&sh.st.dummy[lane]) - base);
        int pos = 0;                                   // next free place of the row's range: wave-uniform, a register
        for_each_product<1, 2, true>(sh.st, cur.m.as, cur.m.ae, SBL, VA, JB, VB,
                                     [&](const auto& act, const auto& col, const auto& val, int) {
          constexpr int R = (int)(sizeof(col) / sizeof(col[0]));
          constexpr int CH = MW_CH <= 0 || MW_CH > R ? R : MW_CH;
#pragma unroll
          for (int c0 = 0; c0 < R; c0 += CH) {
            bool a_[CH]; int c_[CH]; float v_[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
              const int i = c0 + u < R ? c0 + u : 0;
              a_[u] = c0 + u < R ? act[i] : false; c_[u] = col[i]; v_[u] = val[i];
            }
            bool miss[CH];
            probe_rounds(base, dumB, size, shift, a_, c_, v_, err, miss);
            pos = store_misses(miss, c_, v_, pos, lim, JCrow, Crow);
          }
        }, pc, err);
        wave_lds_sync();                               // the adds have landed: the sweep reads their sums
        for (int i0 = 0; i0 < size; i0 += WAVE) {
          const slot_t sv = sh.tab[i0 + lane];
          const bool occ = slot_key(sv) != EMPTY_KEY;
          const unsigned long long mk = ballot64(occ);
          const unsigned o = (unsigned)(pos + mask_rank(mk));
          if (occ && o < lim) { st_out(JCrow + o, slot_key(sv)); st_out(Crow + o, slot_val(sv)); }
          pos += __popcll(mk);
        }
        if (lane == 0 && pos != want) atomicOr(err, ERRF_COUNT_MISMATCH);
        wave_lds_sync();                               // the next row clears the table behind the sweep's reads
      }
    } else if (cur.ls) {                               // a logged row of the four-wave kernel: onto its list (at most one
      if (lane == 0) restList[atomicAdd(restCount, 1)] = cur.m.row;   // entry per row of the bin, which the list holds)
    }
    cur = nxt; nxt = nn; pc = pn;
    q = qn;
  }
  if (took && lane == 0 && tookRows) atomicAdd(took, (unsigned long long)tookRows);
}

// ------------------------------------------------------------------------------------------------
// Exclusive scan of IC[0..m) -> offsets, IC[m] = nnzC (64-bit total kept for the overflow check).
// Two launches: per-tile sums, then a rescan per tile whose block first adds up the sums of the tiles before its own
// (up to SCAN_FOLD_MAX tiles: 256 at a million rows, one value per thread).  Beyond that the sums before a tile are
// too many to add up in every block: a one-block launch scans them in between (k_scan_tiles), as the cut of the
// one-pass path does.
// (thrust::exclusive_scan in the reference: nlibs/gpus/gpu_csr_kernel.cu:149-150)
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 1024;
constexpr int SCAN_ITEMS = 4;                  // ints per thread
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

__global__ __launch_bounds__(SCAN_THREADS) void k_scan_tile_sums(int m, const int* __restrict__ IC,
                                                                  unsigned long long* __restrict__ tileSum) {
  __shared__ unsigned long long red[16];
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int base = blockIdx.x * SCAN_TILE + tid * SCAN_ITEMS;
  unsigned long long s = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) if (base + i < m) s += (unsigned)IC[base + i];
  s = wave_sum_u64(s);
  if (lane == 0) red[w] = s;
  __syncthreads();
  if (tid == 0) { unsigned long long t = 0; for (int i = 0; i < 16; ++i) t += red[i]; tileSum[blockIdx.x] = t; }
}

__global__ __launch_bounds__(1024) void k_scan_tiles(int ntiles, unsigned long long* __restrict__ tileSum,
                                                      unsigned long long* __restrict__ total) {
  __shared__ unsigned long long wsum[16];
  __shared__ unsigned long long running;
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  if (tid == 0) running = 0;
  __syncthreads();
  for (int t0 = 0; t0 < ntiles; t0 += 1024) {
    const int t = t0 + tid;
    const unsigned long long v = t < ntiles ? tileSum[t] : 0ull;
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    unsigned long long woff = 0, tot = 0;
    for (int i = 0; i < 16; ++i) { const unsigned long long s = wsum[i]; tot += s; if (i < w) woff += s; }
    const unsigned long long run = running;
    if (t < ntiles) tileSum[t] = run + woff + incl - v;    // exclusive
    __syncthreads();
    if (tid == 0) running = run + tot;
    __syncthreads();
  }
  if (tid == 0) *total = running;
}

// clampTotal: IC[m] = min(total, INT_MAX) (C.rowPtr: the host rejects an overflow anyway); otherwise the total wraps
// modulo 2^32 like the interior prefixes, so that differences of neighbours stay exact (the dflops scan of the
// classification API, whose consumers take differences).
// FOLD: tileSum holds the tiles' own sums (k_scan_tile_sums) and the last block writes *total; otherwise tileSum holds
// their exclusive scan and *total is there already (k_scan_tiles).
template <bool FOLD>
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_apply(int m, int* __restrict__ IC,
                                                              const unsigned long long* __restrict__ tileSum,
                                                              unsigned long long* __restrict__ total, int clampTotal) {
  __shared__ int wsum[16];
  __shared__ unsigned long long osum[16];
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const int base = blockIdx.x * SCAN_TILE + tid * SCAN_ITEMS;
  int v[SCAN_ITEMS];
  int s = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) { v[i] = base + i < m ? IC[base + i] : 0; s += v[i]; }
  unsigned long long before = 0;                           // FOLD: this thread's share of the tiles before the block's
  if (FOLD) {
    for (int t = tid; t < (int)blockIdx.x; t += SCAN_THREADS) before += tileSum[t];
    before = wave_sum_u64(before);
    if (lane == 0) osum[w] = before;
  }
  const int incl = wave_incl_add(s);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int woff = 0;
  for (int i = 0; i < w; ++i) woff += wsum[i];
  if (FOLD) { before = 0; for (int i = 0; i < 16; ++i) before += osum[i]; }
  else before = tileSum[blockIdx.x];
  int run = (int)before + woff + incl - s;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) { if (base + i < m) IC[base + i] = run; run += v[i]; }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {
    const unsigned long long t = FOLD ? before + tileSum[blockIdx.x] : *total;
    if (FOLD) *total = t;
    IC[m] = (clampTotal && t > 0x7fffffffULL) ? 0x7fffffff : (int)(unsigned)t;
  }
}

// ------------------------------------------------------------------------------------------------
// helpers for the reference-shaped classify outputs and for canonical ordering
// ------------------------------------------------------------------------------------------------
// gathered[q] = rowFlops[rowIds[q]]  (then scanned with the kernels above into dflops[1..m])
__global__ void k_gather_flops(int m, const int* __restrict__ rowIds, const int* __restrict__ rowFlops,
                               int* __restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < m) out[q] = rowFlops[rowIds[q]];
}

// CSR::makeOrdered on the device (nlibs/CSR.cc:73-86).  Rows of <= SORT_MAX entries: one block per row, bitonic sort in
// LDS (k_sort_rows, which also counts the longer rows that are not sorted yet).  Longer rows (the output of the big-row
// hash kernel: up to tens of thousands of entries): a per-row stable LSD radix sort over the column bits, 8 bits per
// pass, between the row's own segment of the arrays and of a scratch copy (k_sort_long_rows) -- the reference's device
// primitives for this are nlibs/bitonic_sort.cuh:19-87 and mindex2-cuda/radix_sort.cuh:2-62.
// Used by tests/drivers, not by the timed path.
constexpr int SORT_MAX = 4096;
template <class V>      // value type: float, or double for hip_csr_sort_rows_f64
__global__ __launch_bounds__(256) void k_sort_rows(int m, const int* __restrict__ IC, int* __restrict__ JC,
                                                    V* __restrict__ C, int* __restrict__ longUnsorted) {
  __shared__ int sk[SORT_MAX];
  __shared__ V sv[SORT_MAX];
  __shared__ int unsorted;
  const int tid = threadIdx.x;
  for (int row = blockIdx.x; row < m; row += gridDim.x) {
    const int s = IC[row], len = IC[row + 1] - s;
    if (len < 2) continue;
    if (len <= SORT_MAX) {
      int p2 = 1;
      while (p2 < len) p2 <<= 1;
      for (int i = tid; i < p2; i += 256) { sk[i] = i < len ? JC[s + i] : 0x7fffffff; sv[i] = i < len ? C[s + i] : V(0); }
      __syncthreads();
      for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = tid; i < p2; i += 256) {
            const int ixj = i ^ j;
            if (ixj > i) {
              const bool up = (i & k) == 0;
              const int a = sk[i], b = sk[ixj];
              if ((a > b) == up) { sk[i] = b; sk[ixj] = a; const V t = sv[i]; sv[i] = sv[ixj]; sv[ixj] = t; }
            }
          }
          __syncthreads();
        }
      }
      for (int i = tid; i < len; i += 256) { JC[s + i] = sk[i]; C[s + i] = sv[i]; }
      __syncthreads();
    } else {
      if (tid == 0) unsorted = 0;
      __syncthreads();
      int bad = 0;
      for (int i = tid; i + 1 < len; i += 256) bad |= JC[s + i] > JC[s + i + 1];
      if (bad) atomicOr(&unsorted, 1);
      __syncthreads();
      if (tid == 0 && unsorted) atomicAdd(longUnsorted, 1);
      __syncthreads();
    }
  }
}

// rows longer than SORT_MAX that are not sorted: stable LSD radix sort, 8 bits per pass over `keyBits` column bits,
// ping-pong between (JC, C) and (JS, CS) inside the row's own segment [IC[row], IC[row+1]); an odd number of passes
// ends with a copy back.  Block = 256 threads; a pass = histogram of the row, scan of the 256 counts, then rounds of
// 256 elements ranked with ballots (order inside the block = index order, so every pass is stable).
template <class V>
__global__ __launch_bounds__(256) void k_sort_long_rows(int m, const int* __restrict__ IC, int* __restrict__ JC,
                                                         V* __restrict__ C, int* __restrict__ JS, V* __restrict__ CS,
                                                         int keyBits) {
  constexpr int NWV = 4;
  __shared__ int hist[256];
  __shared__ int run[256];
  __shared__ int wcnt[NWV][256];
  __shared__ int woff[NWV][256];
  __shared__ int unsorted;
  const int tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  for (int row = blockIdx.x; row < m; row += gridDim.x) {
    const int s = IC[row], len = IC[row + 1] - s;
    if (len <= SORT_MAX) continue;                       // block-uniform
    if (tid == 0) unsorted = 0;
    __syncthreads();
    int bad = 0;
    for (int i = tid; i + 1 < len; i += 256) bad |= JC[s + i] > JC[s + i + 1];
    if (bad) atomicOr(&unsorted, 1);
    __syncthreads();
    const bool need = unsorted != 0;
    __syncthreads();
    if (!need) continue;
    int* kin = JC + s; V* vin = C + s;
    int* kout = JS + s; V* vout = CS + s;
    int passes = 0;
    for (int shift = 0; shift < keyBits; shift += 8, ++passes) {
      hist[tid] = 0;
      __syncthreads();
      for (int i = tid; i < len; i += 256) atomicAdd(&hist[(kin[i] >> shift) & 255], 1);
      __syncthreads();
      if (w == 0) {                                      // exclusive scan of the 256 counts by one wave, 4 per lane
        int c[4], t = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { c[q] = hist[lane * 4 + q]; t += c[q]; }
        int ex = wave_incl_add(t) - t;
#pragma unroll
        for (int q = 0; q < 4; ++q) { run[lane * 4 + q] = ex; ex += c[q]; }
      }
      __syncthreads();
      for (int i0 = 0; i0 < len; i0 += 256) {
#pragma unroll
        for (int q = 0; q < NWV; ++q) wcnt[q][tid] = 0;
        __syncthreads();
        const int i = i0 + tid;
        const bool valid = i < len;
        const int key = valid ? kin[i] : 0;
        const V val = valid ? vin[i] : V(0);
        const int d = (key >> shift) & 255;
        unsigned long long peers = ballot64(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          const unsigned long long mb = ballot64(valid && ((d >> b) & 1));
          peers &= ((d >> b) & 1) ? mb : ~mb;
        }
        const int rank = mask_rank(peers);
        if (valid && rank == 0) wcnt[w][d] = __popcll(peers);
        __syncthreads();
        {
          int r = run[tid];
#pragma unroll
          for (int q = 0; q < NWV; ++q) { woff[q][tid] = r; r += wcnt[q][tid]; }
          run[tid] = r;
        }
        __syncthreads();
        if (valid) { const int dst = woff[w][d] + rank; kout[dst] = key; vout[dst] = val; }
      }
      __threadfence_block();
      __syncthreads();
      int* tk = kin; kin = kout; kout = tk;
      V* tv = vin; vin = vout; vout = tv;
    }
    if (passes & 1) {                                    // the sorted row sits in the scratch segment
      for (int i = tid; i < len; i += 256) { kout[i] = kin[i]; vout[i] = vin[i]; }
    }
    __syncthreads();
  }
}

// (the R-MCL post-step on rows in HBM -- k_rmcl_stats / _compact / _move / _fix_rows, k_zip_extents -- is written once
// for float and double in rmcl_rows_device.hpp)

// self-test of the DPP scans / mask ranks against serial results computed by every lane
__global__ void k_selftest(const int* __restrict__ in, int* __restrict__ bad) {
  __shared__ int buf[WAVE];
  const int lane = lane_id();
  const int v = in[blockIdx.x * WAVE + lane];
  buf[lane] = v;
  const int a = wave_incl_add(v);
  const int mx = wave_incl_max(v & 0xffff);
  const unsigned long long mk = ballot64(v & 1);
  const int rk = mask_rank(mk);
  __syncthreads();
  int ea = 0, em = 0, er = 0;
  for (int i = 0; i <= lane; ++i) { ea += buf[i]; em = max(em, buf[i] & 0xffff); if (i < lane) er += buf[i] & 1; }
  if (a != ea || mx != em || rk != er || wave_sum(v) != __shfl(ea, 63, 64)) atomicAdd(bad, 1);
}

}  // namespace smf
