// Selection (mcl's -S, HipMCL's select) on a device CSR: every row keeps its k largest entries, and the R-MCL loop with
// that row cap.  The reference has no counterpart (its row rule only thresholds: computeThreshold /
// arrayThreshPruneNormalize); the semantics are this library's and are pinned by tests/topk_ref.py.
//
//   hip_csr_row_topk             row i keeps its min(len_i, k) best entries in their storage order
//   hip_csr_row_topk_limits      the longest row of the wave path / of the block path (pure host)
//   hip_gpuRmclIter_device_topk  per iteration X = hip_rmcl_expand_prune(Mgt, Mt), Mt = row_topk(X, k, NORMALISE)
//
// The order.  Entry a beats entry b iff va > vb, or va == vb and ca < cb, or both equal and a is stored before b (rows may
// repeat a column).  Values are compared in V through an ordered integer key (ordered_key), columns through
// ck = INT_MAX - column, so that "better" is "larger" in both fields: the k best entries of a row are the k largest under
// (key, ck), ties on both fields going to the earlier position.  The key is only ever COMPARED:
//   * it sends both zeros to ONE key (-0.0 == +0.0: the column decides between them);
//   * it sends EVERY NaN, whatever its sign bit, to key 0, the lowest: below -inf's, whose key is the smallest of a number
//     (~0xff800000 = 0x007fffff in float).  The plain sign flip alone would put a NaN without a sign bit above +inf and
//     a NaN with one below -inf;
//   * the values written out are the ORIGINAL bits, read again from the input, never values rebuilt from keys: a key
//     cannot give back the sign of a zero or the payload of a NaN.
//
// The work.  k_topk_lens writes min(len, k) per row, counts the rows that are cut (len > k) and lists them per class; the
// kit's scan turns the lengths into the output row pointer and gives nnzN.  Without a cut row the result is three
// device-to-device copies.  Otherwise k_topk_copy copies the uncut rows bit for bit, G lanes per row like k_attractors,
// and the cut rows are SELECTED, not sorted: the threshold entry (the k-th best) is found digit by digit from the most
// significant end of (key, ck); "need" is how many entries are still to be taken among the candidates, the entries that
// agree with the threshold on every digit fixed so far.  At the end an entry is kept iff it is above the threshold prefix,
// or is a candidate and among the first `need` candidates in storage order.  The compaction is stable.
//   wave   (len <= 1024)      one wave per row, the keys in registers: 1, 2, 4, 8 or 16 per lane, a kernel and a list of
//                             rows for each (a row of up to 64 entries is one register).  One BIT per step, a ballot and
//                             a popcount per register: (key >> b) == (prefix >> b | 1) is "candidate with bit b set".  A
//                             padding register holds key 0, which has no bit set and is never counted.  The column bits
//                             are walked only if more entries equal the threshold value than are needed, among those
//                             entries only; position ties and the compaction go by ballot prefix.  No LDS at all.
//   block  (len <= blockCap)  256 threads per row, keys and columns staged once in LDS (48 KiB for either type: three
//                             blocks to a CU's 160 KiB); one BYTE per step, a 256-bin histogram by integer LDS atomics,
//                             the digit picked by a block scan from the top bin down.  The loop ends as soon as the
//                             candidates are exactly the entries needed.  Every wave owns a contiguous quarter of the
//                             row: one counting walk, one writing walk.
//   stream (longer rows)      the block kernel without the staging: every pass reads the row again from global memory.
// SPGEMM_TOPK_NORMALISE divides the kept values of the CUT rows by their sum: the sum is formed in double for both types,
// per lane in storage order, then across the wave by a butterfly, then (block) over the four waves in order: a fixed tree,
// the same bits on every call.  The divisor is that sum rounded to V, the division one IEEE division in V.  Values that
// are not finite and non-negative with a positive sum give whatever the division gives.  No floating-point atomic.
// Uses csr_common_device.hpp (Scratch, enter, check_csr_args, validate_csr, scan_inplace) and clusters::lanes_per_row.
#pragma once

namespace topk {

using namespace csrdev;

constexpr int TK_THREADS = 256, TK_WAVES = TK_THREADS / WAVE;
constexpr int TK_ITEMS = 16, TK_WAVE_CAP = WAVE * TK_ITEMS;        // most keys per lane and the longest row of the wave path
constexpr int TK_WAVE_CLASSES = 5;                                 // rows of up to 64, 128, 256, 512, 1024 entries: 1, 2, 4, 8, 16 keys per lane
constexpr int TK_CLASSES = TK_WAVE_CLASSES + 2;                    // ... the block path, the stream path
constexpr unsigned TK_CK_MAX = 0x7fffffffu;                        // ck = TK_CK_MAX - column: 31 bits

template <class V> struct Traits;
template <> struct Traits<float> { using K = unsigned; static constexpr int BLOCK_CAP = 6144; };            // 8 B an entry
template <> struct Traits<double> { using K = unsigned long long; static constexpr int BLOCK_CAP = 4096; }; // 12 B an entry

static inline int block_cap(bool isDouble) { return isDouble ? Traits<double>::BLOCK_CAP : Traits<float>::BLOCK_CAP; }

template <class V>
__device__ __forceinline__ typename Traits<V>::K value_bits(V v) {
  typename Traits<V>::K b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return b;
}

// larger value <=> larger key; both zeros one key; every NaN key 0, below -inf's (see the head of this file)
template <class V>
__device__ __forceinline__ typename Traits<V>::K ordered_key(V v) {
  using K = typename Traits<V>::K;
  constexpr K SIGN = (K)1 << (sizeof(K) * 8 - 1);
  const K b = value_bits(v);
  if (v != v) return 0;                                            // a NaN of either sign bit
  if ((K)(b << 1) == 0) return SIGN;                               // -0.0 and +0.0
  return (b & SIGN) ? ~b : (b | SIGN);
}

__global__ __launch_bounds__(TK_THREADS) void k_topk_lens(int m, const int* __restrict__ IA, int k, int waveCap, int blockCap,
                                                          int* __restrict__ outLen, int* __restrict__ cnt, int* __restrict__ lists) {
  const long long r = (long long)blockIdx.x * TK_THREADS + threadIdx.x;
  int cls = -1;
  if (r < m) {
    const int len = IA[r + 1] - IA[r];
    outLen[r] = min(len, k);
    if (len > k) {
      if (len <= waveCap) { cls = 0; while ((WAVE << cls) < len) ++cls; }
      else cls = len <= blockCap ? TK_WAVE_CLASSES : TK_WAVE_CLASSES + 1;
    }
  }
#pragma unroll
  for (int c = 0; c < TK_CLASSES; ++c) {                                    // every lane of the wave takes part in the ballots
    const unsigned long long mask = ballot64(cls == c);
    if (mask == 0ull) continue;
    int base = 0;
    if (lane_id() == (int)__builtin_ctzll(mask)) base = atomicAdd(cnt + c, __popcll(mask));
    base = __shfl(base, (int)__builtin_ctzll(mask));
    if (cls == c) lists[(size_t)c * m + base + mask_rank(mask)] = (int)r;
  }
}

// the rows that are not cut, bit for bit (values travel as integers): G lanes per row
template <class V, int G>
__global__ __launch_bounds__(TK_THREADS) void k_topk_copy(int m, int k, const int* __restrict__ IA, const int* __restrict__ JA,
                                                          const V* __restrict__ A, const int* __restrict__ IN,
                                                          int* __restrict__ JN, V* __restrict__ AN) {
  using K = typename Traits<V>::K;
  const int sub = threadIdx.x & (G - 1);
  const long long row = ((long long)blockIdx.x * TK_THREADS + threadIdx.x) / G;
  if (row >= m) return;
  const long long a = IA[row];
  const int len = IA[row + 1] - (int)a;
  if (len > k) return;
  const long long o = IN[row];
  const K* __restrict__ src = reinterpret_cast<const K*>(A);
  K* __restrict__ dst = reinterpret_cast<K*>(AN);
  for (int i = sub; i < len; i += G) {
    JN[o + i] = JA[a + i];
    dst[o + i] = src[a + i];
  }
}

// one wave per cut row of up to 64 * ITEMS entries; register i of lane l holds entry i * 64 + l (storage order = (i, l)).
// The registers are filled and counted in straight-line code: a load past the end reads the row's first entry instead.
template <class V, int ITEMS>
__global__ __launch_bounds__(TK_THREADS) void k_topk_wave(int nrows, const int* __restrict__ rows, int k, int norm,
                                                          const int* __restrict__ IA, const int* __restrict__ JA,
                                                          const V* __restrict__ A, const int* __restrict__ IN,
                                                          int* __restrict__ JN, V* AN) {
  using K = typename Traits<V>::K;
  constexpr int KB = sizeof(K) * 8;
  const int lane = lane_id();
  const long long w = ((long long)blockIdx.x * TK_THREADS + threadIdx.x) >> 6;
  if (w >= nrows) return;                                          // the whole wave; the kernel has no barrier
  const int r = rows[w];
  const long long a = IA[r];
  const int len = IA[r + 1] - (int)a;                              // k < len <= 64 * ITEMS
  const int nIt = (len + WAVE - 1) >> 6;
  K key[ITEMS];
  unsigned ck[ITEMS];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int idx = i * WAVE + lane;
    const bool in = idx < len;
    const long long at = a + (in ? idx : 0);
    const K kv = ordered_key<V>(A[at]);
    const unsigned kc = TK_CK_MAX - (unsigned)JA[at];
    key[i] = in ? kv : (K)0;                                       // padding: no bit set, never counted below
    ck[i] = in ? kc : 0u;
  }
  // the k-th largest key, bit by bit: `need` entries are still to be taken among the entries that agree with tv so far
  K tv = 0;
  int need = k;
#pragma nounroll
  for (int b = KB - 1; b >= 0; --b) {
    const K want = (K)(tv >> b) | (K)1;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) cnt += __popcll(ballot64((K)(key[i] >> b) == want));
    if (cnt >= need) tv |= (K)1 << b; else need -= cnt;
  }
  // the entries equal to the threshold value (key 0 is the NaNs' as well as the padding's: from here on the length matters)
  int nc = 0;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const bool c = key[i] == tv && i * WAVE + lane < len;
    nc += __popcll(ballot64(c));
    ck[i] = c ? ck[i] : 0u;                                        // the others leave the column walk: no bit set, never counted
  }
  const bool tieAll = nc == need;                                  // the usual case: no choice to make among them
  unsigned tc = 0;
  if (!tieAll) {
#pragma nounroll
    for (int b = 30; b >= 0; --b) {
      const unsigned want = (tc >> b) | 1u;
      int cnt = 0;
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) cnt += __popcll(ballot64((ck[i] >> b) == want));
      if (cnt >= need) tc |= 1u << b; else need -= cnt;
    }
  }
  // Who stays: above the threshold in (key, ck), or one of the first `need` entries equal to it in storage order.  The
  // registers are done with: these two walks read the row again (it is in the cache), in loops that stay rolled.
  const K* __restrict__ src = reinterpret_cast<const K*>(A);
  K* dst = reinterpret_cast<K*>(AN);
  unsigned keepM = 0;
  int tieSeen = 0;
  double sum = 0.0;
#pragma nounroll
  for (int i = 0; i < nIt; ++i) {
    const int idx = i * WAVE + lane;
    const bool valid = idx < len;
    const V v = valid ? A[a + idx] : (V)0;
    const K kv = ordered_key<V>(v);
    const unsigned kc = valid ? TK_CK_MAX - (unsigned)JA[a + idx] : 0u;
    const bool cand = valid && kv == tv;
    const bool tie = cand && (tieAll || kc == tc);
    const unsigned long long tb = ballot64(tie);
    const bool keep = valid && (kv > tv || (cand && !tieAll && kc > tc) || (tie && tieSeen + mask_rank(tb) < need));
    tieSeen += __popcll(tb);
    keepM |= keep ? 1u << i : 0u;
    if (norm && keep) sum += (double)v;
  }
  V den = (V)1;
  if (norm) {                                                      // the same tree on every call; every lane ends with the same bits
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    den = (V)sum;
  }
  const long long o = IN[r];
  int running = 0;
#pragma nounroll
  for (int i = 0; i < nIt; ++i) {
    const bool keep = (keepM >> i) & 1u;
    const unsigned long long kb = ballot64(keep);
    const int at = running + mask_rank(kb);
    if (keep && at < k) {                                          // (at < k always: the row's k output slots bound every store)
      const long long from = a + i * WAVE + lane, to = o + at;
      JN[to] = JA[from];
      if (norm) AN[to] = A[from] / den; else dst[to] = src[from];
    }
    running += __popcll(kb);
  }
}

// how the top nd digits of (kv, kc) compare with those of the threshold (tv, tc): -1, 0, 1.  Digits are bytes, the value
// key's first; nd == 0 compares nothing.
template <class K>
__device__ __forceinline__ int prefix_cmp(K kv, unsigned kc, K tv, unsigned tc, int nd) {
  constexpr int VD = sizeof(K), KB = VD * 8;
  if (nd == 0) return 0;
  if (nd < VD) {
    const int sh = KB - 8 * nd;
    const K x = kv >> sh, y = tv >> sh;
    return x > y ? 1 : x < y ? -1 : 0;
  }
  if (kv != tv) return kv > tv ? 1 : -1;
  if (nd == VD) return 0;
  const int sh = 32 - 8 * (nd - VD);
  const unsigned x = kc >> sh, y = tc >> sh;
  return x > y ? 1 : x < y ? -1 : 0;
}

// one block per cut row; STAGED: the row's keys and columns are in LDS (len <= BLOCK_CAP), else every pass reads the row
template <class V, bool STAGED>
__global__ __launch_bounds__(TK_THREADS) void k_topk_block(const int* __restrict__ rows, int k, int norm,
                                                           const int* __restrict__ IA, const int* __restrict__ JA,
                                                           const V* __restrict__ A, const int* __restrict__ IN,
                                                           int* __restrict__ JN, V* AN) {
  using K = typename Traits<V>::K;
  constexpr int VD = sizeof(K), KB = VD * 8, ND = VD + 4, CAP = STAGED ? Traits<V>::BLOCK_CAP : 1;
  __shared__ K skey[CAP];
  __shared__ int scol[CAP];
  __shared__ int hist[256];
  __shared__ int wtot[TK_WAVES], wAbove[TK_WAVES], wCand[TK_WAVES], sel[3];
  __shared__ double wsum[TK_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = rows[blockIdx.x];
  const long long a = IA[r];
  const long long len = IA[r + 1] - (int)a;                        // k < len (<= BLOCK_CAP if STAGED)
  auto key_of = [&](long long i) -> K { if constexpr (STAGED) return skey[i]; else return ordered_key<V>(A[a + i]); };
  auto ck_of = [&](long long i) -> unsigned { if constexpr (STAGED) return TK_CK_MAX - (unsigned)scol[i]; else return TK_CK_MAX - (unsigned)JA[a + i]; };
  if constexpr (STAGED) {
    for (long long i = tid; i < len; i += TK_THREADS) { skey[i] = ordered_key<V>(A[a + i]); scol[i] = JA[a + i]; }
  }
  K tv = 0;
  unsigned tc = 0;
  int need = k, nd = 0;
  while (nd < ND) {                                                // uniform: every thread sees the same sel[]
    hist[tid] = 0;
    __syncthreads();                                               // (the first one also ends the staging)
    const bool inCols = nd >= VD;
    for (long long i = tid; i < len; i += TK_THREADS) {
      const K kv = key_of(i);
      const unsigned kc = inCols ? ck_of(i) : 0u;
      if (prefix_cmp<K>(kv, kc, tv, tc, nd) != 0) continue;
      const int dg = inCols ? (int)((kc >> (24 - 8 * (nd - VD))) & 255u) : (int)((kv >> (KB - 8 * (nd + 1))) & (K)255);
      atomicAdd(&hist[dg], 1);
    }
    __syncthreads();
    // thread t holds bin 255 - t: an inclusive scan in thread order counts from the top bin down
    const int mine = hist[255 - tid];
    int incl = mine;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == WAVE - 1) wtot[w] = incl;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TK_WAVES; ++q) if (q < w) incl += wtot[q];
    if (incl >= need && incl - mine < need) {                      // exactly one thread: the candidates are at least `need`
      sel[0] = 255 - tid;
      sel[1] = need - (incl - mine);
      sel[2] = mine;
    }
    __syncthreads();
    const int dg = sel[0], nc = sel[2];
    need = sel[1];
    if (inCols) tc |= (unsigned)dg << (24 - 8 * (nd - VD)); else tv |= (K)dg << (KB - 8 * (nd + 1));
    ++nd;
    if (nc == need) break;                                         // every candidate is needed: no digit below decides anything
  }
  // wave w owns entries [s0, s1): counts first, so that every wave knows where its kept entries start
  const bool inCols = nd > VD;
  const long long seg = (len + TK_THREADS - 1) / TK_THREADS * WAVE;
  const long long s0 = min(len, w * seg), s1 = min(len, s0 + seg);
  int above = 0, cands = 0;
  for (long long c = s0; c < s1; c += WAVE) {
    const long long i = c + lane;
    int cmp = -1;
    if (i < s1) cmp = prefix_cmp<K>(key_of(i), inCols ? ck_of(i) : 0u, tv, tc, nd);
    above += __popcll(ballot64(cmp > 0));
    cands += __popcll(ballot64(cmp == 0));
  }
  if (lane == 0) { wAbove[w] = above; wCand[w] = cands; }
  __syncthreads();
  int candSeen = 0, running = 0;
#pragma unroll
  for (int q = 0; q < TK_WAVES; ++q) if (q < w) { candSeen += wCand[q]; running += wAbove[q]; }
  running += min(candSeen, need);                                  // the candidates kept in front of this wave
  const long long o = IN[r];
  const K* __restrict__ src = reinterpret_cast<const K*>(A);
  K* dst = reinterpret_cast<K*>(AN);                               // (not __restrict__: the division below reads these stores back)
  double sum = 0.0;
  for (long long c = s0; c < s1; c += WAVE) {
    const long long i = c + lane;
    int cmp = -1;
    if (i < s1) cmp = prefix_cmp<K>(key_of(i), inCols ? ck_of(i) : 0u, tv, tc, nd);
    const unsigned long long cb = ballot64(cmp == 0);
    const bool keep = cmp > 0 || (cmp == 0 && candSeen + mask_rank(cb) < need);
    const unsigned long long kb = ballot64(keep);
    const int at = running + mask_rank(kb);
    if (keep && at < k) {                                          // (at < k always: the row's k output slots bound every store)
      const long long to = o + at;
      JN[to] = JA[a + i];
      dst[to] = src[a + i];                                        // the original bits; a cut row is divided below
      if (norm) sum += (double)A[a + i];
    }
    candSeen += __popcll(cb);
    running += __popcll(kb);
  }
  if (!norm) return;                                               // uniform
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
  if (lane == 0) wsum[w] = sum;
  __threadfence_block();                                           // the row's k values, written by all four waves, are read back below
  __syncthreads();
  double total = wsum[0];
#pragma unroll
  for (int q = 1; q < TK_WAVES; ++q) total += wsum[q];
  const V den = (V)total;
  for (int j = tid; j < k; j += TK_THREADS) AN[o + j] = AN[o + j] / den;
}

template <class V>
static void launch_copy(hipStream_t s, int G, int m, int k, const int* IA, const int* JA, const V* A, const int* IN, int* JN, V* AN) {
  const dim3 grid = clusters::row_grid(m, G), block(TK_THREADS);
  if (G == 4) hipLaunchKernelGGL((k_topk_copy<V, 4>), grid, block, 0, s, m, k, IA, JA, A, IN, JN, AN);
  else if (G == 16) hipLaunchKernelGGL((k_topk_copy<V, 16>), grid, block, 0, s, m, k, IA, JA, A, IN, JN, AN);
  else hipLaunchKernelGGL((k_topk_copy<V, 64>), grid, block, 0, s, m, k, IA, JA, A, IN, JN, AN);
}

template <class V>
static int row_topk(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, int k, int flags,
                    int** dIN, int** dJN, V** dAN, int* nnzN, int* rowsCut) {
  if (dIN) *dIN = nullptr;
  if (dJN) *dJN = nullptr;
  if (dAN) *dAN = nullptr;
  if (nnzN) *nnzN = 0;
  if (rowsCut) *rowsCut = 0;
  if (!dIN || !dJN || !dAN || !nnzN) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  if (k < 1) return fail(SPGEMM_ERR_ARG, "k=%d: a row keeps at least one entry", k);
  if (flags & ~SPGEMM_TOPK_NORMALISE) return fail(SPGEMM_ERR_ARG, "unknown flag bits 0x%x", flags & ~SPGEMM_TOPK_NORMALISE);
  CHK(check_csr_args(m, n, nnz, dIA, dJA, dA));
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *IN = nullptr, *JN = nullptr, *ctl = nullptr, *lists = nullptr;
  V* AN = nullptr;
  unsigned long long* tile = nullptr;
  CSR_ALLOC(&IN, sizeof(int) * ((size_t)m + 1), true);
  if (m == 0) {
    CSR_ALLOC(&JN, sizeof(int), true);
    CSR_ALLOC(&AN, sizeof(V), true);
    CSR_HIP(hipMemsetAsync(IN, 0, sizeof(int), s));
    CSR_HIP(hipStreamSynchronize(s));
    *dIN = IN; *dJN = JN; *dAN = AN;
    return sc.done(SPGEMM_OK);
  }
  int hbad = 0;
  if (int rc = validate_csr(sc, s, m, n, nnz, dIA, dJA, &hbad)) return sc.done(rc);
  if (hbad) return sc.done(clusters::bad_csr(hbad, n, nnz));
  CSR_ALLOC(&ctl, sizeof(int) * TK_CLASSES);
  CSR_ALLOC(&lists, sizeof(int) * TK_CLASSES * (size_t)m);
  CSR_ALLOC(&tile, scan_scratch_bytes((long long)m + 1));
  CSR_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * TK_CLASSES, s));
  const int blockCap = Traits<V>::BLOCK_CAP;
  hipLaunchKernelGGL(k_topk_lens, grid256(m), dim3(TK_THREADS), 0, s, m, dIA, k, TK_WAVE_CAP, blockCap, IN, ctl, lists);
  CSR_HIP(hipGetLastError());
  scan_inplace(s, IN, m, tile);
  unsigned long long total = 0;
  int cut[TK_CLASSES] = {0};
  CSR_HIP(hipMemcpyAsync(&total, tile, sizeof(total), hipMemcpyDeviceToHost, s));
  CSR_HIP(hipMemcpyAsync(cut, ctl, sizeof(cut), hipMemcpyDeviceToHost, s));
  CSR_HIP(hipStreamSynchronize(s));
  const int kept = (int)total;                                     // <= nnz
  long long ncut = 0, nwave = 0;
  for (int c = 0; c < TK_CLASSES; ++c) ncut += cut[c];
  for (int c = 0; c < TK_WAVE_CLASSES; ++c) nwave += cut[c];
  CSR_ALLOC(&JN, sizeof(int) * (size_t)std::max(kept, 1), true);
  CSR_ALLOC(&AN, sizeof(V) * (size_t)std::max(kept, 1), true);
  if (ncut == 0) {                                                 // nothing to select: the input, bit for bit
    CSR_HIP(hipMemcpyAsync(IN, dIA, sizeof(int) * ((size_t)m + 1), hipMemcpyDeviceToDevice, s));
    if (nnz > 0) {
      CSR_HIP(hipMemcpyAsync(JN, dJA, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
      CSR_HIP(hipMemcpyAsync(AN, dA, sizeof(V) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
    }
  } else {
    const int norm = (flags & SPGEMM_TOPK_NORMALISE) ? 1 : 0;
    if (ncut < m) launch_copy<V>(s, clusters::lanes_per_row(m, kept), m, k, dIA, dJA, dA, IN, JN, AN);
    auto wave = [&](auto items, int c) {                           // class c: rows of up to 64 << c entries
      constexpr int ITEMS = decltype(items)::value;
      if (cut[c] > 0)
        hipLaunchKernelGGL((k_topk_wave<V, ITEMS>), dim3((unsigned)cdiv(cut[c], TK_WAVES)), dim3(TK_THREADS), 0, s, cut[c],
                           lists + c * (size_t)m, k, norm, dIA, dJA, dA, IN, JN, AN);
    };
    wave(std::integral_constant<int, 1>{}, 0);
    wave(std::integral_constant<int, 2>{}, 1);
    wave(std::integral_constant<int, 4>{}, 2);
    wave(std::integral_constant<int, 8>{}, 3);
    wave(std::integral_constant<int, 16>{}, 4);
    const int* blockRows = lists + TK_WAVE_CLASSES * (size_t)m;
    if (cut[TK_WAVE_CLASSES] > 0)
      hipLaunchKernelGGL((k_topk_block<V, true>), dim3((unsigned)cut[TK_WAVE_CLASSES]), dim3(TK_THREADS), 0, s, blockRows, k, norm,
                         dIA, dJA, dA, IN, JN, AN);
    if (cut[TK_WAVE_CLASSES + 1] > 0)
      hipLaunchKernelGGL((k_topk_block<V, false>), dim3((unsigned)cut[TK_WAVE_CLASSES + 1]), dim3(TK_THREADS), 0, s, blockRows + m, k,
                         norm, dIA, dJA, dA, IN, JN, AN);
    CSR_HIP(hipGetLastError());
  }
  CSR_HIP(hipStreamSynchronize(s));
  h->topkRows[0] += m - ncut;
  h->topkRows[1] += nwave;
  h->topkRows[2] += cut[TK_WAVE_CLASSES];
  h->topkRows[3] += cut[TK_WAVE_CLASSES + 1];
  *dIN = IN; *dJN = JN; *dAN = AN; *nnzN = kept;
  if (rowsCut) *rowsCut = (int)ncut;
  return sc.done(SPGEMM_OK);
}

static int step(spgemm_handle* h, const int* gI, const int* gJ, const float* gA, int gnnz, const int* tI, const int* tJ,
                const float* tA, int tnnz, int m, int** xI, int** xJ, float** xA, int* xnnz) {
  return hip_rmcl_expand_prune(h, gI, gJ, gA, gnnz, tI, tJ, tA, tnnz, m, m, m, xI, xJ, xA, xnnz);
}
static int step(spgemm_handle* h, const int* gI, const int* gJ, const double* gA, int gnnz, const int* tI, const int* tJ,
                const double* tA, int tnnz, int m, int** xI, int** xJ, double** xA, int* xnnz) {
  return hip_rmcl_expand_prune_f64(h, gI, gJ, gA, gnnz, tI, tJ, tA, tnnz, m, m, m, xI, xJ, xA, xnnz);
}

// a CSR of the pool that goes back to it unless it is handed out
template <class V>
struct Owned {
  int *I = nullptr, *J = nullptr;
  V* X = nullptr;
  int nnz = 0;
  void drop() { for (void* p : {(void*)I, (void*)J, (void*)X}) if (p) spgemm_hip_free(p); I = J = nullptr; X = nullptr; nnz = 0; }
  ~Owned() { drop(); }
};

// The loop with a row cap, composed from the packed public step: X = expand_prune(Mgt, Mt), Mt = row_topk(X, k, NORMALISE).
// Both calls return with their device work done, so a matrix is idle when it is released.
template <class V>
static int rmcl_iter_topk(spgemm_handle* h, int maxIter, int k, int rows, int cols, const int* gI, const int* gJ, const V* gA,
                          int gnnz, const int* tI, const int* tJ, const V* tA, int tnnz, int** oI, int** oJ, V** oA, int* onnz,
                          long long* iterNnz, long long* iterCut) {
  CHK(rmcl_loop_args(maxIter, rows, cols, gI, gJ, gA, gnnz, tI, tJ, tA, tnnz, oI, oJ, oA, onnz));
  if (k < 1) return fail(SPGEMM_ERR_ARG, "k=%d: a row keeps at least one entry", k);
  for (int i = 0; i < maxIter; ++i) {
    if (iterNnz) iterNnz[i] = 0;
    if (iterCut) iterCut[i] = 0;
  }
  if (!h) CHK(default_handle(&h));
  Owned<V> cur;
  if (maxIter == 0) {                                              // no iteration, nothing to cut: a copy of Mt
    hipStream_t s;
    CHK(enter(h, &s));
    DevCSRT<V> copy;
    CHK(rmcl_copy_of_mt(s, rows, tI, tJ, tA, tnnz, &copy));
    copy.give(oI, oJ, oA, onnz);
    return SPGEMM_OK;
  }
  for (int it = 0; it < maxIter; ++it) {
    Owned<V> x, next;
    CHK(step(h, gI, gJ, gA, gnnz, it ? cur.I : tI, it ? cur.J : tJ, it ? cur.X : tA, it ? cur.nnz : tnnz, rows, &x.I, &x.J,
             &x.X, &x.nnz));
    int cut = 0;
    CHK(row_topk<V>(h, rows, cols, x.nnz, x.I, x.J, x.X, k, SPGEMM_TOPK_NORMALISE, &next.I, &next.J, &next.X, &next.nnz, &cut));
    if (iterNnz) iterNnz[it] = next.nnz;
    if (iterCut) iterCut[it] = cut;
    cur.drop();
    cur = next;
    next.I = next.J = nullptr; next.X = nullptr;                   // moved into cur
  }
  *oI = cur.I; *oJ = cur.J; *oA = cur.X; *onnz = cur.nnz;
  cur.I = cur.J = nullptr; cur.X = nullptr;
  return SPGEMM_OK;
}

}  // namespace topk

extern "C" int hip_csr_row_topk(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA, int k,
                                int flags, int** dIN, int** dJN, float** dAN, int* nnzN, int* rowsCut) {
  return topk::row_topk<float>(h, m, n, nnz, dIA, dJA, dA, k, flags, dIN, dJN, dAN, nnzN, rowsCut);
}
extern "C" int hip_csr_row_topk_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                                    int k, int flags, int** dIN, int** dJN, double** dAN, int* nnzN, int* rowsCut) {
  return topk::row_topk<double>(h, m, n, nnz, dIA, dJA, dA, k, flags, dIN, dJN, dAN, nnzN, rowsCut);
}

extern "C" int hip_csr_row_topk_limits(int isDouble, int* waveCap, int* blockCap) {
  if (!waveCap || !blockCap) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *waveCap = topk::TK_WAVE_CAP;
  *blockCap = topk::block_cap(isDouble != 0);
  return SPGEMM_OK;
}

extern "C" int spgemm_hip_debug_topk_paths(spgemm_handle* h, long long* copied, long long* wave, long long* block, long long* stream) {
  if (!h) CHK(default_handle(&h));
  if (copied) *copied = h->topkRows[0];
  if (wave) *wave = h->topkRows[1];
  if (block) *block = h->topkRows[2];
  if (stream) *stream = h->topkRows[3];
  return SPGEMM_OK;
}

extern "C" int hip_gpuRmclIter_device_topk(spgemm_handle* h, int maxIter, int k, int rows, int cols, const int* dgI, const int* dgJ,
                                           const float* dgA, int gnnz, const int* dtI, const int* dtJ, const float* dtA, int tnnz,
                                           int** oI, int** oJ, float** oA, int* onnz, long long* iterNnz, long long* iterCut) {
  return topk::rmcl_iter_topk<float>(h, maxIter, k, rows, cols, dgI, dgJ, dgA, gnnz, dtI, dtJ, dtA, tnnz, oI, oJ, oA, onnz,
                                     iterNnz, iterCut);
}
extern "C" int hip_gpuRmclIter_device_topk_f64(spgemm_handle* h, int maxIter, int k, int rows, int cols, const int* dgI,
                                               const int* dgJ, const double* dgA, int gnnz, const int* dtI, const int* dtJ,
                                               const double* dtA, int tnnz, int** oI, int** oJ, double** oA, int* onnz,
                                               long long* iterNnz, long long* iterCut) {
  return topk::rmcl_iter_topk<double>(h, maxIter, k, rows, cols, dgI, dgJ, dgA, gnnz, dtI, dtJ, dtA, tnnz, oI, oJ, oA, onnz,
                                      iterNnz, iterCut);
}
