// Comparing two device CSRs on the device: one diff report, CSR::differs and CSR::differsStats.
//
// Replaces, on device arrays,
//   CSR::differs                              nlibs/CSR.cc:210-240   (squared Frobenius norm of A - B, a two-pointer merge per row)
//   CSR::isEqual / isRelativeEqual            nlibs/CSR.h:195-245, 284-320 (a dense row scatter per row; here: the fields they need)
//   CSR::differsStats                         nlibs/CSR.cc:381-415   (how the row lengths moved)
//
// hip_csr_diff is one pass over the nnzA + nnzB entries of two m x n matrices whose rows are strictly ascending by column.
// The entries are the work items, A's first and then B's, dealt 1024 to a block whatever rows they belong to -- a
// 20 000-entry row next to empty ones is spread over 20 blocks (40 with its partner row) like any other 20 000 entries.
// An item finds its row by a search in its own rowPtr bounded by the rows of the first and the last item its block
// holds of that matrix (row_of_entry, as the copy kernels do), then its partner by a binary search for its
// column in the same row of the other matrix.  A common column is accounted by A's item; a B item reports only when it
// has no partner.  The same pass compares every item's column with its predecessor's in the row (the "not sorted" flag).
// Reductions: counts and first rows by integer atomics, maxima as the bit patterns of non-negative doubles (ordered like
// integers, so order-independent), sum_sq in double in a fixed order: lane sums its items in tile order, a fixed shuffle
// tree per wave, the four waves in order, one partial per block, and a single-block kernel over the partials.  No
// floating-point atomic anywhere: two calls on the same input return the same bits.
// Both rowPtr arrays are checked (k_check_rowptr) and the flag is read before anything is queued that forms an
// address from a rowPtr value.  Columns are only compared, never used as addresses.
// Uses csr_common_device.hpp (the rowPtr check and its one read-back, row search, lower bound, Scratch).
#pragma once

namespace compare {

using namespace csrdev;

constexpr int CMP_THREADS = 256, CMP_ITEMS = 4, CMP_TILE = CMP_THREADS * CMP_ITEMS;
constexpr int NO_ROW = 0x7fffffff;
constexpr int MAX_PERCENTS = 64;

// accumulators of one hip_csr_diff call (device); the maxima hold the bits of non-negative doubles
struct Acc {
  unsigned long long only_a, only_b, beyond;
  unsigned long long max_abs_err, max_rel_err, max_only_a, max_only_b;
  int rows_len_differ, first_len_row, first_only_row, first_beyond_row;
  int unsorted, pad;
  double sum_sq;
};

__device__ __forceinline__ unsigned long long dbits(double x) { return (unsigned long long)__double_as_longlong(x); }

// rows whose lengths differ and the lowest of them: one lane per row, one pair of atomics per wave that saw one
__global__ __launch_bounds__(256) void k_len_differ(int m, const int* __restrict__ IA, const int* __restrict__ IB,
                                                    Acc* __restrict__ acc) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool d = r < m && (IA[r + 1] - IA[r]) != (IB[r + 1] - IB[r]);
  const unsigned long long mask = __ballot(d);
  if ((threadIdx.x & 63) == 0 && mask) {
    atomicAdd(&acc->rows_len_differ, __popcll(mask));
    atomicMin(&acc->first_len_row, r + __ffsll((long long)mask) - 1);
  }
}

// what one lane, then one wave, then one block has seen
struct Seen {
  unsigned only_a, only_b, beyond;
  int first_only, first_beyond, unsorted;
  double max_abs, max_rel, max_oa, max_ob, sum;
};

__device__ __forceinline__ void wave_fold(Seen& s) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    s.only_a += __shfl_down(s.only_a, d);
    s.only_b += __shfl_down(s.only_b, d);
    s.beyond += __shfl_down(s.beyond, d);
    s.first_only = min(s.first_only, __shfl_down(s.first_only, d));
    s.first_beyond = min(s.first_beyond, __shfl_down(s.first_beyond, d));
    s.unsorted |= __shfl_down(s.unsorted, d);
    s.max_abs = fmax(s.max_abs, __shfl_down(s.max_abs, d));
    s.max_rel = fmax(s.max_rel, __shfl_down(s.max_rel, d));
    s.max_oa = fmax(s.max_oa, __shfl_down(s.max_oa, d));
    s.max_ob = fmax(s.max_ob, __shfl_down(s.max_ob, d));
    s.sum += __shfl_down(s.sum, d);                         // fixed tree: lane 0 ends with the same bits every time
  }
}

template <class V>
__global__ __launch_bounds__(CMP_THREADS) void k_diff_walk(int m, int nnzA, int nnzB, const int* __restrict__ IA,
                                                           const int* __restrict__ JA, const V* __restrict__ A,
                                                           const int* __restrict__ IB, const int* __restrict__ JB,
                                                           const V* __restrict__ B, double rel_tol, double abs_tol,
                                                           Acc* __restrict__ acc, double* __restrict__ partial) {
#pragma clang fp contract(off)                              // every term is one rounding per operation, as the host restates it
  __shared__ int rows[4];                                   // rows of the tile's first / last A item, first / last B item
  __shared__ Seen waves[CMP_THREADS / 64];
  const long long total = (long long)nnzA + nnzB;
  const long long base = (long long)blockIdx.x * CMP_TILE;
  const long long end = base + CMP_TILE < total ? base + CMP_TILE : total;
  if (threadIdx.x == 0 && base < nnzA) {
    const long long last = (end < nnzA ? end : (long long)nnzA) - 1;
    rows[0] = row_of_entry(IA, 0, m - 1, (int)base);
    rows[1] = row_of_entry(IA, rows[0], m - 1, (int)last);
  }
  if (threadIdx.x == 64 && end > nnzA) {
    const long long first = (base > nnzA ? base : (long long)nnzA) - nnzA;
    rows[2] = row_of_entry(IB, 0, m - 1, (int)first);
    rows[3] = row_of_entry(IB, rows[2], m - 1, (int)(end - 1 - nnzA));
  }
  __syncthreads();
  Seen s = {0u, 0u, 0u, NO_ROW, NO_ROW, 0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < CMP_ITEMS; ++k) {
    const long long g = base + k * CMP_THREADS + threadIdx.x;
    if (g >= total) break;
    const bool isA = g < nnzA;
    const int o = (int)(isA ? g : g - nnzA);
    const int* __restrict__ IX = isA ? IA : IB;
    const int* __restrict__ JX = isA ? JA : JB;
    const int* __restrict__ IY = isA ? IB : IA;
    const int* __restrict__ JY = isA ? JB : JA;
    const int r = row_of_entry(IX, rows[isA ? 0 : 2], rows[isA ? 1 : 3], o);
    const int c = JX[o];
    if (o > IX[r] && JX[o - 1] >= c) s.unsorted = 1;
    const int ye = IY[r + 1];
    const int lo = first_at_least(JY, IY[r], ye, c);
    const bool found = lo < ye && JY[lo] == c;
    if (isA) {
      const double a = (double)A[o];
      if (found) {
        const double b = (double)B[lo], d = fabs(a - b), ab = fabs(b);
        if (!(d <= abs_tol + rel_tol * ab)) { ++s.beyond; s.first_beyond = min(s.first_beyond, r); }
        if (d > s.max_abs) s.max_abs = d;                   // a NaN compares false: skipped
        if (ab != 0.0) { const double q = d / ab; if (q > s.max_rel) s.max_rel = q; }
        s.sum += (a - b) * (a - b);
      } else {
        ++s.only_a;
        s.first_only = min(s.first_only, r);
        if (fabs(a) > s.max_oa) s.max_oa = fabs(a);
        s.sum += a * a;
      }
    } else if (!found) {
      const double b = (double)B[o];
      ++s.only_b;
      s.first_only = min(s.first_only, r);
      if (fabs(b) > s.max_ob) s.max_ob = fabs(b);
      s.sum += b * b;
    }
  }
  wave_fold(s);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < CMP_THREADS / 64; ++w) {              // waves in order
    const Seen& t = waves[w];
    s.only_a += t.only_a; s.only_b += t.only_b; s.beyond += t.beyond;
    s.first_only = min(s.first_only, t.first_only);
    s.first_beyond = min(s.first_beyond, t.first_beyond);
    s.unsorted |= t.unsorted;
    s.max_abs = fmax(s.max_abs, t.max_abs); s.max_rel = fmax(s.max_rel, t.max_rel);
    s.max_oa = fmax(s.max_oa, t.max_oa); s.max_ob = fmax(s.max_ob, t.max_ob);
    s.sum += t.sum;
  }
  partial[blockIdx.x] = s.sum;
  if (s.only_a) atomicAdd(&acc->only_a, (unsigned long long)s.only_a);
  if (s.only_b) atomicAdd(&acc->only_b, (unsigned long long)s.only_b);
  if (s.beyond) atomicAdd(&acc->beyond, (unsigned long long)s.beyond);
  if (s.first_only != NO_ROW) atomicMin(&acc->first_only_row, s.first_only);
  if (s.first_beyond != NO_ROW) atomicMin(&acc->first_beyond_row, s.first_beyond);
  if (s.unsorted) atomicOr(&acc->unsorted, 1);
  if (s.max_abs > 0.0) atomicMax(&acc->max_abs_err, dbits(s.max_abs));
  if (s.max_rel > 0.0) atomicMax(&acc->max_rel_err, dbits(s.max_rel));
  if (s.max_oa > 0.0) atomicMax(&acc->max_only_a, dbits(s.max_oa));
  if (s.max_ob > 0.0) atomicMax(&acc->max_only_b, dbits(s.max_ob));
}

// one block: the per-block partials added in a fixed order (lane-strided sums, the shuffle tree, the waves in order)
__global__ __launch_bounds__(CMP_THREADS) void k_diff_sum(int nblk, const double* __restrict__ partial, Acc* __restrict__ acc) {
  __shared__ double waves[CMP_THREADS / 64];
  double sum = 0.0;
  for (int i = threadIdx.x; i < nblk; i += CMP_THREADS) sum += partial[i];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < CMP_THREADS / 64; ++w) sum += waves[w];
  acc->sum_sq = sum;
}

// CSR::differsStats: one lane per row, a histogram per block in LDS, integer atomics into the np + 4 counters.
// rowPtr values are only subtracted here, never used as addresses.
template <class Q>
__global__ __launch_bounds__(256) void k_differs_stats(int m, const int* __restrict__ IA, const int* __restrict__ IB,
                                                       const Q* __restrict__ percents, int np, int* __restrict__ counts) {
  __shared__ int hist[MAX_PERCENTS + 4];
  __shared__ Q sp[MAX_PERCENTS];
  if (threadIdx.x < np + 4) hist[threadIdx.x] = 0;
  if (threadIdx.x < np) sp[threadIdx.x] = percents[threadIdx.x];
  __syncthreads();
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < m) {
    const int acount = IA[r + 1] - IA[r], bcount = IB[r + 1] - IB[r];
    int slot;
    if (acount == 0 && bcount > 0) slot = np + 1;
    else if (acount == 0 && bcount == 0) slot = np + 2;
    else if (acount == bcount) slot = np + 3;
    else {
      const Q percent = (Q)(bcount - acount) / (Q)acount;
      slot = 0;
      while (slot < np && !(percent < sp[slot])) ++slot;
    }
    atomicAdd(&hist[slot], 1);
  }
  __syncthreads();
  if (threadIdx.x < np + 4 && hist[threadIdx.x]) atomicAdd(&counts[threadIdx.x], hist[threadIdx.x]);
}

template <class V>
static int diff(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const V* dA, int nnzA, const int* dIB,
                const int* dJB, const V* dB, int nnzB, double rel_tol, double abs_tol, spgemm_csr_diff* out) {
  if (!out) return fail(SPGEMM_ERR_ARG, "report pointer is null");
  memset(out, 0, sizeof(*out));
  if (m < 0 || n < 0 || nnzA < 0 || nnzB < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (!dIA || !dIB) return fail(SPGEMM_ERR_ARG, "rowPtr is null");
  if ((nnzA > 0 && (!dJA || !dA)) || (nnzB > 0 && (!dJB || !dB)))
    return fail(SPGEMM_ERR_ARG, "CSR arrays null with nnzA=%d nnzB=%d", nnzA, nnzB);
  if (m == 0 && (nnzA > 0 || nnzB > 0)) return fail(SPGEMM_ERR_ARG, "entries in a matrix without rows");
  if (!(rel_tol >= 0.0) || !(abs_tol >= 0.0)) return fail(SPGEMM_ERR_ARG, "tolerances must be non-negative numbers");
  const auto none = [&]() { out->first_len_row = out->first_only_row = out->first_beyond_row = -1; return SPGEMM_OK; };
  if (m == 0) return none();
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int* bad = nullptr;
  Acc* acc = nullptr;
  double* partial = nullptr;
  // (1) both rowPtr arrays, read back before the walk forms addresses from them
  if (int rc = flag_begin(sc, s, &bad)) return sc.done(rc);
  queue_csr_checks(s, m, n, nnzA, dIA, nullptr, bad);
  queue_csr_checks(s, m, n, nnzB, dIB, nullptr, bad);
  int hbad = 0;
  if (read_flag(s, bad, &hbad)) return sc.done(SPGEMM_ERR_HIP);
  if (hbad) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer ending at nnz (nnzA=%d nnzB=%d)", nnzA, nnzB));
  const long long total = (long long)nnzA + nnzB;
  if (total == 0) return sc.done(none());
  // (2) row lengths, the walk, the partials
  const int nblk = cdiv(total, CMP_TILE);
  static const Acc fresh = {0, 0, 0, 0, 0, 0, 0, 0, NO_ROW, NO_ROW, NO_ROW, 0, 0, 0.0};
  CSR_ALLOC(&acc, sizeof(Acc));
  CSR_ALLOC(&partial, sizeof(double) * (size_t)nblk);
  CSR_HIP(hipMemcpyAsync(acc, &fresh, sizeof(Acc), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_len_differ, grid256(m), dim3(256), 0, s, m, dIA, dIB, acc);
  hipLaunchKernelGGL(k_diff_walk<V>, dim3((unsigned)nblk), dim3(CMP_THREADS), 0, s, m, nnzA, nnzB, dIA, dJA, dA, dIB, dJB, dB,
                     rel_tol, abs_tol, acc, partial);
  hipLaunchKernelGGL(k_diff_sum, dim3(1), dim3(CMP_THREADS), 0, s, nblk, partial, acc);
  CSR_HIP(hipGetLastError());
  Acc got;
  CSR_HIP(hipMemcpyAsync(&got, acc, sizeof(Acc), hipMemcpyDeviceToHost, s));
  CSR_HIP(hipStreamSynchronize(s));
  if (got.unsorted) return sc.done(fail(SPGEMM_ERR_INPUT, "a row is not strictly ascending by column (sort the rows first: hip_csr_sort_rows)"));
  const auto row = [](int r) { return r == NO_ROW ? -1 : r; };
  const auto val = [](unsigned long long b) { double d; memcpy(&d, &b, sizeof(d)); return d; };
  out->rows_len_differ = got.rows_len_differ;
  out->first_len_row = row(got.first_len_row);
  out->only_a = (long long)got.only_a;
  out->only_b = (long long)got.only_b;
  out->first_only_row = row(got.first_only_row);
  out->beyond = (long long)got.beyond;
  out->first_beyond_row = row(got.first_beyond_row);
  out->max_abs_err = val(got.max_abs_err);
  out->max_rel_err = val(got.max_rel_err);
  out->max_abs_only_a = val(got.max_only_a);
  out->max_abs_only_b = val(got.max_only_b);
  out->sum_sq = got.sum_sq;
  return sc.done(SPGEMM_OK);
}

template <class Q>
static int differs_stats(spgemm_handle* h, int m, const int* dIA, const int* dIB, const Q* percents, int npercents, int* counts) {
  if (!counts) return fail(SPGEMM_ERR_ARG, "counts pointer is null");
  if (m < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (npercents < 0 || npercents > MAX_PERCENTS) return fail(SPGEMM_ERR_ARG, "npercents=%d outside [0,%d]", npercents, MAX_PERCENTS);
  if (npercents > 0 && !percents) return fail(SPGEMM_ERR_ARG, "percents is null with npercents=%d", npercents);
  if (!dIA || !dIB) return fail(SPGEMM_ERR_ARG, "rowPtr is null");
  const int slots = npercents + 4;
  memset(counts, 0, sizeof(int) * (size_t)slots);
  if (m == 0) return SPGEMM_OK;
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int* dcounts = nullptr;
  Q* dpercents = nullptr;
  CSR_ALLOC(&dcounts, sizeof(int) * (size_t)slots);
  CSR_ALLOC(&dpercents, sizeof(Q) * (size_t)MAX_PERCENTS);
  CSR_HIP(hipMemsetAsync(dcounts, 0, sizeof(int) * (size_t)slots, s));
  if (npercents > 0) CSR_HIP(hipMemcpyAsync(dpercents, percents, sizeof(Q) * (size_t)npercents, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_differs_stats<Q>, grid256(m), dim3(256), 0, s, m, dIA, dIB, dpercents, npercents, dcounts);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipMemcpyAsync(counts, dcounts, sizeof(int) * (size_t)slots, hipMemcpyDeviceToHost, s));
  CSR_HIP(hipStreamSynchronize(s));
  return sc.done(SPGEMM_OK);
}

}  // namespace compare

extern "C" int hip_csr_diff(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const float* dA, int nnzA,
                            const int* dIB, const int* dJB, const float* dB, int nnzB, double rel_tol, double abs_tol,
                            spgemm_csr_diff* out) {
  return compare::diff<float>(h, m, n, dIA, dJA, dA, nnzA, dIB, dJB, dB, nnzB, rel_tol, abs_tol, out);
}

extern "C" int hip_csr_diff_f64(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const double* dA, int nnzA,
                                const int* dIB, const int* dJB, const double* dB, int nnzB, double rel_tol, double abs_tol,
                                spgemm_csr_diff* out) {
  return compare::diff<double>(h, m, n, dIA, dJA, dA, nnzA, dIB, dJB, dB, nnzB, rel_tol, abs_tol, out);
}

extern "C" int hip_csr_differsStats(spgemm_handle* h, int m, const int* dIA, const int* dIB, const float* percents,
                                    int npercents, int* counts) {
  return compare::differs_stats<float>(h, m, dIA, dIB, percents, npercents, counts);
}

extern "C" int hip_csr_differsStats_f64(spgemm_handle* h, int m, const int* dIA, const int* dIB, const double* percents,
                                        int npercents, int* counts) {
  return compare::differs_stats<double>(h, m, dIA, dIB, percents, npercents, counts);
}
