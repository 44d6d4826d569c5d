// Device CSR -> edge-list text on the device: the inverse of edges_device.hpp, the way out for a result.
//
// Replaces the download plus the single-threaded printf("%d\t%d\t%.6lf\n") loop of CSR::output / gpuOutputCSRWrapper
// (nlibs/CSR.cc): the lines "row SEP col SEP value\n" of entries [e0, e0 + cnt) of a device CSR are sized, placed and
// written by kernels, EW_THREADS entries per block, one per lane, through the formatter of edge_print.hpp.
//   k_edgew_length   the row of each entry (row_of_entry, bounded by the rows of the block's first and last entry), the
//                    line's length as ONE byte per entry (0 = slow) and the block's byte count; slow entries are listed
//   (the library's scan over the block byte counts: 32-bit offsets with a 64-bit total, refused above INT32_MAX)
//   k_edgew_write    a block's entries are a contiguous byte span [offs[b], offs[b+1]) of the text: an in-block scan of
//                    the length bytes places each lane, the lane formats into LDS at (span start mod 16) + its offset,
//                    and the block stores the span with 16-byte stores from the 16-byte boundary below its start; only
//                    the bytes of the first and the last 16 that belong to the span go one by one.  A span that does
//                    not fit the stage (only with long slow lines in it) is written by its lanes directly.
// An entry the formatter calls slow (edge_print.hpp: inf, nan, a value outside the format's class) goes to the host as
// (position, row, col, value): the host formats it with snprintf, k_edgew_slow_lengths adds its length to its block's
// byte count BEFORE the scan, the write pass leaves its bytes out and notes where they belong, k_edgew_slow_store puts
// them there AFTER the write pass (the mirror image of k_edges_slow_spans / pack / store).  Without slow entries -- the
// common case -- length pass, scan and the read-back of total and slow count are queued behind each other: no pass and
// no synchronisation is added.
// Generic over the value type V: float (promoted in integers, %.6lf / %.9g) or double (%.6lf / %.17g).
// Uses csr_common_device.hpp (Scratch, the call prologue, the scan, row_of_entry) and the copy lanes of hip_CSR_SpMM.
#pragma once

#include "edge_print.hpp"

#include <future>
#include <memory>

namespace edgesw {

using namespace csrdev;

constexpr int EW_THREADS = 256;                                                   // entries per block
constexpr int EW_STAGE = EW_THREADS * edgeprint::PRINT_LINE_MAX + 16;             // a block of fast lines from any alignment
constexpr size_t EW_DEFAULT_SLAB = size_t(64) << 20;                              // bytes of text per slab of the file entry
enum { EW_BAD_SPAN = 1, EW_BAD_LENGTH = 2 };
static_assert(edgeprint::PRINT_LINE_MAX < 256, "a fast line's length fits the length byte");
static_assert(edgeprint::FIXED6 == SPGEMM_EDGE_FMT_FIXED6 && edgeprint::ROUNDTRIP == SPGEMM_EDGE_FMT_ROUNDTRIP, "one numbering");

// what differs between the two value types: the bits the formatter takes, its P, and the host's snprintf
template <class V> struct PrintValue;
template <> struct PrintValue<float> {
  static constexpr int P = 9;
  static __device__ __forceinline__ uint64_t bits(float v) { return edgeprint::promote_float_bits(__float_as_uint(v)); }
  static int host(char* buf, size_t cap, int fmt, int a, int b, float v) {
    return fmt == edgeprint::FIXED6 ? snprintf(buf, cap, "%d\t%d\t%.6lf\n", a, b, (double)v) : snprintf(buf, cap, "%d %d %.9g\n", a, b, (double)v);
  }
};
template <> struct PrintValue<double> {
  static constexpr int P = 17;
  static __device__ __forceinline__ uint64_t bits(double v) { return (uint64_t)__double_as_longlong(v); }
  static int host(char* buf, size_t cap, int fmt, int a, int b, double v) {
    return fmt == edgeprint::FIXED6 ? snprintf(buf, cap, "%d\t%d\t%.6lf\n", a, b, v) : snprintf(buf, cap, "%d %d %.17g\n", a, b, v);
  }
};

// the two numbers in front of the value, as the flags want them (ONE_BASED wraps like the int it is printed as)
__host__ __device__ inline void line_indices(int row, int col, int flags, int* a, int* b) {
  if (flags & SPGEMM_EDGES_ONE_BASED) { row = (int)((unsigned)row + 1u); col = (int)((unsigned)col + 1u); }
  const bool tr = (flags & SPGEMM_EDGES_TRANSPOSE) != 0;
  *a = tr ? col : row;
  *b = tr ? row : col;
}

// rows of the first and the last entry of the block's EW_THREADS entries: every search of the block stays inside
__device__ __forceinline__ void block_rows(const int* __restrict__ IA, int m, int e0, int cnt, int (&rows)[2]) {
  if (threadIdx.x == 0) {
    const int first = blockIdx.x * EW_THREADS;
    const int last = first + EW_THREADS - 1 < cnt ? first + EW_THREADS - 1 : cnt - 1;
    rows[0] = row_of_entry(IA, 0, m - 1, e0 + first);
    rows[1] = row_of_entry(IA, rows[0], m - 1, e0 + last);
  }
  __syncthreads();
}

// sum over the block of a per-lane int (all lanes active); wsum: one slot per wave.  -> this lane's exclusive prefix
__device__ __forceinline__ int block_excl_add(int v, int (&wsum)[EW_THREADS / smf::WAVE], int* total) {
  const int tid = threadIdx.x, w = tid >> 6;
  const int incl = smf::wave_incl_add(v);
  if ((tid & 63) == 63) wsum[w] = incl;
  __syncthreads();
  int woff = 0, all = 0;
#pragma unroll
  for (int i = 0; i < EW_THREADS / smf::WAVE; ++i) { if (i < w) woff += wsum[i]; all += wsum[i]; }
  *total = all;
  return woff + incl - v;
}

// ctl[0] = number of slow entries, ctl[1] = EW_BAD_* bits (the write pass); slowList has cnt slots and gets positions
// relative to e0, in no particular order
template <class V>
__global__ __launch_bounds__(EW_THREADS) void k_edgew_length(int m, const int* __restrict__ IA, const int* __restrict__ JA,
                                                             const V* __restrict__ A, int e0, int cnt, int fmt, int flags,
                                                             unsigned char* __restrict__ lens, int* __restrict__ sums,
                                                             unsigned* __restrict__ ctl, int* __restrict__ slowList) {
  __shared__ int rows[2];
  __shared__ int wsum[EW_THREADS / smf::WAVE];
  block_rows(IA, m, e0, cnt, rows);
  const int i = blockIdx.x * EW_THREADS + threadIdx.x;
  int len = 0;
  if (i < cnt) {
    const int o = e0 + i;
    const int r = row_of_entry(IA, rows[0], rows[1], o);
    int a, b;
    line_indices(r, JA[o], flags, &a, &b);
    len = edgeprint::line_length(a, b, PrintValue<V>::bits(A[o]), fmt, PrintValue<V>::P);
    if (len == edgeprint::PRINT_SLOW) {
      len = 0;
      slowList[atomicAdd(&ctl[0], 1u)] = i;
    }
    lens[i] = (unsigned char)len;
  }
  int total;
  (void)block_excl_add(len, wsum, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// offs: the exclusive scan of the block byte counts (offs[nblocks] = the text's size).  slowPos ascending, slowLen beside
// it; slowDst[k] = where slow entry k's bytes belong.  text is 16-byte aligned (a pool block).
template <class V>
__global__ __launch_bounds__(EW_THREADS) void k_edgew_write(int m, const int* __restrict__ IA, const int* __restrict__ JA,
                                                            const V* __restrict__ A, int e0, int cnt, int fmt, int flags,
                                                            const unsigned char* __restrict__ lens, const int* __restrict__ offs,
                                                            int nslow, const int* __restrict__ slowPos,
                                                            const int* __restrict__ slowLen, int* __restrict__ slowDst,
                                                            unsigned* __restrict__ ctl, char* __restrict__ text) {
  __shared__ __attribute__((aligned(16))) char stage[EW_STAGE];
  __shared__ int rows[2];
  __shared__ int wsum[EW_THREADS / smf::WAVE];
  block_rows(IA, m, e0, cnt, rows);
  const int tid = threadIdx.x;
  const int i = blockIdx.x * EW_THREADS + tid;
  int len = 0, slowAt = -1;
  if (i < cnt) {
    len = lens[i];
    if (len == 0) {
      slowAt = first_at_least(slowPos, 0, nslow, i);
      len = slowAt < nslow && slowPos[slowAt] == i ? slowLen[slowAt] : 0;
    }
  }
  int total;
  const int excl = block_excl_add(len, wsum, &total);
  const int g0 = offs[blockIdx.x], span = offs[blockIdx.x + 1] - g0;
  if (total != span || g0 < 0 || span < 0) {                     // never with the counts the length pass wrote: no store then
    if (tid == 0) atomicOr(&ctl[1], (unsigned)EW_BAD_SPAN);
    return;
  }
  const int head = g0 & 15;
  const bool staged = head + span <= EW_STAGE;                   // the same for every lane of the block
  if (i < cnt) {
    if (slowAt >= 0) {
      if (slowAt < nslow) slowDst[slowAt] = g0 + excl;
    } else {
      const int o = e0 + i;
      const int r = row_of_entry(IA, rows[0], rows[1], o);
      int a, b;
      line_indices(r, JA[o], flags, &a, &b);
      char* dst = staged ? stage + head + excl : text + g0 + excl;
      if (edgeprint::print_line(dst, a, b, PrintValue<V>::bits(A[o]), fmt, PrintValue<V>::P) != len)
        atomicOr(&ctl[1], (unsigned)EW_BAD_LENGTH);
    }
  }
  if (!staged) return;
  __syncthreads();
  // stage[j] is the text's byte g0 - head + j; the span is j in [head, head + span)
  const int end = head + span;
  char* const base = text + (g0 - head);
  for (int c = tid * 16; c < end; c += EW_THREADS * 16) {
    if (c >= head && c + 16 <= end) {
      *reinterpret_cast<uint4*>(base + c) = *reinterpret_cast<const uint4*>(stage + c);
    } else {
      const int lo = c > head ? c : head, hi = c + 16 < end ? c + 16 : end;
      for (int j = lo; j < hi; ++j) base[j] = stage[j];
    }
  }
}

// slow entries for the host: row, column and value of the listed positions
template <class V>
__global__ void k_edgew_slow_gather(int n, int m, const int* __restrict__ IA, const int* __restrict__ JA, const V* __restrict__ A,
                                    int e0, const int* __restrict__ pos, int* __restrict__ row, int* __restrict__ col,
                                    V* __restrict__ val) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int o = e0 + pos[i];
  row[i] = row_of_entry(IA, 0, m - 1, o);
  col[i] = JA[o];
  val[i] = A[o];
}

// their lengths into the block byte counts, in front of the scan
__global__ void k_edgew_slow_lengths(int n, const int* __restrict__ pos, const int* __restrict__ len, int* __restrict__ sums) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(&sums[pos[i] / EW_THREADS], len[i]);
}

// their bytes into the text, behind the write pass: packed holds them back to back, slow entry i at srcOff[i]
__global__ void k_edgew_slow_store(int n, const int* __restrict__ dst, const int* __restrict__ len, const int* __restrict__ srcOff,
                                   const char* __restrict__ packed, int nbytes, char* __restrict__ text) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int d = dst[i], l = len[i], o = srcOff[i];
  if (d < 0 || l < 0 || (long long)d + l > nbytes) return;      // never: dst comes from the scan the lengths went into
  for (int j = 0; j < l; ++j) text[d + j] = packed[o + j];
}

static float ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// kernel times of one call from events on its stream, read after the call's last synchronisation
struct PhaseEvents {
  hipEvent_t ev[4] = {};
  bool ok = true;
  PhaseEvents() { for (auto& e : ev) ok = ok && hipEventCreate(&e) == hipSuccess; }
  ~PhaseEvents() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
  void mark(int i, hipStream_t s) { if (ok) ok = hipEventRecord(ev[i], s) == hipSuccess; }
  float between(int a, int b) const {
    float ms = 0.f;
    return ok && hipEventElapsedTime(&ms, ev[a], ev[b]) == hipSuccess ? ms : 0.f;
  }
};

// The lines of entries [e0, e0 + cnt) of the CSR as device text.  sizeOnly: stop behind the scan (*dText stays null).
// Adds to st's entries / bytes / slow_entries / ms_length / ms_scan / ms_write / ms_slow.  IA has been validated.
template <class V>
static int format_entries_impl(hipStream_t s, int m, const int* IA, const int* JA, const V* A, int e0, int cnt, int fmt, int flags,
                               bool sizeOnly, char** dText, size_t* nbytes, spgemm_edge_write_stats* st) {
  Scratch sc;
  *dText = nullptr; *nbytes = 0;
  if (cnt == 0) {
    if (!sizeOnly) CSR_ALLOC(dText, 1, true);
    return sc.done(SPGEMM_OK);
  }
  const int nblk = cdiv(cnt, EW_THREADS);
  unsigned char* lens = nullptr;
  int *sums = nullptr, *offs = nullptr, *slowList = nullptr;
  unsigned* ctl = nullptr;
  unsigned long long* tile = nullptr;
  CSR_ALLOC(&lens, (size_t)cnt);
  CSR_ALLOC(&sums, sizeof(int) * (size_t)nblk);
  CSR_ALLOC(&offs, sizeof(int) * ((size_t)nblk + 1));
  CSR_ALLOC(&slowList, sizeof(int) * (size_t)cnt);
  CSR_ALLOC(&ctl, sizeof(unsigned) * 2);
  CSR_ALLOC(&tile, scan_scratch_bytes((long long)nblk + 1));
  PhaseEvents ev;
  CSR_HIP(hipMemsetAsync(ctl, 0, sizeof(unsigned) * 2, s));
  ev.mark(0, s);
  hipLaunchKernelGGL(k_edgew_length<V>, dim3(nblk), dim3(EW_THREADS), 0, s, m, IA, JA, A, e0, cnt, fmt, flags, lens, sums, ctl, slowList);
  CSR_HIP(hipGetLastError());
  ev.mark(1, s);
  unsigned hctl[2] = {0u, 0u};
  unsigned long long total = 0;
  CSR_HIP(hipMemcpyAsync(offs, sums, sizeof(int) * (size_t)nblk, hipMemcpyDeviceToDevice, s));
  CSR_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, s));
  CSR_HIP(scan_total(s, offs, nblk, tile, &total));
  ev.mark(2, s);
  const int nslow = (int)hctl[0];
  if (hctl[0] > (unsigned)cnt) return sc.done(fail(SPGEMM_ERR_INTERNAL, "more slow entries than entries"));
  float msSlow = 0.f;
  int *slowLen = nullptr, *slowDst = nullptr, *dSrcOff = nullptr;
  char* dPacked = nullptr;
  std::vector<int> srcOff;
  std::string packed;
  if (nslow > 0) {
    // (1) which entries, in order; (2) their row, column and value; (3) snprintf; (4) the lengths in front of a second scan
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int> pos((size_t)nslow), hr((size_t)nslow), hc((size_t)nslow), hl((size_t)nslow);
    std::vector<V> hv((size_t)nslow);
    CSR_HIP(hipMemcpyAsync(pos.data(), slowList, sizeof(int) * (size_t)nslow, hipMemcpyDeviceToHost, s));
    CSR_HIP(hipStreamSynchronize(s));
    std::sort(pos.begin(), pos.end());
    int *dR = nullptr, *dC = nullptr;
    V* dV = nullptr;
    CSR_ALLOC(&dR, sizeof(int) * (size_t)nslow);
    CSR_ALLOC(&dC, sizeof(int) * (size_t)nslow);
    CSR_ALLOC(&dV, sizeof(V) * (size_t)nslow);
    CSR_ALLOC(&slowLen, sizeof(int) * (size_t)nslow);
    CSR_ALLOC(&slowDst, sizeof(int) * (size_t)nslow);
    CSR_ALLOC(&dSrcOff, sizeof(int) * (size_t)nslow);
    CSR_HIP(hipMemcpyAsync(slowList, pos.data(), sizeof(int) * (size_t)nslow, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_edgew_slow_gather<V>, grid256(nslow), dim3(256), 0, s, nslow, m, IA, JA, A, e0, slowList, dR, dC, dV);
    CSR_HIP(hipGetLastError());
    CSR_HIP(hipMemcpyAsync(hr.data(), dR, sizeof(int) * (size_t)nslow, hipMemcpyDeviceToHost, s));
    CSR_HIP(hipMemcpyAsync(hc.data(), dC, sizeof(int) * (size_t)nslow, hipMemcpyDeviceToHost, s));
    CSR_HIP(hipMemcpyAsync(hv.data(), dV, sizeof(V) * (size_t)nslow, hipMemcpyDeviceToHost, s));
    CSR_HIP(hipStreamSynchronize(s));
    srcOff.resize((size_t)nslow);
    char line[512];                                    // 11 + 1 + 11 + 1 + %.6lf of -DBL_MAX (317) + 1
    for (int i = 0; i < nslow; ++i) {
      int a, b;
      line_indices(hr[i], hc[i], flags, &a, &b);
      const int l = PrintValue<V>::host(line, sizeof(line), fmt, a, b, hv[i]);
      if (l <= 0 || l >= (int)sizeof(line)) return sc.done(fail(SPGEMM_ERR_INTERNAL, "snprintf of a slow entry returned %d", l));
      if (packed.size() + (size_t)l > (size_t)INT32_MAX) return sc.done(fail(SPGEMM_ERR_OVERFLOW, "the text exceeds INT32_MAX bytes"));
      srcOff[i] = (int)packed.size(); hl[i] = l;
      packed.append(line, (size_t)l);
    }
    CSR_HIP(hipMemcpyAsync(slowLen, hl.data(), sizeof(int) * (size_t)nslow, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_edgew_slow_lengths, grid256(nslow), dim3(256), 0, s, nslow, slowList, slowLen, sums);
    CSR_HIP(hipGetLastError());
    CSR_HIP(hipMemcpyAsync(offs, sums, sizeof(int) * (size_t)nblk, hipMemcpyDeviceToDevice, s));
    CSR_HIP(scan_total(s, offs, nblk, tile, &total));   // a block's count stays an int: 256 lines of at most 341 bytes
    msSlow = ms_since(t0);
  }
  if (st) {
    st->entries += cnt; st->slow_entries += nslow; st->bytes += (long long)total;
    st->ms_length += ev.between(0, 1); st->ms_scan += ev.between(1, 2); st->ms_slow += msSlow;
  }
  if (total > (unsigned long long)INT32_MAX)
    return sc.done(fail(SPGEMM_ERR_OVERFLOW, "%llu bytes of text: offsets are 32-bit (hip_write_edge_file writes slabs)", total));
  *nbytes = (size_t)total;
  if (sizeOnly) return sc.done(SPGEMM_OK);
  CSR_ALLOC(dText, (size_t)total, true);               // pool blocks are at least 256-byte aligned
  ev.mark(2, s);
  hipLaunchKernelGGL(k_edgew_write<V>, dim3(nblk), dim3(EW_THREADS), 0, s, m, IA, JA, A, e0, cnt, fmt, flags, lens, offs, nslow,
                     slowList, slowLen, slowDst, ctl, *dText);
  CSR_HIP(hipGetLastError());
  ev.mark(3, s);
  if (nslow > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    CSR_ALLOC(&dPacked, packed.size());
    CSR_HIP(hipMemcpyAsync(dPacked, packed.data(), packed.size(), hipMemcpyHostToDevice, s));
    CSR_HIP(hipMemcpyAsync(dSrcOff, srcOff.data(), sizeof(int) * (size_t)nslow, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_edgew_slow_store, grid256(nslow), dim3(256), 0, s, nslow, slowDst, slowLen, dSrcOff, dPacked, (int)total, *dText);
    CSR_HIP(hipGetLastError());
    CSR_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, s));
    CSR_HIP(hipStreamSynchronize(s));
    if (st) st->ms_slow += ms_since(t0);
  } else {
    CSR_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, s));
    CSR_HIP(hipStreamSynchronize(s));
  }
  if (hctl[1]) { return sc.done(fail(SPGEMM_ERR_INTERNAL, "line lengths and offsets disagree (0x%x)", hctl[1])); }
  if (st) st->ms_write += ev.between(2, 3);
  return sc.done(SPGEMM_OK);
}

// on an error the text has gone back to the pool: nothing is handed out
template <class V>
static int format_entries(hipStream_t s, int m, const int* IA, const int* JA, const V* A, int e0, int cnt, int fmt, int flags,
                          bool sizeOnly, char** dText, size_t* nbytes, spgemm_edge_write_stats* st) {
  const int rc = format_entries_impl<V>(s, m, IA, JA, A, e0, cnt, fmt, flags, sizeOnly, dText, nbytes, st);
  if (rc != SPGEMM_OK) { *dText = nullptr; *nbytes = 0; }
  return rc;
}

static int check_write_args(int m, int n, int fmt, int flags) {
  if (m < 0 || n < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (fmt != SPGEMM_EDGE_FMT_FIXED6 && fmt != SPGEMM_EDGE_FMT_ROUNDTRIP) return fail(SPGEMM_ERR_ARG, "unknown format %d", fmt);
  if (flags & ~(SPGEMM_EDGES_ONE_BASED | SPGEMM_EDGES_TRANSPOSE)) return fail(SPGEMM_ERR_ARG, "unknown flag bits 0x%x", flags);
  return SPGEMM_OK;
}

// rowPtr monotone from 0, and rowPtr[row0], rowPtr[row1] on the host: one read-back
static int row_range_entries(hipStream_t s, int m, const int* dIA, int row0, int row1, int* e0, int* e1) {
  Scratch sc;
  int* bad = nullptr;
  CHK(flag_begin(sc, s, &bad));
  queue_csr_checks(s, m, 0, -1, dIA, nullptr, bad);
  int h[2] = {0, 0};
  CSR_HIP(hipMemcpyAsync(&h[0], dIA + row0, sizeof(int), hipMemcpyDeviceToHost, s));
  CSR_HIP(hipMemcpyAsync(&h[1], dIA + row1, sizeof(int), hipMemcpyDeviceToHost, s));
  int hbad = 0;
  if (int rc = read_flag(s, bad, &hbad)) return sc.done(rc);
  if (hbad || h[0] < 0 || h[1] < h[0]) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone offset array starting at 0"));
  *e0 = h[0]; *e1 = h[1];
  return sc.done(SPGEMM_OK);
}

static void zero_stats(spgemm_edge_write_stats* st) { if (st) memset(st, 0, sizeof(*st)); }

template <class V>
static int check_range_args(int m, int n, const int* dIA, const int* dJA, const V* dA, int row0, int row1, int fmt, int flags) {
  CHK(check_write_args(m, n, fmt, flags));
  if (row0 < 0 || row0 > row1 || row1 > m) return fail(SPGEMM_ERR_ARG, "rows [%d, %d) of %d", row0, row1, m);
  if (m > 0 && (!dIA || !dJA || !dA)) return fail(SPGEMM_ERR_ARG, "CSR arrays null with m=%d", m);
  return SPGEMM_OK;
}

template <class V>
static int format_csr_edges_entry(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const V* dA, int row0, int row1,
                                  int fmt, int flags, char** dText, size_t* nbytes, spgemm_edge_write_stats* st) {
  zero_stats(st);
  if (dText) *dText = nullptr;
  if (nbytes) *nbytes = 0;
  if (!dText || !nbytes) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  CHK(check_range_args(m, n, dIA, dJA, dA, row0, row1, fmt, flags));
  hipStream_t s;
  CHK(enter(h, &s));
  const auto t0 = std::chrono::steady_clock::now();
  int e0 = 0, e1 = 0;
  if (m > 0) CHK(row_range_entries(s, m, dIA, row0, row1, &e0, &e1));
  const int rc = format_entries<V>(s, m, dIA, dJA, dA, e0, e1 - e0, fmt, flags, false, dText, nbytes, st);
  if (rc != SPGEMM_OK) { zero_stats(st); return rc; }
  if (st) { st->slabs = 1; st->ms_total = ms_since(t0); }
  return SPGEMM_OK;
}

template <class V>
static int csr_to_edge_text_entry(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const V* dA, int row0, int row1,
                                  int fmt, int flags, char* buf, size_t cap, size_t* nbytes, spgemm_edge_write_stats* st) {
  zero_stats(st);
  if (nbytes) *nbytes = 0;
  if (!nbytes) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  CHK(check_range_args(m, n, dIA, dJA, dA, row0, row1, fmt, flags));
  hipStream_t s;
  CHK(enter(h, &s));
  const auto t0 = std::chrono::steady_clock::now();
  int e0 = 0, e1 = 0;
  if (m > 0) CHK(row_range_entries(s, m, dIA, row0, row1, &e0, &e1));
  char* dText = nullptr;
  size_t need = 0;
  int rc = format_entries<V>(s, m, dIA, dJA, dA, e0, e1 - e0, fmt, flags, buf == nullptr, &dText, &need, st);
  if (rc == SPGEMM_OK && buf && need > cap) rc = fail(SPGEMM_ERR_ARG, "the buffer holds %zu bytes, the text has %zu", cap, need);
  if (rc == SPGEMM_OK && buf && need > 0) {
    const auto t1 = std::chrono::steady_clock::now();
    CopyJob job{(void*)buf, (void*)dText, need};
    rc = copy_pageable(h->device, &job, 1, false);
    if (st) st->ms_download = ms_since(t1);
  }
  if (dText) pool().release(dText);
  if (rc != SPGEMM_OK) { zero_stats(st); return rc; }
  *nbytes = need;
  if (st) { st->slabs = 1; st->ms_total = ms_since(t0); }
  return SPGEMM_OK;
}

static size_t slab_bytes_from_env() {
  const char* e = getenv("SPGEMM_EDGE_SLAB");                  // read per call
  if (!e || !*e) return EW_DEFAULT_SLAB;
  char* end = nullptr;
  const unsigned long long v = strtoull(e, &end, 10);
  if (end == e || v == 0) return EW_DEFAULT_SLAB;
  return (size_t)std::min<unsigned long long>(v, (unsigned long long)INT32_MAX);
}

// Header, then the body in slabs of at most slab / PRINT_LINE_MAX entries (at least one): a slab's text is then at most
// `slab` bytes unless it holds slow lines, ends at a line end, and may end anywhere inside a row.  Slab k is formatted and
// brought down into one of two host buffers while a second thread fwrites slab k - 1 out of the other.
template <class V>
static int write_edge_file_entry(spgemm_handle* h, const char* path, int m, int n, const int* dIA, const int* dJA, const V* dA,
                                 int fmt, int flags, int header, spgemm_edge_write_stats* st) {
  zero_stats(st);
  if (!path) return fail(SPGEMM_ERR_ARG, "path is null");
  if (header < 0 || header > 2) return fail(SPGEMM_ERR_ARG, "unknown header kind %d", header);
  CHK(check_range_args(m, n, dIA, dJA, dA, 0, m, fmt, flags));
  if (header == 2) flags |= SPGEMM_EDGES_ONE_BASED;
  struct File { FILE* fp; ~File() { if (fp) fclose(fp); } } file{fopen(path, "wb")};
  if (!file.fp) return fail(SPGEMM_ERR_ARG, "cannot open %s for writing", path);
  hipStream_t s;
  CHK(enter(h, &s));
  const auto t0 = std::chrono::steady_clock::now();
  int e0 = 0, nnz = 0;
  if (m > 0) CHK(row_range_entries(s, m, dIA, 0, m, &e0, &nnz));
  spgemm_edge_write_stats acc;
  memset(&acc, 0, sizeof(acc));
  char head[128];
  size_t headLen = 0;
  CHK(hip_edge_text_write_header(head, sizeof(head), header, m, n, (long long)nnz, &headLen));
  bool fileOk = headLen == 0 || fwrite(head, 1, headLen, file.fp) == headLen;
  acc.bytes = (long long)headLen;
  const long long per = std::max<long long>(1, (long long)(slab_bytes_from_env() / edgeprint::PRINT_LINE_MAX));
  // two host buffers of a slab's largest fast text, not initialised (a slab with slow lines may need a larger one)
  struct HostBuf {
    std::unique_ptr<char[]> p;
    size_t cap = 0;
    char* room(size_t n) { if (n > cap) { p.reset(new char[n]); cap = n; } return p.get(); }
  } hostBuf[2];
  for (auto& b : hostBuf) b.room((size_t)std::min<long long>(per, nnz) * edgeprint::PRINT_LINE_MAX);
  std::future<float> writing;                                   // the fwrite of the previous slab: its milliseconds, < 0 on error
  int rc = SPGEMM_OK;
  for (long long at = 0; at < nnz && rc == SPGEMM_OK && fileOk; at += per) {
    const int cnt = (int)std::min<long long>(per, nnz - at);
    char* dText = nullptr;
    size_t nb = 0;
    rc = format_entries<V>(s, m, dIA, dJA, dA, (int)at, cnt, fmt, flags, false, &dText, &nb, &acc);
    char* const buf = rc == SPGEMM_OK ? hostBuf[acc.slabs & 1].room(nb) : nullptr;
    if (rc == SPGEMM_OK && nb > 0) {
      const auto t1 = std::chrono::steady_clock::now();
      CopyJob job{(void*)buf, (void*)dText, nb};
      rc = copy_pageable(h->device, &job, 1, false);
      acc.ms_download += ms_since(t1);
    }
    if (dText) pool().release(dText);
    if (writing.valid()) { const float ms = writing.get(); if (ms < 0.f) fileOk = false; else acc.ms_file += ms; }
    if (rc == SPGEMM_OK && fileOk) {
      FILE* fp = file.fp;
      const char* p = buf;
      writing = std::async(std::launch::async, [fp, p, nb] {
        const auto t = std::chrono::steady_clock::now();
        return fwrite(p, 1, nb, fp) == nb ? ms_since(t) : -1.f;
      });
      ++acc.slabs;
    }
  }
  if (writing.valid()) { const float ms = writing.get(); if (ms < 0.f) fileOk = false; else acc.ms_file += ms; }
  {
    const auto t = std::chrono::steady_clock::now();
    FILE* fp = file.fp;
    file.fp = nullptr;
    if (fclose(fp) != 0) fileOk = false;
    acc.ms_file += ms_since(t);
  }
  if (rc != SPGEMM_OK) return rc;
  if (!fileOk) return fail(SPGEMM_ERR_ARG, "writing %s failed", path);
  acc.ms_total = ms_since(t0);
  if (st) *st = acc;
  return SPGEMM_OK;
}

}  // namespace edgesw

extern "C" int hip_edge_text_write_header(char* buf, size_t cap, int header, int rows, int cols, long long entries, size_t* nbytes) {
  if (nbytes) *nbytes = 0;
  if (!nbytes) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  if (header < 0 || header > 2) return fail(SPGEMM_ERR_ARG, "unknown header kind %d", header);
  if (rows < 0 || cols < 0 || entries < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (header == 0) return SPGEMM_OK;
  char line[128];
  const int l = snprintf(line, sizeof(line), "%s%d %d %lld\n", header == 2 ? "%%MatrixMarket matrix coordinate real general\n" : "",
                         rows, cols, entries);
  if (!buf || (size_t)l > cap) return fail(SPGEMM_ERR_ARG, "the header needs %d bytes, the buffer holds %zu", l, buf ? cap : (size_t)0);
  memcpy(buf, line, (size_t)l);
  *nbytes = (size_t)l;
  return SPGEMM_OK;
}

extern "C" int hip_format_csr_edges(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const float* dA, int row0,
                                    int row1, int fmt, int flags, char** dText, size_t* nbytes, spgemm_edge_write_stats* st) {
  return edgesw::format_csr_edges_entry<float>(h, m, n, dIA, dJA, dA, row0, row1, fmt, flags, dText, nbytes, st);
}
extern "C" int hip_format_csr_edges_f64(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const double* dA, int row0,
                                        int row1, int fmt, int flags, char** dText, size_t* nbytes, spgemm_edge_write_stats* st) {
  return edgesw::format_csr_edges_entry<double>(h, m, n, dIA, dJA, dA, row0, row1, fmt, flags, dText, nbytes, st);
}

extern "C" int hip_csr_to_edge_text(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const float* dA, int row0,
                                    int row1, int fmt, int flags, char* buf, size_t cap, size_t* nbytes,
                                    spgemm_edge_write_stats* st) {
  return edgesw::csr_to_edge_text_entry<float>(h, m, n, dIA, dJA, dA, row0, row1, fmt, flags, buf, cap, nbytes, st);
}
extern "C" int hip_csr_to_edge_text_f64(spgemm_handle* h, int m, int n, const int* dIA, const int* dJA, const double* dA, int row0,
                                        int row1, int fmt, int flags, char* buf, size_t cap, size_t* nbytes,
                                        spgemm_edge_write_stats* st) {
  return edgesw::csr_to_edge_text_entry<double>(h, m, n, dIA, dJA, dA, row0, row1, fmt, flags, buf, cap, nbytes, st);
}

extern "C" int hip_write_edge_file(spgemm_handle* h, const char* path, int m, int n, const int* dIA, const int* dJA, const float* dA,
                                   int fmt, int flags, int header, spgemm_edge_write_stats* st) {
  return edgesw::write_edge_file_entry<float>(h, path, m, n, dIA, dJA, dA, fmt, flags, header, st);
}
extern "C" int hip_write_edge_file_f64(spgemm_handle* h, const char* path, int m, int n, const int* dIA, const int* dJA,
                                       const double* dA, int fmt, int flags, int header, spgemm_edge_write_stats* st) {
  return edgesw::write_edge_file_entry<double>(h, path, m, n, dIA, dJA, dA, fmt, flags, header, st);
}
