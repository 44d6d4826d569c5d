// Edge-list text -> COO triplets on the device: the parse in front of hip_coo_to_csr.
//
// Replaces, for line-oriented files, the text half of COO::readSNAPFile (nlibs/COO.cc:48-158): the size
// line is read on the host (hip_edge_text_header), the edge lines "from to [value]" are cut and converted here.
//   k_edges_count    '\n' bytes per EDGE_TILE bytes of text (16-byte loads, compared byte-wise)
//   (the library's scan over the tile counts)
//   k_edges_starts   rewalks each tile: the byte offset of the start of line k, for k up to min(lines, declared)
//   k_edges_parse    one line per lane through the scanner of edge_scan.hpp, the block's span of text staged in LDS
// A line the scanner calls slow (edge_scan.hpp: what it does not promise to convert like strtol / strtof) is appended to a
// device list; the host parses exactly those lines with strtol / strtol / strtof and stores their triplets.  A line with
// fewer than two fields stops the reading as in the reference: entries = min(declared, lines, first such line).
// The parse and everything behind it is generic over the value type V: float (QValue float, strtof) or double (FDOUBLE,
// strtod, the entries named _f64).  Counting and cutting the lines does not depend on V.
// Uses csr_common_device.hpp (Scratch, the call prologue, the scan).
#pragma once

#include "edge_scan.hpp"

#include <string>
#include <sys/stat.h>

namespace edges {

using namespace csrdev;

constexpr int EDGE_THREADS = 256;
constexpr int EDGE_TILE = 4096;            // bytes of text per block of the count / starts kernels: 16 per lane
constexpr int EDGE_STAGE = 8192;           // LDS bytes k_edges_parse stages a block's 256 lines in (32 per line)
constexpr unsigned NO_BAD_LINE = 0xffffffffu;
static_assert(EDGE_TILE == EDGE_THREADS * 16, "one 16-byte load per lane");

// what differs between the two value types: the scanner's bit pattern, 1.0 (a missing value), the host's conversion
template <class V> struct EdgeValue;
template <> struct EdgeValue<float> {
  using Bits = uint32_t;
  static constexpr Bits ONE = 0x3f800000u;
  static __device__ __forceinline__ float of_bits(Bits b) { return __uint_as_float(b); }
  static float host(const char* s, char** e) { return strtof(s, e); }
};
template <> struct EdgeValue<double> {
  using Bits = uint64_t;
  static constexpr Bits ONE = 0x3ff0000000000000ull;
  static __device__ __forceinline__ double of_bits(Bits b) { return __longlong_as_double((long long)b); }
  static double host(const char* s, char** e) { return strtod(s, e); }
};

// bit i set: byte off + i of the text is '\n'.  off is a multiple of 16 and the text base 16-byte aligned; the 16 bytes
// that hold the end of the text are read one by one under the bound.
__device__ __forceinline__ unsigned newline_mask16(const unsigned char* __restrict__ text, int nbytes, long long off) {
  unsigned mask = 0;
  if (off + 16 <= nbytes) {
    const uint4 q = *reinterpret_cast<const uint4*>(text + off);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) mask |= (((w[i >> 2] >> ((i & 3) * 8)) & 0xffu) == '\n' ? 1u : 0u) << i;
  } else {
    for (int i = 0; i < 16 && off + i < nbytes; ++i) mask |= (text[off + i] == '\n' ? 1u : 0u) << i;
  }
  return mask;
}

__global__ __launch_bounds__(EDGE_THREADS) void k_edges_count(const unsigned char* __restrict__ text, int nbytes,
                                                              int* __restrict__ counts) {
  __shared__ int red[EDGE_THREADS / smf::WAVE];
  const int tid = threadIdx.x;
  const long long off = (long long)blockIdx.x * EDGE_TILE + tid * 16;
  const int c = smf::wave_sum(__popc(newline_mask16(text, nbytes, off)));
  if ((tid & 63) == 0) red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// tileOff: the exclusive scan of the counts.  Line 0 starts at 0, line k behind newline k - 1; starts[] has cap + 1 slots
// (cap = min(lines, declared) >= 1), so that line k < cap ends at starts[k + 1] - 1.  When the text's last line has no
// '\n' (tailOpen) and is among the cap, its end slot is nbytes + 1.
__global__ __launch_bounds__(EDGE_THREADS) void k_edges_starts(const unsigned char* __restrict__ text, int nbytes,
                                                               const int* __restrict__ tileOff, int cap, int lines,
                                                               int tailOpen, unsigned* __restrict__ starts) {
  __shared__ int wsum[EDGE_THREADS / smf::WAVE];
  const int tid = threadIdx.x, w = tid >> 6;
  const long long off = (long long)blockIdx.x * EDGE_TILE + tid * 16;
  unsigned mask = newline_mask16(text, nbytes, off);
  const int c = __popc(mask);
  const int incl = smf::wave_incl_add(c);
  if ((tid & 63) == 63) wsum[w] = incl;
  __syncthreads();
  int woff = 0;
  for (int i = 0; i < w; ++i) woff += wsum[i];
  long long line = (long long)tileOff[blockIdx.x] + woff + incl - c + 1;      // the line behind this lane's first newline
  while (mask) {
    const int bit = __ffs(mask) - 1;
    mask &= mask - 1;
    if (line <= cap) starts[line] = (unsigned)(off + bit + 1);
    ++line;
  }
  if (blockIdx.x == 0 && tid == 0) {
    starts[0] = 0u;
    if (tailOpen && cap == lines) starts[lines] = (unsigned)nbytes + 1u;
  }
}

// ctl[0] = first bad line (atomicMin, NO_BAD_LINE if none), ctl[1] = number of slow lines, ctl[2] = a line start that is
// out of order or outside the text was met (an internal error: nothing is read through it); slowList has cap slots.
// The block's lines k0 .. k1-1 are contiguous text [starts[k0], starts[k1] - 1): staged through LDS with 16-byte loads
// from the 16-byte boundary below its start when that fits EDGE_STAGE, else every lane reads its line from global
// memory (a line of any length).  No byte outside [0, nbytes) is read: the 16 bytes holding the end of the text are
// copied one by one.
template <class V>
__global__ __launch_bounds__(EDGE_THREADS) void k_edges_parse(const unsigned char* __restrict__ text, int nbytes,
                                                              const unsigned* __restrict__ starts, int cap, int flags,
                                                              int* __restrict__ dRow, int* __restrict__ dCol,
                                                              V* __restrict__ dVal, unsigned* __restrict__ ctl,
                                                              int* __restrict__ slowList) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[EDGE_STAGE];
  const int tid = threadIdx.x;
  const long long k0 = (long long)blockIdx.x * EDGE_THREADS;
  const long long k1 = k0 + EDGE_THREADS < cap ? k0 + EDGE_THREADS : cap;
  const unsigned s0 = starts[k0], s1 = starts[k1] - 1u;        // s1 <= nbytes
  if (s0 > s1 || s1 > (unsigned)nbytes) {                      // never with the starts k_edges_starts writes: no read then
    if (tid == 0) atomicOr(&ctl[2], 1u);
    return;
  }
  const unsigned a0 = s0 & ~15u;
  const bool staged = s1 - a0 <= (unsigned)EDGE_STAGE;         // the same for every lane of the block
  if (staged) {
    for (unsigned o = a0 + (unsigned)tid * 16u; o < s1; o += EDGE_THREADS * 16u) {
      if ((long long)o + 16 <= nbytes) {
        *reinterpret_cast<uint4*>(stage + (o - a0)) = *reinterpret_cast<const uint4*>(text + o);
      } else {
        for (unsigned i = 0; i < 16u && o + i < s1; ++i) stage[o - a0 + i] = text[o + i];
      }
    }
    __syncthreads();
  }
  const long long k = k0 + tid;
  if (k >= cap) return;
  const unsigned b = starts[k], e = starts[k + 1] - 1u;
  if (b < s0 || e < b || e > s1) { atomicOr(&ctl[2], 1u); return; }
  const int len = (int)(e - b);
  int from = 0, to = 0;
  typename EdgeValue<V>::Bits vbits = EdgeValue<V>::ONE;      // a missing value is 1.0
  const int got = staged ? edgescan::edge_scan_line_as(stage + (b - a0), len, &from, &to, &vbits)
                         : edgescan::edge_scan_line_as(text + b, len, &from, &to, &vbits);
  if (got == edgescan::EDGE_SLOW) {
    slowList[atomicAdd(&ctl[1], 1u)] = (int)k;
  } else if (got < 2) {
    atomicMin(&ctl[0], (unsigned)k);
  } else {
    if (flags & SPGEMM_EDGES_ONE_BASED) { from = (int)((unsigned)from - 1u); to = (int)((unsigned)to - 1u); }
    const bool tr = (flags & SPGEMM_EDGES_TRANSPOSE) != 0;
    dRow[k] = tr ? to : from;
    dCol[k] = tr ? from : to;
    dVal[k] = EdgeValue<V>::of_bits(vbits);
  }
}

// the slow lines' text for the host: {start, length} per listed line, then the bytes packed at the host's offsets
__global__ void k_edges_slow_spans(int n, const int* __restrict__ list, const unsigned* __restrict__ starts,
                                   unsigned* __restrict__ spans) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = list[i];
  spans[2 * i] = starts[k];
  spans[2 * i + 1] = starts[k + 1] - 1u - starts[k];
}

__global__ void k_edges_slow_pack(int n, const unsigned* __restrict__ spans, const unsigned* __restrict__ offs,
                                  const unsigned char* __restrict__ text, unsigned char* __restrict__ packed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned b = spans[2 * i], len = spans[2 * i + 1], o = offs[i];
  for (unsigned j = 0; j < len; ++j) packed[o + j] = text[b + j];
}

template <class V>
__global__ void k_edges_slow_store(int n, const int* __restrict__ at, const int* __restrict__ r, const int* __restrict__ c,
                                   const V* __restrict__ v, int* __restrict__ dRow, int* __restrict__ dCol,
                                   V* __restrict__ dVal) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dRow[at[i]] = r[i]; dCol[at[i]] = c[i]; dVal[at[i]] = v[i];
}

// parse_edge of nlibs/COO.cc, the conversions sscanf("%d%d%f") performs ("%d%d%lf" under FDOUBLE): what a slow line is
// parsed with
template <class V>
static int host_parse_edge(const char* s, int* from, int* to, V* val) {
  char* e = nullptr;
  const long a = strtol(s, &e, 10);
  if (e == s) return 0;
  const char* s2 = e;
  const long b = strtol(s2, &e, 10);
  if (e == s2) return 1;
  *from = (int)a; *to = (int)b;
  const char* s3 = e;
  const V v = EdgeValue<V>::host(s3, &e);
  if (e == s3) return 2;
  *val = v;
  return 3;
}

static float ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// the argument checks the three device entries share; outputs are already known to be non-null
static int check_edge_args(const void* text, size_t nbytes, int flags) {
  if (!text && nbytes > 0) return fail(SPGEMM_ERR_ARG, "text is null with nbytes=%zu", nbytes);
  if (flags & ~(SPGEMM_EDGES_ONE_BASED | SPGEMM_EDGES_TRANSPOSE)) return fail(SPGEMM_ERR_ARG, "unknown flag bits 0x%x", flags);
  return SPGEMM_OK;
}

// The device work behind both entries.  dText: the text on the device (16-byte aligned); hText: the same bytes on the
// host, or null (then the slow lines, and only they, are copied back).  Fills st's lines / first_bad_line / entries /
// slow_lines / ms_split / ms_parse / ms_slow.
template <class V>
static int parse_lines(hipStream_t s, const unsigned char* dText, const char* hText, int nbytes, int declared, int flags,
                       int** dRow, int** dCol, V** dVal, int* entries, spgemm_edge_stats* st) {
  Scratch sc;
  auto t0 = std::chrono::steady_clock::now();
  long long lines = 0;
  int* counts = nullptr;
  const int ntiles = cdiv(nbytes, EDGE_TILE);
  unsigned char last = '\n';                          // the text's last byte: a line without '\n' behind it counts too
  if (nbytes > 0) {
    unsigned long long* tile = nullptr;
    CSR_ALLOC(&counts, sizeof(int) * ((size_t)ntiles + 1));
    CSR_ALLOC(&tile, scan_scratch_bytes((long long)ntiles + 1));
    hipLaunchKernelGGL(k_edges_count, dim3(ntiles), dim3(EDGE_THREADS), 0, s, dText, nbytes, counts);
    if (hText) last = (unsigned char)hText[nbytes - 1];
    else CSR_HIP(hipMemcpyAsync(&last, dText + nbytes - 1, 1, hipMemcpyDeviceToHost, s));   // lands before scan_total's wait
    unsigned long long newlines = 0;
    CSR_HIP(scan_total(s, counts, ntiles, tile, &newlines));
    lines = (long long)newlines + (last != '\n' ? 1 : 0);
  }
  const int cap = (int)std::min<long long>(std::max(declared, 0), lines);
  int *R = nullptr, *C = nullptr;
  V* W = nullptr;
  CSR_ALLOC(&R, sizeof(int) * (size_t)std::max(cap, 1), true);
  CSR_ALLOC(&C, sizeof(int) * (size_t)std::max(cap, 1), true);
  CSR_ALLOC(&W, sizeof(V) * (size_t)std::max(cap, 1), true);
  long long firstBad = -1;
  int nslow = 0;
  float msSplit = 0.f, msParse = 0.f, msSlow = 0.f;
  if (cap > 0) {
    unsigned *starts = nullptr, *ctl = nullptr;
    int* slowList = nullptr;
    CSR_ALLOC(&starts, sizeof(unsigned) * ((size_t)cap + 1));
    CSR_ALLOC(&ctl, sizeof(unsigned) * 3);
    CSR_ALLOC(&slowList, sizeof(int) * (size_t)cap);
    CSR_HIP(hipMemsetAsync(ctl, 0xff, sizeof(unsigned), s));
    CSR_HIP(hipMemsetAsync(ctl + 1, 0, sizeof(unsigned) * 2, s));
    hipLaunchKernelGGL(k_edges_starts, dim3(ntiles), dim3(EDGE_THREADS), 0, s, dText, nbytes, counts, cap, (int)lines,
                       last != '\n' ? 1 : 0, starts);
    CSR_HIP(hipGetLastError());
    CSR_HIP(hipStreamSynchronize(s));
    msSplit = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(k_edges_parse<V>, dim3(cdiv(cap, EDGE_THREADS)), dim3(EDGE_THREADS), 0, s, dText, nbytes, starts, cap,
                       flags, R, C, W, ctl, slowList);
    CSR_HIP(hipGetLastError());
    unsigned hctl[3] = {NO_BAD_LINE, 0u, 0u};
    CSR_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, s));
    CSR_HIP(hipStreamSynchronize(s));
    if (hctl[2] || hctl[1] > (unsigned)cap) return sc.done(fail(SPGEMM_ERR_INTERNAL, "line starts out of order"));
    msParse = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (hctl[0] != NO_BAD_LINE) firstBad = (long long)hctl[0];
    nslow = (int)hctl[1];
    if (nslow > 0) {
      // (1) where the slow lines are; (2) their bytes: the host's own copy, or packed on the device and copied back
      unsigned* dSpans = nullptr;
      std::vector<int> list((size_t)nslow);
      std::vector<unsigned> spans((size_t)nslow * 2);
      CSR_ALLOC(&dSpans, sizeof(unsigned) * 2 * (size_t)nslow);
      hipLaunchKernelGGL(k_edges_slow_spans, grid256(nslow), dim3(256), 0, s, nslow, slowList, starts, dSpans);
      CSR_HIP(hipMemcpyAsync(list.data(), slowList, sizeof(int) * (size_t)nslow, hipMemcpyDeviceToHost, s));
      CSR_HIP(hipMemcpyAsync(spans.data(), dSpans, sizeof(unsigned) * 2 * (size_t)nslow, hipMemcpyDeviceToHost, s));
      CSR_HIP(hipStreamSynchronize(s));
      std::vector<unsigned> offs((size_t)nslow);
      std::vector<unsigned char> packed;
      if (!hText) {
        size_t total = 0;
        for (int i = 0; i < nslow; ++i) { offs[i] = (unsigned)total; total += spans[2 * (size_t)i + 1]; }   // <= nbytes
        packed.resize(std::max<size_t>(total, 1));
        unsigned* dOffs = nullptr;
        unsigned char* dPacked = nullptr;
        CSR_ALLOC(&dOffs, sizeof(unsigned) * (size_t)nslow);
        CSR_ALLOC(&dPacked, std::max<size_t>(total, 1));
        CSR_HIP(hipMemcpyAsync(dOffs, offs.data(), sizeof(unsigned) * (size_t)nslow, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_edges_slow_pack, grid256(nslow), dim3(256), 0, s, nslow, dSpans, dOffs, dText, dPacked);
        if (total) CSR_HIP(hipMemcpyAsync(packed.data(), dPacked, total, hipMemcpyDeviceToHost, s));
        CSR_HIP(hipStreamSynchronize(s));
      }
      // (3) exactly parse_edge on each; the good ones go back as {line, row, col, value}
      std::vector<int> at, hr, hc;
      std::vector<V> hv;
      std::string line;
      for (int i = 0; i < nslow; ++i) {
        const unsigned len = spans[2 * (size_t)i + 1];
        const char* p = hText ? hText + spans[2 * (size_t)i] : (const char*)packed.data() + offs[i];
        line.assign(p, len);
        int from = 0, to = 0;
        V val = 1;
        const int got = host_parse_edge<V>(line.c_str(), &from, &to, &val);
        if (got < 2) { if (firstBad < 0 || list[i] < firstBad) firstBad = list[i]; continue; }
        if (flags & SPGEMM_EDGES_ONE_BASED) { from = (int)((unsigned)from - 1u); to = (int)((unsigned)to - 1u); }
        const bool tr = (flags & SPGEMM_EDGES_TRANSPOSE) != 0;
        at.push_back(list[i]); hr.push_back(tr ? to : from); hc.push_back(tr ? from : to); hv.push_back(val);
      }
      if (const int n = (int)at.size()) {
        int *dAt = nullptr, *dR = nullptr, *dC = nullptr;
        V* dV = nullptr;
        CSR_ALLOC(&dAt, sizeof(int) * (size_t)n);
        CSR_ALLOC(&dR, sizeof(int) * (size_t)n);
        CSR_ALLOC(&dC, sizeof(int) * (size_t)n);
        CSR_ALLOC(&dV, sizeof(V) * (size_t)n);
        CSR_HIP(hipMemcpyAsync(dAt, at.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
        CSR_HIP(hipMemcpyAsync(dR, hr.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
        CSR_HIP(hipMemcpyAsync(dC, hc.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
        CSR_HIP(hipMemcpyAsync(dV, hv.data(), sizeof(V) * (size_t)n, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_edges_slow_store<V>, grid256(n), dim3(256), 0, s, n, dAt, dR, dC, dV, R, C, W);
        CSR_HIP(hipGetLastError());
        CSR_HIP(hipStreamSynchronize(s));
      }
      msSlow = ms_since(t0);
    }
  } else {
    CSR_HIP(hipStreamSynchronize(s));
    msSplit = ms_since(t0);
  }
  const int n = (int)(firstBad >= 0 ? std::min<long long>(cap, firstBad) : cap);
  if (st) {
    st->lines = lines; st->first_bad_line = firstBad; st->entries = n; st->slow_lines = nslow;
    st->ms_split = msSplit; st->ms_parse = msParse; st->ms_slow = msSlow;
  }
  *dRow = R; *dCol = C; *dVal = W; *entries = n;
  return sc.done(SPGEMM_OK);
}

template <class V>
static bool null_outputs(int** a, int** b, V** c, int* n, spgemm_edge_stats* st) {
  if (st) memset(st, 0, sizeof(*st));
  if (st) st->first_bad_line = -1;
  if (!a || !b || !c || !n) return true;
  *a = nullptr; *b = nullptr; *c = nullptr; *n = 0;
  return false;
}

}  // namespace edges

extern "C" int hip_edge_text_header(const char* text, size_t nbytes, int* rows, int* cols, int* declared, int* one_based,
                                    int* symmetric, size_t* data_offset) {
  if (!rows || !cols || !declared || !one_based || !symmetric || !data_offset) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *rows = *cols = *declared = *one_based = *symmetric = 0;
  *data_offset = 0;
  if (!text && nbytes > 0) return fail(SPGEMM_ERR_ARG, "text is null with nbytes=%zu", nbytes);
  size_t pos = 0;
  std::string line;
  auto next = [&]() {                                  // fgets over the buffer: the line with its '\n'
    if (pos >= nbytes) return false;
    const char* nl = (const char*)memchr(text + pos, '\n', nbytes - pos);
    const size_t stop = nl ? (size_t)(nl - text) + 1 : nbytes;
    line.assign(text + pos, stop - pos);
    pos = stop;
    return true;
  };
  if (!next()) return SPGEMM_OK;
  if (line[0] == '%') {                                // MatrixMarket banner: 5 tokens, the 5th is the storage scheme
    char t[5][64];
    if (sscanf(line.c_str(), "%63s %63s %63s %63s %63s", t[0], t[1], t[2], t[3], t[4]) == 5) {
      *one_based = 1;
      for (char* p = t[4]; *p; ++p) *p = (char)tolower((unsigned char)*p);
      *symmetric = strcmp(t[4], "symmetric") == 0;
    }
  }
  while (line[0] == '#' || line[0] == '%')
    if (!next()) return SPGEMM_OK;                     // only comments: no sizes, nothing to parse
  int a = 0, b = 0, c = 0;
  const int got = sscanf(line.c_str(), "%d %d %d", &a, &b, &c);
  if (got == 2) { *rows = *cols = a; *declared = b; }
  else if (got == 3) { *rows = a; *cols = b; *declared = c; }
  else return fail(SPGEMM_ERR_INPUT, "cannot parse the size line");
  *data_offset = pos;
  return SPGEMM_OK;
}

// ---- the three entries, for V = float and V = double ---------------------------------------------------------------------
namespace edges {

template <class V>
static int parse_edge_lines_entry(spgemm_handle* h, const char* dText, size_t nbytes, int declared, int flags, int** dRow,
                                  int** dCol, V** dVal, int* entries, spgemm_edge_stats* st) {
  if (null_outputs(dRow, dCol, dVal, entries, st)) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  CHK(check_edge_args(dText, nbytes, flags));
  if ((uintptr_t)dText & 15u) return fail(SPGEMM_ERR_ARG, "the device text is not 16-byte aligned");
  if (nbytes > (size_t)INT32_MAX) return fail(SPGEMM_ERR_OVERFLOW, "%zu bytes of text: offsets are 32-bit", nbytes);
  hipStream_t s;
  CHK(enter(h, &s));
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = parse_lines<V>(s, (const unsigned char*)dText, nullptr, (int)nbytes, declared, flags, dRow, dCol, dVal, entries, st);
  if (st && rc == SPGEMM_OK) st->ms_total = ms_since(t0);
  return rc;
}

template <class V>
static int parse_edge_text_entry(spgemm_handle* h, const char* text, size_t nbytes, int declared, int flags, int** dRow,
                                 int** dCol, V** dVal, int* entries, spgemm_edge_stats* st) {
  if (null_outputs(dRow, dCol, dVal, entries, st)) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  CHK(check_edge_args(text, nbytes, flags));
  if (nbytes > (size_t)INT32_MAX) return fail(SPGEMM_ERR_OVERFLOW, "%zu bytes of text: offsets are 32-bit", nbytes);
  hipStream_t s;
  CHK(enter(h, &s));
  const auto t0 = std::chrono::steady_clock::now();
  Scratch sc;
  unsigned char* dText = nullptr;
  CSR_ALLOC(&dText, std::max<size_t>(nbytes, 1));       // pool blocks are at least 256-byte aligned
  CopyJob job{(void*)text, (void*)dText, nbytes};
  if (int rc = copy_pageable(h->device, &job, 1, true)) return sc.done(rc);
  const float msUpload = ms_since(t0);
  const int rc = parse_lines<V>(s, dText, text, (int)nbytes, declared, flags, dRow, dCol, dVal, entries, st);
  if (st && rc == SPGEMM_OK) { st->ms_upload = msUpload; st->ms_total = ms_since(t0); }
  sc.done(SPGEMM_OK);                                   // the text copy goes back to the pool either way
  return rc;
}

static int coo_to_csr_of(spgemm_handle* h, int rows, int cols, int nnz, const int* dRow, const int* dCol, const float* dVal,
                         int flags, int** dIA, int** dJA, float** dA, int* nnzOut) {
  return hip_coo_to_csr(h, rows, cols, nnz, dRow, dCol, dVal, flags, dIA, dJA, dA, nnzOut);
}
static int coo_to_csr_of(spgemm_handle* h, int rows, int cols, int nnz, const int* dRow, const int* dCol, const double* dVal,
                         int flags, int** dIA, int** dJA, double** dA, int* nnzOut) {
  return hip_coo_to_csr_f64(h, rows, cols, nnz, dRow, dCol, dVal, flags, dIA, dJA, dA, nnzOut);
}

template <class V>
static int read_edge_file_entry(spgemm_handle* h, const char* path, int isTrans, int cooFlags, int* rows, int* cols,
                                int** dIA, int** dJA, V** dA, int* nnz, spgemm_edge_stats* st) {
  if (null_outputs(dIA, dJA, dA, nnz, st) || !rows || !cols) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  *rows = *cols = 0;
  if (!path) return fail(SPGEMM_ERR_ARG, "path is null");
  FILE* fp = fopen(path, "rb");
  if (!fp) return fail(SPGEMM_ERR_ARG, "cannot open %s", path);
  struct stat sb;
  if (fstat(fileno(fp), &sb) != 0 || !S_ISREG(sb.st_mode)) { fclose(fp); return fail(SPGEMM_ERR_ARG, "%s is not a readable file", path); }
  if (sb.st_size > (off_t)INT32_MAX) { fclose(fp); return fail(SPGEMM_ERR_OVERFLOW, "%s: %lld bytes, offsets are 32-bit", path, (long long)sb.st_size); }
  // The file is mapped, not copied: the upload lanes then move it from the page cache straight into their pinned slots,
  // eight threads at a time (a malloc()ed copy costs a single-threaded pass over the text plus its page faults first).
  // The mapping is private and read-only; the file must not be truncated while the call runs.
  const size_t len = (size_t)sb.st_size;
  struct Map { void* p; size_t n; ~Map() { if (p != MAP_FAILED && n) munmap(p, n); } } map{MAP_FAILED, len};
  if (len > 0) {
    map.p = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fileno(fp), 0);
    if (map.p == MAP_FAILED) { fclose(fp); return fail(SPGEMM_ERR_ARG, "cannot map %s", path); }
    (void)madvise(map.p, len, MADV_WILLNEED);
  }
  fclose(fp);
  const char* const text = len > 0 ? (const char*)map.p : "";
  int r = 0, c = 0, declared = 0, oneBased = 0, symmetric = 0;
  size_t off = 0;
  CHK(hip_edge_text_header(text, len, &r, &c, &declared, &oneBased, &symmetric, &off));
  if (symmetric) return fail(SPGEMM_ERR_INPUT, "%s is a symmetric MatrixMarket file, a token stream: use the host loader", path);
  const int flags = (oneBased ? SPGEMM_EDGES_ONE_BASED : 0) | (isTrans ? SPGEMM_EDGES_TRANSPOSE : 0);
  int *dR = nullptr, *dC = nullptr, n = 0;
  V* dV = nullptr;
  CHK(parse_edge_text_entry<V>(h, text + off, len - off, declared, flags, &dR, &dC, &dV, &n, st));
  const int rc = coo_to_csr_of(h, r, c, n, dR, dC, dV, cooFlags, dIA, dJA, dA, nnz);
  pool().release(dR); pool().release(dC); pool().release(dV);
  if (rc == SPGEMM_OK) { *rows = r; *cols = c; }
  return rc;
}

}  // namespace edges

extern "C" int hip_parse_edge_lines(spgemm_handle* h, const char* dText, size_t nbytes, int declared, int flags,
                                    int** dRow, int** dCol, float** dVal, int* entries, spgemm_edge_stats* st) {
  return edges::parse_edge_lines_entry<float>(h, dText, nbytes, declared, flags, dRow, dCol, dVal, entries, st);
}
extern "C" int hip_parse_edge_lines_f64(spgemm_handle* h, const char* dText, size_t nbytes, int declared, int flags,
                                        int** dRow, int** dCol, double** dVal, int* entries, spgemm_edge_stats* st) {
  return edges::parse_edge_lines_entry<double>(h, dText, nbytes, declared, flags, dRow, dCol, dVal, entries, st);
}

extern "C" int hip_parse_edge_text(spgemm_handle* h, const char* text, size_t nbytes, int declared, int flags,
                                   int** dRow, int** dCol, float** dVal, int* entries, spgemm_edge_stats* st) {
  return edges::parse_edge_text_entry<float>(h, text, nbytes, declared, flags, dRow, dCol, dVal, entries, st);
}
extern "C" int hip_parse_edge_text_f64(spgemm_handle* h, const char* text, size_t nbytes, int declared, int flags,
                                       int** dRow, int** dCol, double** dVal, int* entries, spgemm_edge_stats* st) {
  return edges::parse_edge_text_entry<double>(h, text, nbytes, declared, flags, dRow, dCol, dVal, entries, st);
}

extern "C" int hip_read_edge_file(spgemm_handle* h, const char* path, int isTrans, int cooFlags, int* rows, int* cols,
                                  int** dIA, int** dJA, float** dA, int* nnz, spgemm_edge_stats* st) {
  return edges::read_edge_file_entry<float>(h, path, isTrans, cooFlags, rows, cols, dIA, dJA, dA, nnz, st);
}
extern "C" int hip_read_edge_file_f64(spgemm_handle* h, const char* path, int isTrans, int cooFlags, int* rows, int* cols,
                                      int** dIA, int** dJA, double** dA, int* nnz, spgemm_edge_stats* st) {
  return edges::read_edge_file_entry<double>(h, path, isTrans, cooFlags, rows, cols, dIA, dJA, dA, nnz, st);
}
