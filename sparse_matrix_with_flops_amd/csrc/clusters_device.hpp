// Clusters from a finished R-MCL flow matrix on the device: attractors, connected components, labels -> clusters.
//
// The reference stops at Mt (nlibs/qrmcl.cc:136-164): reading clusters out of it meant a download and a union-find on the
// host.  Nothing here is mirrored; the semantics are this library's and are pinned by tests/clusters_ref.py.
//
//   hip_rmcl_attractors           parent[i] = column of the largest value of row i (row i = the flow out of node i)
//   hip_csr_connected_components  label[v]  = smallest vertex id of v's weakly connected component (pattern only)
//   hip_labels_to_clusters        canonical labels -> cluster numbers, and the members of every cluster
//   hip_rmcl_clusters             the three chained: components of the functional graph i -> parent[i]
//
// Attractors.  G lanes per row, G in {4, 16, 64} picked on the host from nnz / m (lanes_per_row).  Every lane strides
// over its row keeping one (value, column) pair, the G lanes fold their pairs with __shfl_xor, and lanes 0 .. 64/G-1
// of a wave store the wave's 64/G consecutive parents with one store instruction.  No LDS, no atomics.  The order on
// pairs: (v, c) beats (bv, bc) iff v > bv, or v == bv and c < bc, from (-inf, INT_MAX).  A NaN compares false both ways
// and never wins; -0.0 == +0.0, so the smaller column wins between them.  "Beats or equals" is a total preorder on the
// non-NaN pairs and two pairs that tie in both fields are interchangeable, so the winner does not depend on the order in
// which pairs meet: not on the storage order of the row, not on G.  Values are compared in V; double never passes float.
//
// Components: hook and shortcut in rounds on ONE array f (the caller's label array), f[v] = v at the start.
//   hook      for every stored entry (u, v): fu = f[u], fv = f[v] (relaxed agent-scope atomic loads); if they differ,
//             atomicMin(&f[max(fu, fv)], min(fu, fv)); a returned old value above the new one sets changed[round].
//   shortcut  every vertex chases f towards its root (the x with f[x] == x) and stores where it got.  Nothing hooks
//             meanwhile.  A chase takes at most CC_CHASE steps; a lane that has not seen its root by then says so in a
//             second word, and the host repeats the shortcut until no lane says so (every pass divides the depth of the
//             forest by CC_CHASE, so a chain of 2^31 is flat after six; trees of R-MCL and of scrambled ids need one).
// The host reads {changed, cut short} of a round behind its two kernels, in one copy; a round whose hook changed nothing
// ends the loop.
//
// Why this is right although the L2s of the XCDs are not coherent with each other, that is, although a load inside a
// kernel may return an OLDER value of a word that another block is lowering (never one older than the kernel's start:
// a kernel boundary on one stream writes back and invalidates, so each kernel starts from a fresh view):
//   (a) f[x] <= x always.  True at the start; a hook stores min(fu, fv) into f[max(fu, fv)] only if that lowers it; the
//       shortcut stores a value reached by descending from f[x].
//   (b) f[x] is always a vertex of x's component.  Every value ever stored in f was read from f (by induction a vertex of
//       the component of the word it was read from), and a hook joins f[u] and f[v] only across a stored entry (u, v).
//       A stale fu or fv is an earlier value of the same word: (a) and (b) held for it as well.
//   (c) Every word only ever decreases, and atomicMin acts on the word itself, not on a cached copy: a stale load can
//       make a hook aim at a vertex that is no root any more or offer a larger value than the newest one, which costs a
//       round at worst.  It cannot raise a word or carry a vertex across components.
//   (d) The shortcut.  During its passes nobody hooks, so the roots of the round's forest do not move; every value a
//       pass stores into f[x] is an ancestor of x in that forest, so a chase that meets an older or a newer value of
//       f[x] is still on x's way to root(x).  By (a) each step descends strictly (the loop also stops at any step that
//       would not).  A pass in which no chase was cut short has stored root(x) into every f[x]: behind the shortcut the
//       forest is flat, f[f[x]] == f[x], at the start of every hook kernel.
//   (e) The fixed point.  If a hook kernel lowers nothing, f did not move during it, so every load returned the flat
//       forest of its start.  An entry with fu != fv would then have found the root max(fu, fv) with f[root] == root
//       above min(fu, fv) and lowered it: so every stored entry has fu == fv.  f is then constant on every component, its
//       value c satisfies f[c] == c (flat) and c <= x for every x of the component (a): c is the minimum.
//   (f) Termination.  sum(f) is a non-negative integer that strictly decreases in every round but the last.  Faster:
//       a root with a stored entry to a tree of a smaller root is no root after the hook, whatever the loads returned
//       (either the hook aimed at it, or the load saw it lowered already), so the number of trees of a component at
//       least halves per round: at most ceil(log2 m) + 1 rounds.  CC_MAX_ROUNDS (64) is far above that; reaching it
//       returns SPGEMM_ERR_INTERNAL, never a spin.
// No floating-point atomic, no wait of one block for another, nothing depends on the order in which blocks run; the result
// is the same array on every call.  A path whose ids ascend along it hooks into ONE chain in round 1: that is the case
// the bound on a chase is for (an unbounded chase would make m^2 / 2 dependent loads there).
//
// Labels -> clusters.  Validated first: 0 <= label[v] <= v and label[label[v]] == label[v] (the second read happens only
// behind the first test, in the same lane).  rank = exclusive scan of (label[v] == v), k = its total,
// cluster[v] = rank[label[v]]; the keys (cluster << 32) | v start in ascending v, so stable radix passes over the cluster
// bits alone leave every cluster's members ascending; ptr[c] = lower bound of c << 32 in the sorted keys.
// Uses csr_common_device.hpp (Scratch, enter, check_csr_args, validate_csr, scan_total, radix_sort_bits, first_at_least).
#pragma once

namespace clusters {

using namespace csrdev;

constexpr int CL_THREADS = 256;
constexpr int CC_MAX_ROUNDS = SPGEMM_CC_MAX_ROUNDS;
constexpr int CC_CHASE = 64;                               // steps of one chase
constexpr int CC_MAX_PASSES = 8;                           // shortcut passes of one round: 64^6 > 2^31
enum { BAD_LABEL = 32 };

// lanes per row of the attractor and hook kernels, from the mean row length
static inline int lanes_per_row(int m, int nnz) {
  const int avg = m > 0 ? nnz / m : 0;
  return avg <= 8 ? 4 : avg <= 64 ? 16 : 64;
}
static inline dim3 row_grid(int m, int G) { return dim3((unsigned)std::max<long long>(1, ((long long)m * G + CL_THREADS - 1) / CL_THREADS)); }

template <class V>
__device__ __forceinline__ bool beats(V v, int c, V bv, int bc) { return v > bv || (v == bv && c < bc); }

__device__ __forceinline__ int load_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <class V, int G>
__global__ __launch_bounds__(CL_THREADS) void k_attractors(int m, const int* __restrict__ IA, const int* __restrict__ JA,
                                                           const V* __restrict__ A, int* __restrict__ parent) {
  const int lane = threadIdx.x & 63, sub = lane & (G - 1);
  const long long t = (long long)blockIdx.x * CL_THREADS + threadIdx.x;
  const long long row = t / G;
  V bv = (V)-INFINITY;
  int bc = INT_MAX;
  if (row < m) {
    const long long e = IA[row + 1];
    for (long long o = (long long)IA[row] + sub; o < e; o += G) {
      const V v = A[o];
      const int c = JA[o];
      if (beats(v, c, bv, bc)) { bv = v; bc = c; }
    }
  }
#pragma unroll
  for (int d = G / 2; d > 0; d >>= 1) {                      // every lane of the wave takes part: rows past m hold the start pair
    const V ov = __shfl_xor(bv, d);
    const int oc = __shfl_xor(bc, d);
    if (beats(ov, oc, bv, bc)) { bv = ov; bc = oc; }
  }
  // the wave's 64 / G rows are consecutive: lane l takes the winner of group l, one store instruction per wave
  const int got = __shfl(bc, (lane * G) & 63);
  const long long r = (t - lane) / G + lane;
  if (lane < 64 / G && r < m) parent[r] = got == INT_MAX ? (int)r : got;
}

template <int G>
__global__ __launch_bounds__(CL_THREADS) void k_cc_hook(int m, const int* __restrict__ IA, const int* __restrict__ JA, int* f,
                                                        int* changed) {
  const int sub = threadIdx.x & (G - 1);
  const long long row = ((long long)blockIdx.x * CL_THREADS + threadIdx.x) / G;
  if (row >= m) return;
  bool lowered = false;
  const long long e = IA[row + 1];
  for (long long o = (long long)IA[row] + sub; o < e; o += G) {
    const int fu = load_agent(f + row), fv = load_agent(f + JA[o]);
    if (fu == fv) continue;
    const int hi = max(fu, fv), lo = min(fu, fv);
    if (atomicMin(f + hi, lo) > lo) lowered = true;
  }
  if (lowered) __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CL_THREADS) void k_cc_shortcut(int m, int* f, int* cut) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= m) return;
  const int first = load_agent(f + x);
  int r = first;
  bool root = false;
  for (int step = 0; step < CC_CHASE; ++step) {
    const int p = load_agent(f + r);
    if (p >= r) { root = true; break; }                      // p == r: the root; p > r never (f[x] <= x), and would end here too
    r = p;
  }
  if (r != first) __hip_atomic_store(f + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!root) __hip_atomic_store(cut, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CL_THREADS) void k_count_roots(int m, const int* __restrict__ label, int* __restrict__ count) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long roots = __ballot(v < m && label[v] == v);
  if ((threadIdx.x & 63) == 0 && roots) atomicAdd(count, __popcll(roots));
}

// canonical: label[v] in [0, v] and label[label[v]] == label[v]
__global__ void k_check_labels(int m, const int* __restrict__ label, int* __restrict__ bad) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= m) return;
  const int l = label[v];
  if ((unsigned)l > (unsigned)v || label[l] != l) atomicOr(bad, (int)BAD_LABEL);
}

__global__ void k_is_root(int m, const int* __restrict__ label, int* __restrict__ rank) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < m) rank[v] = label[v] == v;
}

__global__ void k_cluster_keys(int m, const int* __restrict__ label, const int* __restrict__ rank, int* __restrict__ cluster,
                               unsigned long long* __restrict__ keys, int* __restrict__ ids) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= m) return;
  const int c = rank[label[v]];
  cluster[v] = c;
  keys[v] = ((unsigned long long)(unsigned)c << 32) | (unsigned)v;
  ids[v] = v;
}

__global__ void k_cluster_starts(int m, int k, const unsigned long long* __restrict__ keys, int* __restrict__ ptr) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= k) ptr[c] = first_at_least(keys, 0, m, (unsigned long long)(unsigned)c << 32);
}

template <class V>
static void launch_attractors(hipStream_t s, int G, int m, const int* dIA, const int* dJA, const V* dA, int* dParent) {
  if (G == 4) hipLaunchKernelGGL((k_attractors<V, 4>), row_grid(m, 4), dim3(CL_THREADS), 0, s, m, dIA, dJA, dA, dParent);
  else if (G == 16) hipLaunchKernelGGL((k_attractors<V, 16>), row_grid(m, 16), dim3(CL_THREADS), 0, s, m, dIA, dJA, dA, dParent);
  else hipLaunchKernelGGL((k_attractors<V, 64>), row_grid(m, 64), dim3(CL_THREADS), 0, s, m, dIA, dJA, dA, dParent);
}

static void launch_hook(hipStream_t s, int G, int m, const int* dIA, const int* dJA, int* f, int* changed) {
  if (G == 4) hipLaunchKernelGGL(k_cc_hook<4>, row_grid(m, 4), dim3(CL_THREADS), 0, s, m, dIA, dJA, f, changed);
  else if (G == 16) hipLaunchKernelGGL(k_cc_hook<16>, row_grid(m, 16), dim3(CL_THREADS), 0, s, m, dIA, dJA, f, changed);
  else hipLaunchKernelGGL(k_cc_hook<64>, row_grid(m, 64), dim3(CL_THREADS), 0, s, m, dIA, dJA, f, changed);
}

static int bad_csr(int hbad, int n, int nnz) {
  if (hbad & BAD_ROWPTR) return fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer ending at nnz=%d", nnz);
  if (hbad & BAD_COLUMN) return fail(SPGEMM_ERR_INPUT, "column outside [0,%d)", n);
  return SPGEMM_OK;
}

template <class V>
static int attractors(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, int* dParent) {
  CHK(check_csr_args(m, n, nnz, dIA, dJA, dA));
  if (m != n) return fail(SPGEMM_ERR_ARG, "the flow matrix is %d x %d, not square", m, n);
  if (m > 0 && !dParent) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  if (m == 0) return SPGEMM_OK;
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int hbad = 0;
  if (int rc = validate_csr(sc, s, m, n, nnz, dIA, dJA, &hbad)) return sc.done(rc);
  if (hbad) return sc.done(bad_csr(hbad, n, nnz));
  launch_attractors<V>(s, lanes_per_row(m, nnz), m, dIA, dJA, dA, dParent);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  return sc.done(SPGEMM_OK);
}

static int components(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, int* dLabel, int* ncomp, int* rounds) {
  if (ncomp) *ncomp = 0;
  if (rounds) *rounds = 0;
  if (m < 0 || n < 0 || nnz < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (m != n) return fail(SPGEMM_ERR_ARG, "the matrix is %d x %d, not square", m, n);
  if ((m > 0 && !dIA) || (nnz > 0 && !dJA)) return fail(SPGEMM_ERR_ARG, "CSR arrays null with m=%d nnz=%d", m, nnz);
  if (m == 0 && nnz > 0) return fail(SPGEMM_ERR_ARG, "nnz=%d in a matrix without rows", nnz);
  if ((m > 0 && !dLabel) || !ncomp) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  if (m == 0) return SPGEMM_OK;
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int hbad = 0;
  if (int rc = validate_csr(sc, s, m, n, nnz, dIA, dJA, &hbad)) return sc.done(rc);
  if (hbad) return sc.done(bad_csr(hbad, n, nnz));
  // {changed, cut short} of every round, the word of a repeated shortcut pass, the root count
  constexpr int CTL_EXTRA = 2 * CC_MAX_ROUNDS, CTL_COUNT = CTL_EXTRA + 1, CTL_INTS = CTL_COUNT + 1;
  int* ctl = nullptr;
  CSR_ALLOC(&ctl, sizeof(int) * CTL_INTS);
  CSR_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * CTL_INTS, s));
  hipLaunchKernelGGL(reorder::k_iota, grid256(m), dim3(256), 0, s, m, dLabel);
  const int G = lanes_per_row(m, nnz);
  int done = 0;
  for (int r = 0; r < CC_MAX_ROUNDS; ++r) {
    launch_hook(s, G, m, dIA, dJA, dLabel, ctl + 2 * r);
    hipLaunchKernelGGL(k_cc_shortcut, grid256(m), dim3(CL_THREADS), 0, s, m, dLabel, ctl + 2 * r + 1);
    CSR_HIP(hipGetLastError());
    int flags[2] = {0, 0};
    CSR_HIP(hipMemcpyAsync(flags, ctl + 2 * r, sizeof(flags), hipMemcpyDeviceToHost, s));
    CSR_HIP(hipStreamSynchronize(s));
    for (int pass = 1; flags[1]; ++pass) {                 // deep chains only: again until every chase has seen its root
      if (pass == CC_MAX_PASSES) return sc.done(fail(SPGEMM_ERR_INTERNAL, "connected components: forest not flat after %d passes", pass));
      CSR_HIP(hipMemsetAsync(ctl + CTL_EXTRA, 0, sizeof(int), s));
      hipLaunchKernelGGL(k_cc_shortcut, grid256(m), dim3(CL_THREADS), 0, s, m, dLabel, ctl + CTL_EXTRA);
      CSR_HIP(hipGetLastError());
      CSR_HIP(hipMemcpyAsync(&flags[1], ctl + CTL_EXTRA, sizeof(int), hipMemcpyDeviceToHost, s));
      CSR_HIP(hipStreamSynchronize(s));
    }
    done = r + 1;
    if (!flags[0]) break;
    if (done == CC_MAX_ROUNDS) return sc.done(fail(SPGEMM_ERR_INTERNAL, "connected components: no fixed point in %d rounds", CC_MAX_ROUNDS));
  }
  hipLaunchKernelGGL(k_count_roots, grid256(m), dim3(CL_THREADS), 0, s, m, dLabel, ctl + CTL_COUNT);
  CSR_HIP(hipGetLastError());
  int count = 0;
  CSR_HIP(hipMemcpyAsync(&count, ctl + CTL_COUNT, sizeof(int), hipMemcpyDeviceToHost, s));
  CSR_HIP(hipStreamSynchronize(s));
  *ncomp = count;
  if (rounds) *rounds = done;
  return sc.done(SPGEMM_OK);
}

static int labels_to_clusters(spgemm_handle* h, int m, const int* dLabel, int* k, int** dCluster, int** dClusterPtr, int** dMembers) {
  if (k) *k = 0;
  if (dCluster) *dCluster = nullptr;
  if (dClusterPtr) *dClusterPtr = nullptr;
  if (dMembers) *dMembers = nullptr;
  if (!k || !dCluster || !dClusterPtr || !dMembers) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  if (m < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (m > 0 && !dLabel) return fail(SPGEMM_ERR_ARG, "labels null with m=%d", m);
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *cluster = nullptr, *ptr = nullptr, *members = nullptr, *idxB = nullptr, *rank = nullptr, *bhist = nullptr;
  unsigned long long *keyA = nullptr, *keyB = nullptr, *tile = nullptr;
  if (m == 0) {
    CSR_ALLOC(&cluster, sizeof(int), true);
    CSR_ALLOC(&ptr, sizeof(int), true);
    CSR_ALLOC(&members, sizeof(int), true);
    CSR_HIP(hipMemsetAsync(ptr, 0, sizeof(int), s));
    CSR_HIP(hipStreamSynchronize(s));
    *dCluster = cluster; *dClusterPtr = ptr; *dMembers = members;
    return sc.done(SPGEMM_OK);
  }
  int* bad = nullptr;
  if (int rc = flag_begin(sc, s, &bad)) return sc.done(rc);
  hipLaunchKernelGGL(k_check_labels, grid256(m), dim3(256), 0, s, m, dLabel, bad);
  int hbad = 0;
  if (int rc = read_flag(s, bad, &hbad)) return sc.done(rc);
  if (hbad) return sc.done(fail(SPGEMM_ERR_INPUT, "labels are not canonical: label[v] <= v and label[label[v]] == label[v]"));
  // rank of every root among the roots = the cluster's number; k = their count
  CSR_ALLOC(&rank, sizeof(int) * ((size_t)m + 1));
  CSR_ALLOC(&tile, scan_scratch_bytes(std::max<long long>((long long)m + 1, (long long)cdiv(m, RS_TILE) * RS_RADIX + 1)));
  hipLaunchKernelGGL(k_is_root, grid256(m), dim3(256), 0, s, m, dLabel, rank);
  unsigned long long total = 0;
  CSR_HIP(scan_total(s, rank, m, tile, &total));
  const int kk = (int)total;                               // 1 <= kk <= m: label[0] == 0 is a root
  const int nblk = cdiv(m, RS_TILE);
  CSR_ALLOC(&cluster, sizeof(int) * (size_t)m, true);
  CSR_ALLOC(&ptr, sizeof(int) * ((size_t)kk + 1), true);
  CSR_ALLOC(&members, sizeof(int) * (size_t)m, true);
  CSR_ALLOC(&idxB, sizeof(int) * (size_t)m);
  CSR_ALLOC(&keyA, sizeof(unsigned long long) * (size_t)m);
  CSR_ALLOC(&keyB, sizeof(unsigned long long) * (size_t)m);
  CSR_ALLOC(&bhist, sizeof(int) * ((size_t)nblk * RS_RADIX + 1));
  hipLaunchKernelGGL(k_cluster_keys, grid256(m), dim3(256), 0, s, m, dLabel, rank, cluster, keyA, members);
  int* idxA = members;
  radix_sort_bits(s, m, 32, 32 + bits_of(kk - 1), keyA, keyB, idxA, idxB, bhist, tile);
  if (idxA != members)                                     // an odd number of passes left the ids in the scratch array
    CSR_HIP(hipMemcpyAsync(members, idxA, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(k_cluster_starts, grid256((long long)kk + 1), dim3(256), 0, s, m, kk, keyA, ptr);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  *k = kk; *dCluster = cluster; *dClusterPtr = ptr; *dMembers = members;
  return sc.done(SPGEMM_OK);
}

template <class V>
static int rmcl_clusters(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, int* k,
                         int** dCluster, int** dClusterPtr, int** dMembers) {
  if (k) *k = 0;
  if (dCluster) *dCluster = nullptr;
  if (dClusterPtr) *dClusterPtr = nullptr;
  if (dMembers) *dMembers = nullptr;
  if (!k || !dCluster || !dClusterPtr || !dMembers) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  CHK(check_csr_args(m, n, nnz, dIA, dJA, dA));
  if (m != n) return fail(SPGEMM_ERR_ARG, "the flow matrix is %d x %d, not square", m, n);
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *parent = nullptr, *rowPtr = nullptr, *label = nullptr;
  CSR_ALLOC(&parent, sizeof(int) * (size_t)std::max(m, 1));
  CSR_ALLOC(&rowPtr, sizeof(int) * ((size_t)m + 1));
  CSR_ALLOC(&label, sizeof(int) * (size_t)std::max(m, 1));
  // the functional graph i -> parent[i] is the CSR (rowPtr = 0..m, columns = parent): one entry per row
  hipLaunchKernelGGL(reorder::k_iota, grid256((long long)m + 1), dim3(256), 0, s, m + 1, rowPtr);
  CSR_HIP(hipGetLastError());
  int ncomp = 0, rounds = 0;
  if (int rc = attractors<V>(h, m, n, nnz, dIA, dJA, dA, parent)) return sc.done(rc);
  if (int rc = components(h, m, m, m, rowPtr, parent, label, &ncomp, &rounds)) return sc.done(rc);
  return sc.done(labels_to_clusters(h, m, label, k, dCluster, dClusterPtr, dMembers));
}

}  // namespace clusters

extern "C" int hip_rmcl_attractor_lanes(int m, int nnz) { return clusters::lanes_per_row(m, nnz); }

extern "C" int hip_rmcl_attractors(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                                   int* dParent) {
  return clusters::attractors<float>(h, m, n, nnz, dIA, dJA, dA, dParent);
}
extern "C" int hip_rmcl_attractors_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                                       int* dParent) {
  return clusters::attractors<double>(h, m, n, nnz, dIA, dJA, dA, dParent);
}

extern "C" int hip_csr_connected_components(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, int* dLabel,
                                            int* ncomp, int* rounds) {
  return clusters::components(h, m, n, nnz, dIA, dJA, dLabel, ncomp, rounds);
}

extern "C" int hip_labels_to_clusters(spgemm_handle* h, int m, const int* dLabel, int* k, int** dCluster, int** dClusterPtr,
                                      int** dMembers) {
  return clusters::labels_to_clusters(h, m, dLabel, k, dCluster, dClusterPtr, dMembers);
}

extern "C" int hip_rmcl_clusters(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA, int* k,
                                 int** dCluster, int** dClusterPtr, int** dMembers) {
  return clusters::rmcl_clusters<float>(h, m, n, nnz, dIA, dJA, dA, k, dCluster, dClusterPtr, dMembers);
}
extern "C" int hip_rmcl_clusters_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                                     int* k, int** dCluster, int** dClusterPtr, int** dMembers) {
  return clusters::rmcl_clusters<double>(h, m, n, nnz, dIA, dJA, dA, k, dCluster, dClusterPtr, dMembers);
}
