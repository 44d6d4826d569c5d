// Sparse add and the symmetrisation of a directed graph on the device: C = alpha*A + beta*B, diagonal scaling, degree
// counts and factors, and the three published symmetrisations of a directed graph in front of (R-)MCL.
//
// The reference has no counterpart: its loader transposes (readSNAPFile(isTrans), nlibs/COO.h:19) and R-MCL is then run
// on whatever the file held.  The semantics are this library's and are pinned by tests/symmetrize_ref.py.
//
//   hip_csr_add             C = alpha*A + beta*B, the union of two patterns with strictly ascending rows
//   hip_csr_scale           VOut[j] = (rowScale[r] * VA[j]) * colScale[JA[j]]
//   hip_csr_col_counts      entries per column (the in-degree; the out-degree is the row length)
//   hip_degree_factors      count -> count^-exponent, 0 for a count of 0
//   hip_csr_symmetrize      A + A^T, A*A^T + A^T*A, or the degree-discounted form, composed from the calls above and the
//                           library's transpose, product and row sort
//
// hip_csr_add walks ENTRIES, not rows, as hip_csr_diff does: the nnzA + nnzB entries are the work items, A's first and
// then B's, dealt 1024 to a block whatever rows they belong to -- a 20 000-entry hub row is spread over 20 blocks like
// any other 20 000 entries.  An item finds its row by a search in its own rowPtr bounded by the rows of the first and the
// last item its block holds of that matrix, and its partner by a lower bound for its column in the same row of the other
// matrix (first_at_least).
//   pass 1 (k_add_mark)   every item compares its column with [0, n) and with its predecessor's in the row (the flags);
//                         a B item also writes onlyB[j] = 1 when A's row does not hold its column.  Read-only on the
//                         inputs; columns are compared, never used as addresses.
//   scan                  S = exclusive scan of onlyB (nnzB + 1 entries, the library's scan with its 64-bit total);
//                         nnzC = nnzA + S[nnzB];  IC[r] = IA[r] + S[IB[r]].
//   pass 2 (k_add_write)  an A item o of row r, column c, with lb = the lower bound of c in B's row, goes to
//                         IC[r] + (o - IA[r]) + (S[lb] - S[IB[r]]): the entries of A in front of it plus the B-only entries
//                         of the row below c; it adds B[lb] when JB[lb] == c.  A B-only item j (S[j+1] != S[j]) with la =
//                         the lower bound of its column in A's row goes to IC[r] + (la - IA[r]) + (S[j] - S[IB[r]]).
// Every output slot is written by exactly one item, so there is no atomic and no order in which blocks run that could
// show: two calls return the same bits.  The host reads the flags of pass 1 before pass 2 is queued: with both rowPtr
// arrays monotone and every row strictly ascending the positions above stay inside [IC[r], IC[r+1]).
// Values: contraction is off, every operation rounds once: V(alpha)*a + V(beta)*b, V(alpha)*a, V(beta)*b.  An entry whose
// sum is zero stays: the structure depends on the patterns only.
// Uses csr_common_device.hpp (enter, check_csr_args, Scratch, the rowPtr / column checks and their one read-back,
// scan_total, row_of_entry, first_at_least, tile_rows).
#pragma once

namespace symmetrize {

using namespace csrdev;

constexpr int ADD_THREADS = 256, ADD_ITEMS = 4, ADD_TILE = ADD_THREADS * ADD_ITEMS;
static_assert(ADD_TILE == CP_TILE, "k_scale deals its entries with tile_rows, which spans CP_TILE entries");
enum { BAD_ORDER = 64 };

// rows of the tile's first / last A item (rows[0], rows[1]) and first / last B item (rows[2], rows[3]); items are A's
// entries, then B's
__device__ __forceinline__ void pair_tile_rows(int m, int nnzA, const int* __restrict__ IA, const int* __restrict__ IB,
                                               long long base, long long end, int (&rows)[4]) {
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
}

// pass 1: the flags of both operands and onlyB.  With nnzB == 0 it is the check of one matrix (IB, JB, onlyB unused).
__global__ __launch_bounds__(ADD_THREADS) void k_add_mark(int m, int n, int nnzA, int nnzB, const int* __restrict__ IA,
                                                          const int* __restrict__ JA, const int* __restrict__ IB,
                                                          const int* __restrict__ JB, int* __restrict__ onlyB,
                                                          int* __restrict__ bad) {
  __shared__ int rows[4];
  const long long total = (long long)nnzA + nnzB;
  const long long base = (long long)blockIdx.x * ADD_TILE;
  const long long end = base + ADD_TILE < total ? base + ADD_TILE : total;
  pair_tile_rows(m, nnzA, IA, IB, base, end, rows);
  int flags = 0;
#pragma unroll
  for (int k = 0; k < ADD_ITEMS; ++k) {
    const long long g = base + k * ADD_THREADS + threadIdx.x;
    if (g >= total) break;
    const bool isA = g < nnzA;
    const int o = (int)(isA ? g : g - nnzA);
    const int* __restrict__ IX = isA ? IA : IB;
    const int* __restrict__ JX = isA ? JA : JB;
    const int r = row_of_entry(IX, rows[isA ? 0 : 2], rows[isA ? 1 : 3], o);
    const int c = JX[o];
    if ((unsigned)c >= (unsigned)n) flags |= BAD_COLUMN;
    if (o > IX[r] && JX[o - 1] >= c) flags |= BAD_ORDER;
    if (!isA) {
      const int ae = IA[r + 1];
      const int la = first_at_least(JA, IA[r], ae, c);
      onlyB[o] = !(la < ae && JA[la] == c);
    }
  }
  if (flags) atomicOr(bad, flags);
}

__global__ void k_add_rowptr(int m, const int* __restrict__ IA, const int* __restrict__ IB, const int* __restrict__ S,
                             int* __restrict__ IC) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r <= m) IC[r] = IA[r] + S[IB[r]];
}

// pass 2: every item writes the one output slot that is its own (see the head of the file)
template <class V>
__global__ __launch_bounds__(ADD_THREADS) void k_add_write(int m, int nnzA, int nnzB, V alpha, V beta,
                                                           const int* __restrict__ IA, const int* __restrict__ JA,
                                                           const V* __restrict__ A, const int* __restrict__ IB,
                                                           const int* __restrict__ JB, const V* __restrict__ B,
                                                           const int* __restrict__ S, const int* __restrict__ IC,
                                                           int* __restrict__ JC, V* __restrict__ C) {
#pragma clang fp contract(off)                              // one rounding per operation, as the host restates it
  __shared__ int rows[4];
  const long long total = (long long)nnzA + nnzB;
  const long long base = (long long)blockIdx.x * ADD_TILE;
  const long long end = base + ADD_TILE < total ? base + ADD_TILE : total;
  pair_tile_rows(m, nnzA, IA, IB, base, end, rows);
#pragma unroll
  for (int k = 0; k < ADD_ITEMS; ++k) {
    const long long g = base + k * ADD_THREADS + threadIdx.x;
    if (g >= total) break;
    if (g < nnzA) {
      const int o = (int)g;
      const int r = row_of_entry(IA, rows[0], rows[1], o);
      const int c = JA[o];
      const int b0 = IB[r], be = IB[r + 1];
      const int lb = first_at_least(JB, b0, be, c);
      const int dst = IC[r] + (o - IA[r]) + (S[lb] - S[b0]);
      V v = alpha * A[o];
      if (lb < be && JB[lb] == c) v = v + beta * B[lb];
      JC[dst] = c;
      C[dst] = v;
    } else {
      const int j = (int)(g - nnzA);
      if (S[j + 1] == S[j]) continue;                       // a common column: A's item writes it
      const int r = row_of_entry(IB, rows[2], rows[3], j);
      const int c = JB[j];
      const int a0 = IA[r];
      const int la = first_at_least(JA, a0, IA[r + 1], c);
      const int dst = IC[r] + (la - a0) + (S[j] - S[IB[r]]);
      JC[dst] = c;
      C[dst] = beta * B[j];
    }
  }
}

// VOut[j] = (rowScale[r] * VA[j]) * colScale[JA[j]]; VOut may be VA (an item reads its own entry before it writes it)
template <class V>
__global__ __launch_bounds__(CP_THREADS) void k_scale(int m, int nnz, const int* __restrict__ IA, const int* __restrict__ JA,
                                                      const V* VA, const V* __restrict__ rowScale,
                                                      const V* __restrict__ colScale, V* VOut) {
  __shared__ int rows[2];
  const long long base = (long long)blockIdx.x * CP_TILE;
  if (rowScale) tile_rows(IA, m, nnz, base, rows);
#pragma unroll
  for (int k = 0; k < CP_ITEMS; ++k) {
    const long long o = base + k * CP_THREADS + threadIdx.x;
    if (o >= nnz) break;
    V v = VA[o];
    if (rowScale) v = rowScale[row_of_entry(IA, rows[0], rows[1], (int)o)] * v;
    if (colScale) v = v * colScale[JA[o]];
    VOut[o] = v;
  }
}

// integer atomics: the counts are the same on every call
__global__ void k_col_counts(int nnz, const int* __restrict__ JA, int* __restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nnz) atomicAdd(&count[JA[i]], 1);
}

template <class V>
__global__ void k_degree_factors(int len, const int* __restrict__ count, double exponent, V* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= len) return;
  const int c = count[i];
  out[i] = c > 0 ? (V)pow((double)c, -exponent) : (V)0;
}

static int bad_operand(const char* who, int hbad, int n, int nnz) {
  if (hbad & BAD_ROWPTR) return fail(SPGEMM_ERR_INPUT, "%srowPtr is not a monotone row pointer ending at nnz (nnz=%d)", who, nnz);
  if (hbad & BAD_COLUMN) return fail(SPGEMM_ERR_INPUT, "%scolumn outside [0,%d)", who, n);
  if (hbad & BAD_ORDER) return fail(SPGEMM_ERR_INPUT, "%sa row is not strictly ascending by column (sort the rows first: hip_csr_sort_rows)", who);
  return SPGEMM_OK;
}

template <class V>
static int add(spgemm_handle* h, int m, int n, double alpha, const int* dIA, const int* dJA, const V* dA, int nnzA,
               double beta, const int* dIB, const int* dJB, const V* dB, int nnzB, int** dIC, int** dJC, V** dC, int* nnzC) {
  if (dIC) *dIC = nullptr;
  if (dJC) *dJC = nullptr;
  if (dC) *dC = nullptr;
  if (nnzC) *nnzC = 0;
  if (!dIC || !dJC || !dC || !nnzC) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  CHK(check_csr_args(m, n, nnzA, dIA, dJA, dA));
  CHK(check_csr_args(m, n, nnzB, dIB, dJB, dB));
  if (alpha != alpha || beta != beta) return fail(SPGEMM_ERR_ARG, "alpha / beta is not a number");
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int *bad = nullptr, *S = nullptr, *IC = nullptr, *JC = nullptr;
  V* C = nullptr;
  unsigned long long* tile = nullptr;
  // (1) both rowPtr arrays, read back before the walk forms addresses from them
  if (int rc = flag_begin(sc, s, &bad)) return sc.done(rc);
  queue_csr_checks(s, m, n, nnzA, dIA, nullptr, bad);
  queue_csr_checks(s, m, n, nnzB, dIB, nullptr, bad);
  int hbad = 0;
  if (int rc = read_flag(s, bad, &hbad)) return sc.done(rc);
  if (hbad) return sc.done(fail(SPGEMM_ERR_INPUT, "rowPtr is not a monotone row pointer ending at nnz (nnzA=%d nnzB=%d)", nnzA, nnzB));
  const long long total = (long long)nnzA + nnzB;
  const unsigned nblk = (unsigned)std::max(1, cdiv(total, ADD_TILE));
  // (2) pass 1 and the scan; the flags and the total come back before anything is placed
  CSR_ALLOC(&S, sizeof(int) * ((size_t)nnzB + 1));
  CSR_ALLOC(&tile, scan_scratch_bytes((long long)nnzB + 1));
  if (total > 0)
    hipLaunchKernelGGL(k_add_mark, dim3(nblk), dim3(ADD_THREADS), 0, s, m, n, nnzA, nnzB, dIA, dJA, dIB, dJB, S, bad);
  CSR_HIP(hipGetLastError());
  unsigned long long onlyB = 0;
  CSR_HIP(scan_total(s, S, nnzB, tile, &onlyB));
  if (int rc = read_flag(s, bad, &hbad)) return sc.done(rc);
  if (hbad) return sc.done(bad_operand("", hbad, n, 0));
  const unsigned long long nnz64 = (unsigned long long)nnzA + onlyB;
  if (nnz64 > (unsigned long long)INT_MAX)
    return sc.done(fail(SPGEMM_ERR_OVERFLOW, "nnz(C) = %llu does not fit int32", nnz64));
  const int nc = (int)nnz64;
  // (3) the row pointer and pass 2
  CSR_ALLOC(&IC, sizeof(int) * ((size_t)m + 1), true);
  CSR_ALLOC(&JC, sizeof(int) * (size_t)std::max(nc, 1), true);
  CSR_ALLOC(&C, sizeof(V) * (size_t)std::max(nc, 1), true);
  if (m == 0) {
    CSR_HIP(hipMemsetAsync(IC, 0, sizeof(int), s));
  } else {
    hipLaunchKernelGGL(k_add_rowptr, grid256((long long)m + 1), dim3(256), 0, s, m, dIA, dIB, S, IC);
    if (total > 0)
      hipLaunchKernelGGL(k_add_write<V>, dim3(nblk), dim3(ADD_THREADS), 0, s, m, nnzA, nnzB, (V)alpha, (V)beta, dIA, dJA, dA,
                         dIB, dJB, dB, S, IC, JC, C);
  }
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  *dIC = IC; *dJC = JC; *dC = C; *nnzC = nc;
  return sc.done(SPGEMM_OK);
}

template <class V>
static int scale(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const V* dA, const V* dRowScale,
                 const V* dColScale, V* dOut) {
  CHK(check_csr_args(m, n, nnz, dIA, dJA, dA));
  if (nnz > 0 && !dOut) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  if (nnz == 0) return SPGEMM_OK;
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int hbad = 0;
  if (int rc = validate_csr(sc, s, m, n, nnz, dIA, dColScale ? dJA : nullptr, &hbad)) return sc.done(rc);
  if (hbad) return sc.done(bad_operand("", hbad, n, nnz));
  hipLaunchKernelGGL(k_scale<V>, dim3((unsigned)cdiv(nnz, CP_TILE)), dim3(CP_THREADS), 0, s, m, nnz, dIA, dJA, dA, dRowScale,
                     dColScale, dOut);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  return sc.done(SPGEMM_OK);
}

static int col_counts(spgemm_handle* h, int n, int nnz, const int* dJA, int* dCount) {
  if (n < 0 || nnz < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (nnz > 0 && !dJA) return fail(SPGEMM_ERR_ARG, "columns null with nnz=%d", nnz);
  if (n > 0 && !dCount) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  if (n == 0 && nnz == 0) return SPGEMM_OK;
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  int hbad = 0;
  if (int rc = validate_csr(sc, s, 0, n, nnz, nullptr, dJA, &hbad)) return sc.done(rc);
  if (hbad) return sc.done(bad_operand("", hbad, n, nnz));
  if (n > 0) CSR_HIP(hipMemsetAsync(dCount, 0, sizeof(int) * (size_t)n, s));
  if (nnz > 0) hipLaunchKernelGGL(k_col_counts, grid256(nnz), dim3(256), 0, s, nnz, dJA, dCount);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  return sc.done(SPGEMM_OK);
}

template <class V>
static int degree_factors(spgemm_handle* h, int len, const int* dCount, double exponent, V* dOut) {
  if (len < 0) return fail(SPGEMM_ERR_ARG, "negative size");
  if (len > 0 && (!dCount || !dOut)) return fail(SPGEMM_ERR_ARG, "arrays null with len=%d", len);
  if (exponent != exponent) return fail(SPGEMM_ERR_ARG, "the exponent is not a number");
  if (len == 0) return SPGEMM_OK;
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  hipLaunchKernelGGL(k_degree_factors<V>, grid256(len), dim3(256), 0, s, len, dCount, exponent, dOut);
  CSR_HIP(hipGetLastError());
  CSR_HIP(hipStreamSynchronize(s));
  return sc.done(SPGEMM_OK);
}

static int product(spgemm_handle* h, const int* IA, const int* JA, const float* A, int nnzA, const int* IB, const int* JB,
                   const float* B, int nnzB, int m, int k, int n, int** IC, int** JC, float** C, int* nnzC) {
  return hip_gpuSpMM(h, IA, JA, A, nnzA, IB, JB, B, nnzB, m, k, n, IC, JC, C, nnzC);
}
static int product(spgemm_handle* h, const int* IA, const int* JA, const double* A, int nnzA, const int* IB, const int* JB,
                   const double* B, int nnzB, int m, int k, int n, int** IC, int** JC, double** C, int* nnzC) {
  return hip_gpuSpMM_f64(h, IA, JA, A, nnzA, IB, JB, B, nnzB, m, k, n, IC, JC, C, nnzC);
}

// a CSR that one of the library's calls handed out; its arrays go back to the pool with the Scratch they are kept in
template <class V>
struct Made {
  int *I = nullptr, *J = nullptr;
  V* X = nullptr;
  int nnz = 0;
  void keep(Scratch& sc) { for (void* p : {(void*)I, (void*)J, (void*)X}) if (p) sc.tmp.push_back(p); }
};

// P = X * Y (m x m) with its rows sorted by column, kept in sc
template <class V>
static int sorted_product(spgemm_handle* h, Scratch& sc, int m, const int* IX, const int* JX, const V* X, int nnzX,
                          const int* IY, const int* JY, const V* Y, int nnzY, Made<V>& P) {
  const int rc = product(h, IX, JX, X, nnzX, IY, JY, Y, nnzY, m, m, m, &P.I, &P.J, &P.X, &P.nnz);
  P.keep(sc);
  if (rc) return rc;
  return sort_rows<V>(h, m, P.I, P.J, P.X);
}

template <class V>
static int symmetrize(spgemm_handle* h, int mode, double alpha, double beta, int m, const int* dIA, const int* dJA, const V* dA,
                      int nnz, int** dIS, int** dJS, V** dS, int* nnzS) {
  if (dIS) *dIS = nullptr;
  if (dJS) *dJS = nullptr;
  if (dS) *dS = nullptr;
  if (nnzS) *nnzS = 0;
  if (!dIS || !dJS || !dS || !nnzS) return fail(SPGEMM_ERR_ARG, "output pointer is null");
  if (mode != SPGEMM_SYM_SUM && mode != SPGEMM_SYM_BIBLIOMETRIC && mode != SPGEMM_SYM_DEGREE_DISCOUNTED)
    return fail(SPGEMM_ERR_ARG, "unknown symmetrisation mode %d", mode);
  CHK(check_csr_args(m, m, nnz, dIA, dJA, dA));
  if (mode == SPGEMM_SYM_DEGREE_DISCOUNTED && (alpha != alpha || beta != beta))
    return fail(SPGEMM_ERR_ARG, "alpha / beta is not a number");
  hipStream_t s;
  CHK(enter(h, &s));
  Scratch sc;
  // (1) A itself: rowPtr, then the column range and the order of every row (pass 1 of the add on A alone), read back
  //     before any of the calls below indexes with a value of A
  int* bad = nullptr;
  int hbad = 0;
  if (int rc = flag_begin(sc, s, &bad)) return sc.done(rc);
  queue_csr_checks(s, m, m, nnz, dIA, nullptr, bad);
  if (int rc = read_flag(s, bad, &hbad)) return sc.done(rc);
  if (hbad) return sc.done(bad_operand("", hbad, m, nnz));
  if (nnz > 0) {
    hipLaunchKernelGGL(k_add_mark, dim3((unsigned)cdiv(nnz, ADD_TILE)), dim3(ADD_THREADS), 0, s, m, m, nnz, 0, dIA, dJA,
                       (const int*)nullptr, (const int*)nullptr, (int*)nullptr, bad);
    CSR_HIP(hipGetLastError());
    if (int rc = read_flag(s, bad, &hbad)) return sc.done(rc);
    if (hbad) return sc.done(bad_operand("", hbad, m, nnz));
  }
  Made<V> T, P1, P2;
  if (mode == SPGEMM_SYM_SUM) {
    int rc = reorder::transpose<V>(h, m, m, nnz, dIA, dJA, dA, &T.I, &T.J, &T.X);
    T.keep(sc);
    if (rc) return sc.done(rc);
    return sc.done(add<V>(h, m, m, 1.0, dIA, dJA, dA, nnz, 1.0, T.I, T.J, T.X, nnz, dIS, dJS, dS, nnzS));
  }
  if (mode == SPGEMM_SYM_BIBLIOMETRIC) {
    int rc = reorder::transpose<V>(h, m, m, nnz, dIA, dJA, dA, &T.I, &T.J, &T.X);
    T.keep(sc);
    if (rc) return sc.done(rc);
    if ((rc = sorted_product<V>(h, sc, m, dIA, dJA, dA, nnz, T.I, T.J, T.X, nnz, P1))) return sc.done(rc);
    if ((rc = sorted_product<V>(h, sc, m, T.I, T.J, T.X, nnz, dIA, dJA, dA, nnz, P2))) return sc.done(rc);
    return sc.done(add<V>(h, m, m, 1.0, P1.I, P1.J, P1.X, P1.nnz, 1.0, P2.I, P2.J, P2.X, P2.nnz, dIS, dJS, dS, nnzS));
  }
  // degree-discounted: Y * Y^T + Z^T * Z with Y = Do^-alpha A Di^(-beta/2), Z = Do^(-alpha/2) A Di^-beta
  int *dOut = nullptr, *dIn = nullptr;
  V *fo = nullptr, *foHalf = nullptr, *fi = nullptr, *fiHalf = nullptr, *Y = nullptr, *Z = nullptr;
  const size_t mm = (size_t)std::max(m, 1), ne = (size_t)std::max(nnz, 1);
  CSR_ALLOC(&dOut, sizeof(int) * mm);
  CSR_ALLOC(&dIn, sizeof(int) * mm);
  CSR_ALLOC(&fo, sizeof(V) * mm);
  CSR_ALLOC(&foHalf, sizeof(V) * mm);
  CSR_ALLOC(&fi, sizeof(V) * mm);
  CSR_ALLOC(&fiHalf, sizeof(V) * mm);
  CSR_ALLOC(&Y, sizeof(V) * ne);
  CSR_ALLOC(&Z, sizeof(V) * ne);
  if (m > 0) hipLaunchKernelGGL(reorder::k_gather_lens, grid256(m), dim3(256), 0, s, m, dIA, (const int*)nullptr, dOut);
  CSR_HIP(hipGetLastError());
  int rc = col_counts(h, m, nnz, dJA, dIn);
  if (!rc) rc = degree_factors<V>(h, m, dOut, alpha, fo);
  if (!rc) rc = degree_factors<V>(h, m, dOut, alpha * 0.5, foHalf);
  if (!rc) rc = degree_factors<V>(h, m, dIn, beta, fi);
  if (!rc) rc = degree_factors<V>(h, m, dIn, beta * 0.5, fiHalf);
  if (!rc) rc = scale<V>(h, m, m, nnz, dIA, dJA, dA, fo, fiHalf, Y);
  if (!rc) rc = scale<V>(h, m, m, nnz, dIA, dJA, dA, foHalf, fi, Z);
  if (rc) return sc.done(rc);
  Made<V> YT, ZT;
  rc = reorder::transpose<V>(h, m, m, nnz, dIA, dJA, Y, &YT.I, &YT.J, &YT.X);
  YT.keep(sc);
  if (rc) return sc.done(rc);
  rc = reorder::transpose<V>(h, m, m, nnz, dIA, dJA, Z, &ZT.I, &ZT.J, &ZT.X);
  ZT.keep(sc);
  if (rc) return sc.done(rc);
  if ((rc = sorted_product<V>(h, sc, m, dIA, dJA, Y, nnz, YT.I, YT.J, YT.X, nnz, P1))) return sc.done(rc);
  if ((rc = sorted_product<V>(h, sc, m, ZT.I, ZT.J, ZT.X, nnz, dIA, dJA, Z, nnz, P2))) return sc.done(rc);
  return sc.done(add<V>(h, m, m, 1.0, P1.I, P1.J, P1.X, P1.nnz, 1.0, P2.I, P2.J, P2.X, P2.nnz, dIS, dJS, dS, nnzS));
}

}  // namespace symmetrize

extern "C" int hip_csr_add(spgemm_handle* h, int m, int n, double alpha, const int* dIA, const int* dJA, const float* dA,
                           int nnzA, double beta, const int* dIB, const int* dJB, const float* dB, int nnzB, int** dIC,
                           int** dJC, float** dC, int* nnzC) {
  return symmetrize::add<float>(h, m, n, alpha, dIA, dJA, dA, nnzA, beta, dIB, dJB, dB, nnzB, dIC, dJC, dC, nnzC);
}
extern "C" int hip_csr_add_f64(spgemm_handle* h, int m, int n, double alpha, const int* dIA, const int* dJA, const double* dA,
                               int nnzA, double beta, const int* dIB, const int* dJB, const double* dB, int nnzB, int** dIC,
                               int** dJC, double** dC, int* nnzC) {
  return symmetrize::add<double>(h, m, n, alpha, dIA, dJA, dA, nnzA, beta, dIB, dJB, dB, nnzB, dIC, dJC, dC, nnzC);
}

extern "C" int hip_csr_scale(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const float* dA,
                             const float* dRowScale, const float* dColScale, float* dOut) {
  return symmetrize::scale<float>(h, m, n, nnz, dIA, dJA, dA, dRowScale, dColScale, dOut);
}
extern "C" int hip_csr_scale_f64(spgemm_handle* h, int m, int n, int nnz, const int* dIA, const int* dJA, const double* dA,
                                 const double* dRowScale, const double* dColScale, double* dOut) {
  return symmetrize::scale<double>(h, m, n, nnz, dIA, dJA, dA, dRowScale, dColScale, dOut);
}

extern "C" int hip_csr_col_counts(spgemm_handle* h, int n, int nnz, const int* dJA, int* dCount) {
  return symmetrize::col_counts(h, n, nnz, dJA, dCount);
}

extern "C" int hip_degree_factors(spgemm_handle* h, int len, const int* dCount, double exponent, float* dOut) {
  return symmetrize::degree_factors<float>(h, len, dCount, exponent, dOut);
}
extern "C" int hip_degree_factors_f64(spgemm_handle* h, int len, const int* dCount, double exponent, double* dOut) {
  return symmetrize::degree_factors<double>(h, len, dCount, exponent, dOut);
}

extern "C" int hip_csr_symmetrize(spgemm_handle* h, int mode, double alpha, double beta, int m, const int* dIA, const int* dJA,
                                  const float* dA, int nnz, int** dIS, int** dJS, float** dS, int* nnzS) {
  return symmetrize::symmetrize<float>(h, mode, alpha, beta, m, dIA, dJA, dA, nnz, dIS, dJS, dS, nnzS);
}
extern "C" int hip_csr_symmetrize_f64(spgemm_handle* h, int mode, double alpha, double beta, int m, const int* dIA,
                                      const int* dJA, const double* dA, int nnz, int** dIS, int** dJS, double** dS, int* nnzS) {
  return symmetrize::symmetrize<double>(h, mode, alpha, beta, m, dIA, dJA, dA, nnz, dIS, dJS, dS, nnzS);
}
