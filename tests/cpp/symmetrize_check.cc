// tests/cpp/symmetrize_check.cc — a directed edge list made undirected on the device, through this project's C++ mirror.
//   symmetrize_check.x <edge list>
//   load WITHOUT rmclInit's self loops (readSNAPFile(f, false) + dedupe + toCSR), to the device, gpuSymmetrize(SUM); the
//   result is downloaded and compared, structure and value bits, with a host two-pointer A + A^T written here.  Then the
//   chain a user runs on a directed file: rmclInit's flags (self loops, row-normalise) on the symmetrised graph, two
//   gpuRmclIterDevice steps and gpuRmclClusters, against the clusters the host reads out of the downloaded flow matrix.
//   Prints the counts, then "Same" or the first difference; exit code 0 iff Same.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spgemm_hip.h"
#include "COO.h"
#include "CSR.h"
#include "gpus/gpu_csr_kernel.h"
#include "qrmcl.h"

struct HostCsr {
  std::vector<int> rowPtr, colInd;
  std::vector<QValue> values;
};

// A^T by a counting sort over the columns: rows of the result ascend because A is walked in row order
static HostCsr host_transpose(const CSR& A) {
  HostCsr T;
  T.rowPtr.assign((size_t)A.cols + 1, 0);
  T.colInd.resize((size_t)A.nnz);
  T.values.resize((size_t)A.nnz);
  for (int p = 0; p < A.nnz; ++p) ++T.rowPtr[(size_t)A.colInd[p] + 1];
  for (int c = 0; c < A.cols; ++c) T.rowPtr[(size_t)c + 1] += T.rowPtr[(size_t)c];
  std::vector<int> at(T.rowPtr.begin(), T.rowPtr.end() - 1);
  for (int r = 0; r < A.rows; ++r)
    for (int p = A.rowPtr[r]; p < A.rowPtr[r + 1]; ++p) {
      const int q = at[(size_t)A.colInd[p]]++;
      T.colInd[(size_t)q] = r;
      T.values[(size_t)q] = A.values[p];
    }
  return T;
}

// A + A^T, a two-pointer merge per row; a common column holds 1*a + 1*b
static HostCsr host_sum(const CSR& A) {
  const HostCsr T = host_transpose(A);
  HostCsr S;
  S.rowPtr.assign((size_t)A.rows + 1, 0);
  for (int r = 0; r < A.rows; ++r) {
    int i = A.rowPtr[r], j = T.rowPtr[(size_t)r];
    const int ie = A.rowPtr[r + 1], je = T.rowPtr[(size_t)r + 1];
    while (i < ie || j < je) {
      if (j == je || (i < ie && A.colInd[i] < T.colInd[(size_t)j])) {
        S.colInd.push_back(A.colInd[i]); S.values.push_back(A.values[i]); ++i;
      } else if (i == ie || T.colInd[(size_t)j] < A.colInd[i]) {
        S.colInd.push_back(T.colInd[(size_t)j]); S.values.push_back(T.values[(size_t)j]); ++j;
      } else {
        S.colInd.push_back(A.colInd[i]); S.values.push_back(A.values[i] + T.values[(size_t)j]); ++i; ++j;
      }
    }
    S.rowPtr[(size_t)r + 1] = (int)S.colInd.size();
  }
  return S;
}

// per vertex the number of its cluster: the argmax column of every row (the smaller column on a tie, the row itself when
// nothing wins), a union-find that hangs the larger root under the smaller, clusters numbered by ascending smallest member
static std::vector<int> host_clusters(const CSR& M, int* k) {
  std::vector<int> f((size_t)M.rows);
  for (int i = 0; i < M.rows; ++i) f[(size_t)i] = i;
  const auto find = [&](int x) { while (f[(size_t)x] != x) x = f[(size_t)x]; return x; };
  for (int i = 0; i < M.rows; ++i) {
    QValue bv = -INFINITY;
    int bc = INT_MAX;
    for (int p = M.rowPtr[i]; p < M.rowPtr[i + 1]; ++p)
      if (M.values[p] > bv || (M.values[p] == bv && M.colInd[p] < bc)) { bv = M.values[p]; bc = M.colInd[p]; }
    if (bc == INT_MAX) continue;
    const int a = find(i), b = find(bc);
    if (a != b) f[(size_t)(a > b ? a : b)] = a > b ? b : a;
  }
  std::vector<int> rank((size_t)M.rows), cluster((size_t)M.rows);
  int n = 0;
  for (int v = 0; v < M.rows; ++v) rank[(size_t)v] = find(v) == v ? n++ : -1;
  for (int v = 0; v < M.rows; ++v) cluster[(size_t)v] = rank[(size_t)find(v)];
  *k = n;
  return cluster;
}

int main(int argc, char* argv[]) {
  if (argc != 2) { printf("usage: symmetrize_check.x <edge list>\n"); return 2; }
  COO coo;
  coo.readSNAPFile(argv[1], false);
  coo.orderedAndDuplicatesRemoving();
  CSR A = coo.toCSR();
  coo.dispose();
  CSR dA = A.toGpuCSR();
  CSR dS = gpuSymmetrize(dA, SPGEMM_SYM_SUM);
  CSR S = dS.toCpuCSR();
  const HostCsr want = host_sum(A);
  printf("m=%d nnz(A)=%d nnz(A+A^T)=%d (host %d)\n", A.rows, A.nnz, S.nnz, (int)want.colInd.size());
  bool same = S.rows == A.rows && S.cols == A.cols && S.nnz == (int)want.colInd.size();
  if (!same) printf("shape or nnz differ\n");
  for (int r = 0; same && r <= A.rows; ++r)
    if (S.rowPtr[r] != want.rowPtr[(size_t)r]) { printf("rowPtr[%d]: %d, host %d\n", r, S.rowPtr[r], want.rowPtr[(size_t)r]); same = false; }
  for (int p = 0; same && p < S.nnz; ++p)
    if (S.colInd[p] != want.colInd[(size_t)p] || memcmp(&S.values[p], &want.values[(size_t)p], sizeof(QValue)) != 0) {
      printf("entry %d: (%d, %.9g), host (%d, %.9g)\n", p, S.colInd[p], (double)S.values[p], want.colInd[(size_t)p],
             (double)want.values[(size_t)p]);
      same = false;
    }

  // the chain on the symmetrised graph: its entries as triplets, rmclInit's flags on the device, two steps, the clusters
  COO sym;
  sym.rows = S.rows; sym.cols = S.cols; sym.nnz = S.nnz;
  sym.cooRowIndex = (int*)malloc(sizeof(int) * (size_t)(S.nnz > 0 ? S.nnz : 1));
  sym.cooColIndex = (int*)malloc(sizeof(int) * (size_t)(S.nnz > 0 ? S.nnz : 1));
  sym.cooVal = (QValue*)malloc(sizeof(QValue) * (size_t)(S.nnz > 0 ? S.nnz : 1));
  for (int r = 0; r < S.rows; ++r)
    for (int p = S.rowPtr[r]; p < S.rowPtr[r + 1]; ++p) {
      sym.cooRowIndex[p] = r; sym.cooColIndex[p] = S.colInd[p]; sym.cooVal[p] = S.values[p];
    }
  CSR dMt = sym.toGpuCSR(SPGEMM_COO_SELF_LOOPS | SPGEMM_COO_ROW_NORMALISE);
  CSR dOut = gpuRmclIterDevice(2, dMt, dMt);
  int k = 0, wantK = 0;
  const std::vector<int> cluster = gpuRmclClusters(dOut, &k);
  CSR out = dOut.toCpuCSR();
  const std::vector<int> wantCluster = host_clusters(out, &wantK);
  long differ = k != wantK;
  for (size_t v = 0; v < wantCluster.size(); ++v) differ += cluster[v] != wantCluster[v];
  printf("nnz(Mt)=%d after 2 iterations, clusters=%d (host %d), cluster numbers that differ: %ld\n", out.nnz, k, wantK, differ);
  same = same && differ == 0;
  printf("%s\n", same ? "Same" : "Diffs");
  out.dispose(); dOut.deviceDispose(); dMt.deviceDispose(); sym.dispose();
  S.dispose(); dS.deviceDispose(); dA.deviceDispose(); A.dispose();
  return same ? 0 : 1;
}
