// tests/cpp/topk_check.cc — selection through this project's C++ mirror, on the device.
//   topk_check.x <edge list>
//   load, rmclInit, to the device, one product Mt * Mt there (gpuSpMMWrapper), then CSR::gpuRowTopK on it for k = 1, 3 and
//   64.  The product is downloaded once and the same selection is made on the host: per row a std::stable_sort of the
//   positions under the library's order (larger value, then smaller column; the stable sort keeps the earlier position
//   first; NaN last), the first k of them back in storage order.  The device and the host see the same input bits, so
//   rowPtr, colInd and the value bits must be identical.  Prints the counts, then "Same" or "Diffs"; exit code 0 iff Same.
#include <algorithm>
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

// a before b in the library's order, positions apart (a NaN ranks below every number; -0.0 == +0.0)
static bool beats(QValue va, int ca, QValue vb, int cb) {
  const bool na = std::isnan(va), nb = std::isnan(vb);
  if (na != nb) return nb;
  if (!na && va != vb) return va > vb;
  return ca < cb;
}

static long host_differences(const CSR& X, const CSR& got, int k) {
  long differ = 0;
  int out = 0;
  std::vector<int> pos;
  for (int r = 0; r < X.rows; ++r) {
    const int a = X.rowPtr[r], len = X.rowPtr[r + 1] - a;
    pos.resize((size_t)len);
    for (int i = 0; i < len; ++i) pos[(size_t)i] = i;
    if (len > k) {
      std::stable_sort(pos.begin(), pos.end(), [&](int x, int y) {
        return beats(X.values[a + x], X.colInd[a + x], X.values[a + y], X.colInd[a + y]);
      });
      pos.resize((size_t)k);
      std::sort(pos.begin(), pos.end());
    }
    differ += got.rowPtr[r] != out;
    for (int p : pos) {
      if (out < got.nnz)
        differ += got.colInd[out] != X.colInd[a + p] || memcmp(&got.values[out], &X.values[a + p], sizeof(QValue)) != 0;
      ++out;
    }
  }
  return differ + (got.rowPtr[X.rows] != out) + (got.nnz != out);
}

int main(int argc, char* argv[]) {
  if (argc != 2) { printf("usage: topk_check.x <edge list>\n"); return 2; }
  COO cooAt;
  cooAt.readSNAPFile(argv[1], true);
  CSR Mt = rmclInit(cooAt);
  cooAt.dispose();
  CSR dMt = Mt.toGpuCSR();
  CSR dX = gpuSpMMWrapper(dMt, dMt);
  CSR X = dX.toCpuCSR();
  int longest = 0;
  for (int r = 0; r < X.rows; ++r) longest = std::max(longest, X.rowPtr[r + 1] - X.rowPtr[r]);
  printf("m=%d nnz(Mt)=%d nnz(Mt*Mt)=%d longest row=%d\n", X.rows, Mt.nnz, X.nnz, longest);
  long differ = 0;
  for (int k : {1, 3, 64}) {
    CSR dN = dX.gpuRowTopK(k);
    CSR N = dN.toCpuCSR();
    const long d = host_differences(X, N, k);
    printf("k=%d: nnz %d, differences %ld\n", k, N.nnz, d);
    differ += d;
    N.dispose();
    dN.deviceDispose();
  }
  printf("%s\n", differ == 0 ? "Same" : "Diffs");
  X.dispose(); dX.deviceDispose(); dMt.deviceDispose(); Mt.dispose();
  return differ == 0 ? 0 : 1;
}
