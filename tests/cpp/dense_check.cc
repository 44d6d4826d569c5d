// tests/cpp/dense_check.cc — the dense matrix on this project's C++ mirror, on the device.
//   dense_check.x <edge list>
//   (a) the 5 x 6 known answer of the reference's tests/CSR_test.cc:66-78 (tests/golden/dense_kat.json holds the same
//       vectors): the array on the device -> CSR::gpuInitWithDenseMatrix -> the three arrays compared with the expected
//       ones -> gpuDenseMatrix of that CSR is the array again; the host CSR::initWithDenseMatrix on the same array.
//       One line per check ("kat <check>: ok" / "... FAILED").
//   (b) the scenario of correctTests/dense-somp.cc: load, rmclInit, C = gpuSpMMWrapper(A, A); dense(A) * dense(A) through
//       gpuDenseGemm, written back out as a CSR (hip_dense_to_csr, KEEP_ABS, tol 0); both row-sorted; one hip_csr_diff
//       report at the reference's 1e-6 relative.  Prints "Same" or "Diffs".
//   (c) the float product of two seeded random matrices, 70 x 67 x 131, against a host std::fmaf chain over ascending k:
//       "fmaf chain: <n> of <cells> elements differ", and the largest error against a long double product relative to
//       sum_k |a||b|: "max error / sum|a||b| = <x>".
//   "Pass" at the end and exit code 0 iff (a) passed, (b) is Same and (c) has 0 differing elements.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/spgemm_hip.h"
#include "COO.h"
#include "CSR.h"
#include "DenseMatrix.h"
#include "gpus/gpu_csr_kernel.h"
#include "qrmcl.h"

static int failures = 0;

static void check(const char* what, bool ok) {
  printf("kat %s: %s\n", what, ok ? "ok" : "FAILED");
  if (!ok) ++failures;
}

template <class T>
static bool device_equals(const T* d, const std::vector<T>& want) {
  std::vector<T> got(want.size());
  if (!want.empty() && spgemm_hip_memcpy_d2h(got.data(), d, sizeof(T) * want.size())) return false;
  return want.empty() || !memcmp(got.data(), want.data(), sizeof(T) * want.size());
}

static void known_answer() {
  const int rows = 5, cols = 6;
  const std::vector<QValue> dMM = {1, 2, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 4, 0, 0, 0, 5, 0, 0, 0, 0, 2, 0, 3, 0, 0, 1, 0, 8};
  const std::vector<int> rowPtr = {0, 2, 3, 5, 6, 9}, colInd = {0, 1, 2, 1, 5, 4, 0, 3, 5};
  const std::vector<QValue> values = {1, 2, 3, 4, 5, 2, 3, 1, 8};
  DenseMatrix h(rows, cols);
  memcpy(h.values, dMM.data(), sizeof(QValue) * dMM.size());
  DenseMatrix d = h.toGpuDenseMatrix();
  CSR dA = d.toGpuCSR();
  check("shape", dA.rows == rows && dA.cols == cols && dA.nnz == (int)colInd.size());
  check("rowPtr", device_equals(dA.rowPtr, rowPtr));
  check("colInd", device_equals(dA.colInd, colInd));
  check("values", device_equals(dA.values, values));
  DenseMatrix back = DenseMatrix::gpuDenseMatrix(dA);
  check("dense again", device_equals(back.values, dMM));
  CSR hA;
  hA.initWithDenseMatrix(dMM.data(), rows, cols);
  check("host form", hA.nnz == 9 && !memcmp(hA.rowPtr, rowPtr.data(), sizeof(int) * 6) &&
                         !memcmp(hA.colInd, colInd.data(), sizeof(int) * 9) && !memcmp(hA.values, values.data(), sizeof(QValue) * 9));
  DenseMatrix hD(hA);
  check("host dense again", !memcmp(hD.values, dMM.data(), sizeof(QValue) * dMM.size()));
  hD.dispose(); hA.dispose(); back.deviceDispose(); dA.deviceDispose(); d.deviceDispose(); h.dispose();
}

static bool dense_somp(const char* file) {
  COO cooAt;
  cooAt.readSNAPFile(file, true);
  CSR A = rmclInit(cooAt);
  cooAt.dispose();
  CSR dA = A.toGpuCSR();
  CSR dC = gpuSpMMWrapper(dA, dA);
  DenseMatrix dDA = DenseMatrix::gpuDenseMatrix(dA), dDB = DenseMatrix::gpuDenseMatrix(dA);
  DenseMatrix dDC = gpuDenseGemm(dDA, dDB);
  CSR dE = dDC.toGpuCSR(SPGEMM_DENSE_KEEP_ABS, 0.0);
  DenseMatrix::orDie(hip_csr_sort_rows(0, dC.rows, dC.rowPtr, dC.colInd, dC.values), "sort C");
  DenseMatrix::orDie(hip_csr_sort_rows(0, dE.rows, dE.rowPtr, dE.colInd, dE.values), "sort dense C");
  spgemm_csr_diff d;
  DenseMatrix::orDie(hip_csr_diff(0, dC.rows, dC.cols, dC.rowPtr, dC.colInd, dC.values, dC.nnz, dE.rowPtr, dE.colInd, dE.values,
                                  dE.nnz, 1e-6, 0.0, &d), "hip_csr_diff");
  const bool same = d.rows_len_differ == 0 && d.only_a == 0 && d.only_b == 0 && d.beyond == 0;
  printf("m=k=n=%d nnzA=%d nnzC=%d dense nnzC=%d\n", A.rows, A.nnz, dC.nnz, dE.nnz);
  printf("%s\n", same ? "Same" : "Diffs");
  dE.deviceDispose(); dDC.deviceDispose(); dDB.deviceDispose(); dDA.deviceDispose(); dC.deviceDispose(); dA.deviceDispose();
  A.dispose();
  return same;
}

static long fmaf_chain() {
  const int m = 70, n = 67, k = 131;
  std::mt19937 gen(20240607u);
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  DenseMatrix A(m, k), B(k, n);
  for (int i = 0; i < m * k; ++i) A.values[i] = u(gen);
  for (int i = 0; i < k * n; ++i) B.values[i] = u(gen);
  DenseMatrix dA = A.toGpuDenseMatrix(), dB = B.toGpuDenseMatrix();
  DenseMatrix dC = gpuDenseGemm(dA, dB);
  DenseMatrix C = dC.toCpuDenseMatrix();
  long differ = 0;
  long double worst = 0;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) {
      float c = 0.0f;
      long double exact = 0, mag = 0;
      for (int t = 0; t < k; ++t) {
        const float a = A.values[i * k + t], b = B.values[t * n + j];
        c = std::fmaf(a, b, c);
        exact += (long double)a * b;
        mag += fabsl((long double)a * b);
      }
      const float got = C.values[i * n + j];
      if (memcmp(&got, &c, sizeof(float))) ++differ;
      if (mag > 0 && fabsl(got - exact) / mag > worst) worst = fabsl(got - exact) / mag;
    }
  printf("fmaf chain: %ld of %d elements differ\n", differ, m * n);
  printf("max error / sum|a||b| = %.3Le (k * 2^-24 = %.3e)\n", worst, k * 5.9604644775390625e-08);
  C.dispose(); dC.deviceDispose(); dB.deviceDispose(); dA.deviceDispose(); B.dispose(); A.dispose();
  return differ;
}

int main(int argc, char* argv[]) {
  if (argc != 2) { printf("usage: dense_check.x <edge list>\n"); return 2; }
  known_answer();
  const bool same = dense_somp(argv[1]);
  const long differ = fmaf_chain();
  const bool pass = failures == 0 && same && differ == 0;
  printf("%s\n", pass ? "Pass" : "FAILED");
  return pass ? 0 : 1;
}
