// DenseMatrix.h — mirror of the reference's `struct DenseMatrix` (nlibs/DenseMatrix.h): rows x cols values, row-major, no
// padding.  The host form is the reference's (malloc in place of mkl_malloc).  The device form holds a device array in
// the SAME struct, as CSR does after toGpuCSR(): gpuDenseMatrix(dA) is the constructor on a device CSR
// (hip_csr_to_dense), gpuDenseGemm the cblas_dgemm call of correctTests/dense-somp.cc (alpha 1, beta 0, no transposes:
// hip_dense_gemm), toGpuCSR CSR::initWithDenseMatrix on the device (hip_dense_to_csr).  The work is done by
// libspgemm_hip.so (include/spgemm_hip.h, "dense matrix").  Header-only; every device call exits on error.
#ifndef SMF_DENSEMATRIX_H_
#define SMF_DENSEMATRIX_H_
#include <cstdio>
#include <cstdlib>

#include "../../../include/spgemm_hip.h"
#include "CSR.h"

struct DenseMatrix {
  QValue* values;
  int rows, cols;

  DenseMatrix() : values(0), rows(0), cols(0) {}
  // nlibs/DenseMatrix.h:6-21 on a host CSR: zero-fill, then every entry in storage order
  DenseMatrix(const CSR& csr) : rows(csr.rows), cols(csr.cols) {
    values = (QValue*)calloc((size_t)rows * cols + 1, sizeof(QValue));
    for (int i = 0; i < rows; i++)
      for (int j = csr.rowPtr[i]; j < csr.rowPtr[i + 1]; j++) values[(size_t)i * cols + csr.colInd[j]] = csr.values[j];
  }
  // nlibs/DenseMatrix.h:23-30: all zero
  DenseMatrix(const int irows, const int icols) : rows(irows), cols(icols) {
    values = (QValue*)calloc((size_t)rows * cols + 1, sizeof(QValue));
  }
  void dispose() { free(values); values = 0; }

  // ---- the device form ----
  static void orDie(int rc, const char* what) {
    if (rc != SPGEMM_OK) { printf("%s: %s\n", what, spgemm_hip_last_error()); exit(EXIT_FAILURE); }
  }
  static DenseMatrix gpuAlloc(int rows, int cols) {
    DenseMatrix d;
    d.rows = rows; d.cols = cols;
    orDie(spgemm_hip_malloc((void**)&d.values, sizeof(QValue) * ((size_t)rows * cols + 1)), "DenseMatrix (device)");
    return d;
  }
  // DenseMatrix(const CSR&) on a device CSR (after toGpuCSR)
  static DenseMatrix gpuDenseMatrix(const CSR& dA) {
    DenseMatrix d = gpuAlloc(dA.rows, dA.cols);
    orDie(hip_csr_to_dense(0, dA.rows, dA.cols, dA.nnz, dA.rowPtr, dA.colInd, dA.values, d.values, dA.cols), "gpuDenseMatrix");
    return d;
  }
  DenseMatrix toGpuDenseMatrix() const {
    DenseMatrix d = gpuAlloc(rows, cols);
    if ((size_t)rows * cols) orDie(spgemm_hip_memcpy_h2d(d.values, values, sizeof(QValue) * (size_t)rows * cols), "toGpuDenseMatrix");
    return d;
  }
  DenseMatrix toCpuDenseMatrix() const {
    DenseMatrix h(rows, cols);
    if ((size_t)rows * cols) orDie(spgemm_hip_memcpy_d2h(h.values, values, sizeof(QValue) * (size_t)rows * cols), "toCpuDenseMatrix");
    return h;
  }
  // device CSR of the kept cells; the defaults are CSR::initWithDenseMatrix's rule
  CSR toGpuCSR(int rule = SPGEMM_DENSE_KEEP_REFERENCE, double tol = 1e-8) const {
    return CSR::gpuInitWithDenseMatrix(values, rows, cols, rule, tol);
  }
  void deviceDispose() { spgemm_hip_free(values); values = 0; }
};

// dC = dA * dB on device matrices, a new device matrix
inline DenseMatrix gpuDenseGemm(const DenseMatrix& dA, const DenseMatrix& dB) {
  if (dA.cols != dB.rows) { printf("gpuDenseGemm: shape mismatch\n"); exit(EXIT_FAILURE); }
  DenseMatrix dC = DenseMatrix::gpuAlloc(dA.rows, dB.cols);
  DenseMatrix::orDie(hip_dense_gemm(0, dA.rows, dB.cols, dA.cols, dA.values, dA.cols, dB.values, dB.cols, dC.values, dB.cols),
                     "gpuDenseGemm");
  return dC;
}
#endif
