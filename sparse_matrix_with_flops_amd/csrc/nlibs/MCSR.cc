// MCSR.cc — see MCSR.h.  Host-side glue only; the split and the concatenation run in libspgemm_hip.so.
#include "MCSR.h"
#include "../../../include/spgemm_hip.h"

#include <cstdio>
#include <cstdlib>

static void mcsr_or_die(int rc, const char* what) {
  if (rc != SPGEMM_OK) { printf("%s: %s\n", what, spgemm_hip_last_error()); exit(EXIT_FAILURE); }
}

MCSR::MCSR(const CSR& dcsr, const int r, const int c, const int blockRows, const int blockCols)
    : CSR(), BCSR(blockRows, blockCols, r, c) {
  rows = dcsr.rows;
  cols = dcsr.cols;
  mcsr_or_die(hip_csr_to_mcsr(0, dcsr.rows, dcsr.cols, dcsr.nnz, dcsr.rowPtr, dcsr.colInd, dcsr.values, r, c, blockRows,
                              blockCols, &(BCSR::rowPtr), &(BCSR::colInd), &(BCSR::values), &nnzb, &(CSR::rowPtr),
                              &(CSR::colInd), &(CSR::values), &(CSR::nnz)), "MCSR");
  BCSR::nnz = dcsr.nnz - CSR::nnz;
}

void MCSR::dispose() {
  BCSR::dispose();
  CSR::deviceDispose();
}

CSR MCSR::toCSR(double drop_tol) const {
  CSR dC;
  mcsr_or_die(hip_mcsr_to_csr(0, rows, cols, r, c, m, n, nnzb, BCSR::rowPtr, BCSR::colInd, BCSR::values, CSR::nnz,
                              CSR::rowPtr, CSR::colInd, CSR::values, drop_tol, &dC.rowPtr, &dC.colInd, &dC.values, &dC.nnz),
              "MCSR::toCSR");
  dC.rows = rows;
  dC.cols = cols;
  return dC;
}
