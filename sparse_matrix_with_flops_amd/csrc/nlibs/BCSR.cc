// BCSR.cc — see BCSR.h.  Host-side glue only; the tiling and the row walk run in libspgemm_hip.so.
#include "BCSR.h"
#include "../../../include/spgemm_hip.h"

#include <cstdio>
#include <cstdlib>

static void bcsr_or_die(int rc, const char* what) {
  if (rc != SPGEMM_OK) { printf("%s: %s\n", what, spgemm_hip_last_error()); exit(EXIT_FAILURE); }
}

static int blocks_of(int len, int tile) { return tile > 0 ? (int)(((long long)len + tile - 1) / tile) : 0; }

BCSR::BCSR(int m, int n, int r, int c)
    : r(r), c(c), m(m), n(n), bm(blocks_of(m, r)), bn(blocks_of(n, c)), nnz(0), nnzb(0), values(0), colInd(0), rowPtr(0) {}

BCSR::BCSR(const CSR& dcsr, const int r, const int c)
    : r(r), c(c), m(dcsr.rows), n(dcsr.cols), bm(blocks_of(dcsr.rows, r)), bn(blocks_of(dcsr.cols, c)), nnz(dcsr.nnz), nnzb(0),
      values(0), colInd(0), rowPtr(0) {
  bcsr_or_die(hip_csr_to_bcsr(0, m, n, dcsr.nnz, dcsr.rowPtr, dcsr.colInd, dcsr.values, r, c, &rowPtr, &colInd, &values, &nnzb),
              "BCSR");
}

void BCSR::dispose() {
  spgemm_hip_free(values); values = 0;
  spgemm_hip_free(colInd); colInd = 0;
  spgemm_hip_free(rowPtr); rowPtr = 0;
  nnzb = 0;
}

CSR BCSR::toCSR(double drop_tol) const {
  CSR dC;
  bcsr_or_die(hip_bcsr_to_csr(0, m, n, r, c, nnzb, rowPtr, colInd, values, drop_tol, &dC.rowPtr, &dC.colInd, &dC.values,
                              &dC.nnz), "BCSR::toCSR");
  dC.rows = m;
  dC.cols = n;
  return dC;
}

bool BCSR::isEqual(const CSR& dB) const {
  if (m != dB.rows || n != dB.cols) { printf("%d x %d VS B %d x %d\n", m, n, dB.rows, dB.cols); return false; }
  CSR mine = toCSR(1e-9), theirs;
  theirs.rows = dB.rows; theirs.cols = dB.cols; theirs.nnz = dB.nnz;
  bcsr_or_die(hip_csr_permute(0, dB.rows, dB.cols, dB.nnz, dB.rowPtr, dB.colInd, dB.values, 0, 0, &theirs.rowPtr,
                              &theirs.colInd, &theirs.values), "BCSR::isEqual (copy of B)");
  bcsr_or_die(hip_csr_sort_rows(0, mine.rows, mine.rowPtr, mine.colInd, mine.values), "BCSR::isEqual (sort)");
  bcsr_or_die(hip_csr_sort_rows(0, theirs.rows, theirs.rowPtr, theirs.colInd, theirs.values), "BCSR::isEqual (sort)");
  spgemm_csr_diff d;
  bcsr_or_die(hip_csr_diff(0, m, n, mine.rowPtr, mine.colInd, mine.values, mine.nnz, theirs.rowPtr, theirs.colInd,
                           theirs.values, theirs.nnz, 0.0, 1e-9, &d), "BCSR::isEqual (diff)");
  mine.deviceDispose();
  theirs.deviceDispose();
  if (d.rows_len_differ) printf("row %d: lengths differ\n", d.first_len_row);
  else if (d.beyond) printf("row=%d: a value differs by more than 1e-9\n", d.first_beyond_row);
  return d.rows_len_differ == 0 && d.beyond == 0 && d.max_abs_only_b <= 1e-9;
}
