// BCSR.h — mirror of the reference's `struct BCSR` (nlibs/BCSR.h:6-64) on DEVICE arrays: an m x n matrix stored as r x c
// dense tiles.  Same fields: rowPtr is int[bm + 1] over the block rows, colInd holds nnzb block columns, values holds
// nnzb * r * c numbers (tile k at k * r * c, entry (i, col) in cell (i % r) * c + col % c, every other cell 0); nnz is the
// source CSR's, as the reference keeps it.  The tiles of a block row are in first-occurrence order.  The work is done by
// libspgemm_hip.so (include/spgemm_hip.h, "blocked CSR").
#ifndef SMF_BCSR_H_
#define SMF_BCSR_H_
#include "CSR.h"

struct BCSR {
  int r, c;
  int m, n;
  int bm, bn;
  int nnz;              // of the CSR it was made from
  int nnzb;             // tiles (the reference reads rowPtr[bm]; that is device memory here)

  QValue* values;       // device, nnzb * r * c
  int* colInd;          // device, nnzb
  int* rowPtr;          // device, bm + 1

  // nlibs/BCSR.cc:3-65 on a device CSR (after toGpuCSR): hip_csr_to_bcsr.  r before c, as the reference's definition has
  // them (its header declares c first; the definition is what runs).  Exits on error.
  BCSR(const CSR& dcsr, const int r, const int c);
  // nlibs/BCSR.h:17-27: the shape alone, no arrays
  BCSR(int m, int n, int r, int c);

  void dispose();
  // nlibs/BCSR.h:61-63; 0 without tiles (the reference divides by zero there)
  double nonzeroDensity() const { return nnzb > 0 ? (double)nnz / ((double)nnzb * r * c) * 100.0 : 0.0; }
  // the tiles written out as a device CSR (hip_bcsr_to_csr): a cell is kept when fabs(v) > drop_tol
  CSR toCSR(double drop_tol = 1e-9) const;
  // nlibs/BCSR.cc:67-116 against a device CSR: another shape is false (with a line, before any device work); then the
  // tiles are written out with drop_tol = 1e-9, that and a copy of dB are row-sorted on the device and one hip_csr_diff
  // report (abs_tol = 1e-9, rel_tol = 0) is read: equal iff the row lengths agree, no common column is further than 1e-9
  // apart and no entry only dB holds exceeds 1e-9.  dB itself is not modified.
  bool isEqual(const CSR& dB) const;
};
#endif
