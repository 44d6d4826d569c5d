// MCSR.h — mirror of the reference's `struct MCSR : public CSR, BCSR` (nlibs/MCSR.h:6-9) on DEVICE arrays: the top-left
// blockRows x blockCols corner of a matrix as r x c dense tiles (the BCSR base: m = blockRows, n = blockCols, bm =
// blockRows / r, bn = ceil(blockCols / c)), everything else as a CSR with global columns (the CSR base: rows x cols of
// the whole matrix).  The definition is the reference's fill pass (nlibs/MCSR.cc:58-92); its count pass is wrong for
// r > 1 and is not reproduced.  BCSR::nnz is the number of entries that went into the corner, repeats counted (the
// reference leaves it 0).  The work is done by libspgemm_hip.so (include/spgemm_hip.h, "mixed CSR").
#ifndef SMF_MCSR_H_
#define SMF_MCSR_H_
#include "BCSR.h"
#include "CSR.h"

struct MCSR : public CSR, BCSR {
  // nlibs/MCSR.cc:3-97 on a device CSR (after toGpuCSR): hip_csr_to_mcsr.  r before c, as the reference's definition has
  // them (its header declares c first).  Exits on error; prints none of the reference's debug output.
  MCSR(const CSR& dcsr, const int r, const int c, const int blockRows, const int blockCols);

  // both parts back to the pool
  void dispose();
  // the two parts written out as one device CSR (hip_mcsr_to_csr): the corner's row i, then the remainder's row i
  CSR toCSR(double drop_tol = 1e-9) const;
  // BCSR::nonzeroDensity of the corner
  double nonzeroDensity() const { return BCSR::nonzeroDensity(); }
};
#endif
