// CSR.h — host-side mirror of the reference's `struct CSR` (nlibs/CSR.h:23-50) for the SpGEMM path.
// Same fields, same ownership rules (three malloc()ed arrays on the host, device arrays in the SAME struct after
// toGpuCSR(), dispose()==free(), deviceDispose()==device free), same method names, so a driver written against the
// reference compiles against this header.  The arithmetic lives in libspgemm_hip.so (include/spgemm_hip.h); nothing
// here computes a product on the CPU.
#ifndef SMF_CSR_H_
#define SMF_CSR_H_
#include <vector>
#include "tools/macro.h"

struct CSR {
  QValue* values;   // nnz
  int* colInd;      // nnz, 0-based, unsorted inside a row unless makeOrdered() was called
  int* rowPtr;      // rows + 1
  int rows, cols, nnz;

  CSR() : values(0), colInd(0), rowPtr(0), rows(0), cols(0), nnz(0) {}
  CSR(QValue* v, int* ci, int* rp, int r, int c, int nz) { init(v, ci, rp, r, c, nz); }
  void init(QValue* v, int* ci, int* rp, int r, int c, int nz) { values = v; colInd = ci; rowPtr = rp; rows = r; cols = c; nnz = nz; }

  // nlibs/CSR.h:54-82: the cells of a rows x cols row-major array that are not below 1e-8, row by row (negative values
  // and zeros are dropped, NaN stays: NaN < 1e-8 is false); arrays malloc()ed
  void initWithDenseMatrix(const QValue* dvalues, const int rows, const int cols);
  // the same walk on a DEVICE array (hip_dense_to_csr) -> device CSR; rule / tol as in include/spgemm_hip.h, the defaults
  // are the reference's.  Exits on error.
  static CSR gpuInitWithDenseMatrix(const QValue* dvalues, const int rows, const int cols, int rule = 0, double tol = 1e-8);
  CSR deepCopy() const;                 // nlibs/CSR.cc:97-106
  void makeOrdered();                   // nlibs/CSR.cc:73-86: sort every row by (col, value)
  void toAbs();                         // nlibs/CSR.h:152-158
  void averAndNormRowQValue();          // nlibs/CSR.cc:88-95
  int rowCount(int r) const { return rowPtr[r + 1] - rowPtr[r]; }
  void dispose();                       // nlibs/CSR.h:323-327: free() x3
  void output(const char* msg) const;   // nlibs/CSR.h:110-130 (zero-based form)

  // comparison.  isEqual keeps the reference's semantics (nlibs/CSR.h:195-245: dims, rowPtr, |dv| <= 1e-7 through a
  // dense row scatter).  isParityEqual is the stricter rule this project is judged on: rowPtr and colInd identical
  // (both operands ordered), values within `rel` relative.
  bool isEqual(const CSR& B) const;
  bool isParityEqual(const CSR& B, double rel = 1e-6) const;

  // device mirror, nlibs/CSR.cc:342-379 (cudaMalloc/cudaMemcpy there, spgemm_hip_malloc/memcpy here)
  CSR toGpuCSR() const;
  CSR toCpuCSR() const;
  void deviceDispose();

  // C = this * B on the MI355X: sits where CSR::spmm / omp_spmm / somp_spmm / flops_spmm / group_spmm sit
  // (nlibs/CSR.cc:59-208).  Host CSRs in, host CSR out (arrays malloc()ed).  `stride` is the CPU scheduling knob of
  // the reference's signatures; accepted and ignored.  Exits on error like the reference's GPU path.
  CSR hip_spmm(const CSR& B, const int stride = 512) const;

  // reordering, nlibs/CSR.cc:431-494, on the MI355X through hip_csr_permute / hip_csr_transpose /
  // hip_csr_row_descending_permutation: host CSR in (uploaded), host CSR out (arrays malloc()ed, dispose() stays valid).
  // P is a host permutation of the rows (PM) or columns (MP); PMPt / PtMP need a square matrix.  Exit on error.
  CSR PM(const int P[]) const;          // nlibs/CSR.cc:431-445: row i of the result = row P[i]
  CSR MP(const int P[]) const;          // nlibs/CSR.cc:447-464: column c becomes P[c]
  CSR PMPt(const int P[]) const;        // nlibs/CSR.cc:466-473: one pass, no PM temporary
  CSR PtMP(const int P[]) const;        // nlibs/CSR.cc:475-482: undoes PMPt(P)
  int* rowDescendingOrderPermutation(); // nlibs/CSR.cc:484-494: malloc()ed int[rows]; equal lengths by ascending row id
  CSR transpose() const;                // the transposed load (readSNAPFile(isTrans), nlibs/COO.h:19) for any CSR

  // 2 * (number of intermediate products), the reference's original getSpMMFlops (nlibs/cpu_csr_kernel.cc:39-56)
  long long spMMFlops(const CSR& B) const;

  // 18 power-of-two buckets of the row lengths (nlibs/CSR.cc:241-248); host CSR: counted here, device CSR
  // (after toGpuCSR): hip_nnzStats
  std::vector<int> nnzStats() const;
  std::vector<int> gpuNnzStats() const;
  // how the row lengths moved from *this to B (nlibs/CSR.cc:381-415; the drift report of the R-MCL loop under --stats):
  // counts[k] = rows whose relative change (len_B - len_A) / len_A is below percents[k] (first such k), counts[n] = the
  // rest, then three more: rows that appeared (0 -> >0), rows empty in both, rows unchanged.  n = percents.size().
  std::vector<int> differsStats(const CSR& B, const std::vector<QValue>& percents) const;
  // the squared Frobenius norm of *this - B (nlibs/CSR.cc:210-240: how far an R-MCL iteration moved Mt); both operands
  // ordered (makeOrdered), summed in QValue by the reference's two-pointer merge
  QValue differs(const CSR& B) const;

  // the same three on DEVICE CSRs (after toGpuCSR, rows ordered: hip_csr_sort_rows) through hip_csr_diff /
  // hip_csr_differsStats, nothing downloaded.  gpuDiffers accumulates in double and rounds once to QValue.  gpuIsEqual is
  // isEqual's rule (dims, nnz, row lengths, |dv| <= 1e-7) and prints the first offending row like isEqual does.
  QValue gpuDiffers(const CSR& dB) const;
  std::vector<int> gpuDiffersStats(const CSR& dB, const std::vector<QValue>& percents) const;
  bool gpuIsEqual(const CSR& dB) const;

  // selection on a DEVICE CSR (hip_csr_row_topk; no counterpart in the reference, whose row rule only thresholds): every
  // row keeps its min(len, k) best entries in storage order -- larger value, then smaller column, then earlier position,
  // NaN last -- as a new DEVICE CSR.  flags: 0 or SPGEMM_TOPK_NORMALISE (the kept values of the rows that were cut are
  // divided by their sum).  Exits on error.
  CSR gpuRowTopK(int k, int flags = 0) const;
};
#endif
