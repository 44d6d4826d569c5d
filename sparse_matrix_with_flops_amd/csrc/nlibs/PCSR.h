// PCSR.h — mirror of the reference's `struct PCSR` (nlibs/PCSR.h:5-10) on DEVICE arrays: a matrix cut into c column
// blocks of width stride() = ceil(cols / c), every block an ordinary CSR of shape rows x stride() with block-local
// columns.  Same fields, same ownership rule: the blocks made by the constructor are views into three packed arrays
// (block 0 holds the base pointers) and dispose() frees those only (nlibs/PCSR.h:39-50); blocks filled in one by one, as
// spmm() does, are separate allocations and dispose() frees each (`packed` says which).  The work is done by libspgemm_hip.so
// (include/spgemm_hip.h, "column-partitioned CSR").
#ifndef SMF_PCSR_H_
#define SMF_PCSR_H_
#include "CSR.h"

struct PCSR {
  int rows, cols;
  int c;
  CSR* blocks;          // c device CSRs
  // the blocks are views into block 0's arrays.  The reference tells by blocks[1].rowPtr - blocks[0].rowPtr == rows + 1;
  // two separate blocks handed out by the device pool can lie exactly that far apart, so the fact is kept instead.
  bool packed;

  // nlibs/PCSR.cc:3-56 on a device CSR (after toGpuCSR): hip_csr_split_columns.  Exits on error.
  PCSR(const CSR& dcsr, const int c);
  // nlibs/PCSR.h:32-37: c empty blocks to be filled in
  PCSR(const int rows, const int cols, const int c);

  int stride() const { return cols > 0 ? (cols + c - 1) / c : 1; }
  int nnz() const {
    int tnnz = 0;
    for (int b = 0; b < c; ++b) tnnz += blocks[b].nnz;
    return tnnz;
  }
  void dispose();

  // one device CSR rows x cols: row i = block 0's row i, block 1's row i, ... with global columns (hip_pcsr_join)
  CSR join() const;
  // nlibs/PCSR.h:52-100 against a device CSR: shape and nnz first (false, with the reference's lines, before any device
  // work), then the joined blocks and a copy of dB are row-sorted on the device and one hip_csr_diff report is read by
  // CSR::isEqual's rule (row lengths equal, |dv| <= 1e-7).  dB itself is not modified.
  bool isEqual(const CSR& dB) const;
};

// PCSR spmm(const CSR& A, const PCSR& pB, stride) of correctTests/pcsrTest.cc:7-19 on device operands: hip_pcsr_spmm
PCSR spmm(const CSR& dA, const PCSR& pB);
#endif
