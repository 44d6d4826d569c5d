// PCSR.cc — see PCSR.h.  Host-side glue only; split, join and the products run in libspgemm_hip.so.
#include "PCSR.h"
#include "../../../include/spgemm_hip.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static void pcsr_or_die(int rc, const char* what) {
  if (rc != SPGEMM_OK) { printf("%s: %s\n", what, spgemm_hip_last_error()); exit(EXIT_FAILURE); }
}

static CSR* empty_blocks(int c) {
  CSR* blocks = (CSR*)malloc((size_t)(c > 0 ? c : 1) * sizeof(CSR));
  if (!blocks) { printf("out of host memory allocating %d blocks\n", c); exit(EXIT_FAILURE); }
  for (int b = 0; b < c; ++b) blocks[b] = CSR();
  return blocks;
}

PCSR::PCSR(const int rows, const int cols, const int c) : rows(rows), cols(cols), c(c), blocks(empty_blocks(c)), packed(false) {}

PCSR::PCSR(const CSR& dcsr, const int c) : rows(dcsr.rows), cols(dcsr.cols), c(c), blocks(empty_blocks(c)), packed(true) {
  int *rowPtr = 0, *colInd = 0;
  QValue* values = 0;
  std::vector<int> blockPtr((size_t)(c > 0 ? c : 0) + 1, 0);
  pcsr_or_die(hip_csr_split_columns(0, rows, cols, dcsr.nnz, dcsr.rowPtr, dcsr.colInd, dcsr.values, c, &rowPtr, &colInd,
                                    &values, blockPtr.data()), "PCSR");
  for (int b = 0; b < c; ++b)                                 // nlibs/PCSR.cc:29-32
    blocks[b].init(values + blockPtr[b], colInd + blockPtr[b], rowPtr + (size_t)b * ((size_t)rows + 1), rows, stride(),
                   blockPtr[b + 1] - blockPtr[b]);
}

void PCSR::dispose() {                                        // nlibs/PCSR.h:39-50
  if (packed) {
    if (c >= 1) blocks[0].deviceDispose();
  } else {
    for (int b = 0; b < c; ++b) blocks[b].deviceDispose();
  }
  free(blocks);
  blocks = 0;
}

// the block table the C side takes: c rowPtr / colInd / values device pointers and c counts
struct BlockTable {
  std::vector<const int*> I, J;
  std::vector<const QValue*> A;
  std::vector<int> nnz;
  explicit BlockTable(const PCSR& p) {
    for (int b = 0; b < p.c; ++b) {
      I.push_back(p.blocks[b].rowPtr); J.push_back(p.blocks[b].colInd); A.push_back(p.blocks[b].values);
      nnz.push_back(p.blocks[b].nnz);
    }
  }
};

CSR PCSR::join() const {
  const BlockTable t(*this);
  CSR dC;
  pcsr_or_die(hip_pcsr_join(0, rows, cols, c, t.I.data(), t.J.data(), t.A.data(), t.nnz.data(), &dC.rowPtr, &dC.colInd,
                            &dC.values, &dC.nnz), "PCSR::join");
  dC.rows = rows;
  dC.cols = cols;
  return dC;
}

bool PCSR::isEqual(const CSR& dB) const {
  bool flag = true;
  if (rows != dB.rows) { printf("rows = %d\tB_rows = %d\n", rows, dB.rows); flag = false; }
  if (cols != dB.cols) { printf("cols = %d\tB_cols = %d\n", cols, dB.cols); flag = false; }
  const int tnnz = nnz();
  if (tnnz != dB.nnz) { printf("nnz = %d\tB_nnz = %d\n", tnnz, dB.nnz); flag = false; }
  if (!flag) return false;
  CSR mine = join(), theirs;
  theirs.rows = dB.rows; theirs.cols = dB.cols; theirs.nnz = dB.nnz;
  pcsr_or_die(hip_csr_permute(0, dB.rows, dB.cols, dB.nnz, dB.rowPtr, dB.colInd, dB.values, 0, 0, &theirs.rowPtr,
                              &theirs.colInd, &theirs.values), "PCSR::isEqual (copy of B)");
  pcsr_or_die(hip_csr_sort_rows(0, mine.rows, mine.rowPtr, mine.colInd, mine.values), "PCSR::isEqual (sort)");
  pcsr_or_die(hip_csr_sort_rows(0, theirs.rows, theirs.rowPtr, theirs.colInd, theirs.values), "PCSR::isEqual (sort)");
  const bool same = mine.gpuIsEqual(theirs);
  mine.deviceDispose();
  theirs.deviceDispose();
  return same;
}

PCSR spmm(const CSR& dA, const PCSR& pB) {
  if (dA.cols != pB.rows) { printf("spmm: A is %dx%d but pB is %dx%d\n", dA.rows, dA.cols, pB.rows, pB.cols); exit(EXIT_FAILURE); }
  PCSR pC(dA.rows, pB.cols, pB.c);
  const BlockTable t(pB);
  std::vector<int*> I((size_t)pB.c), J((size_t)pB.c);
  std::vector<QValue*> C((size_t)pB.c);
  std::vector<int> nnz((size_t)pB.c);
  pcsr_or_die(hip_pcsr_spmm(0, dA.rowPtr, dA.colInd, dA.values, dA.nnz, dA.rows, dA.cols, pB.cols, pB.c, t.I.data(),
                            t.J.data(), t.A.data(), t.nnz.data(), I.data(), J.data(), C.data(), nnz.data()), "spmm");
  for (int b = 0; b < pB.c; ++b) pC.blocks[b].init(C[(size_t)b], J[(size_t)b], I[(size_t)b], dA.rows, pB.stride(), nnz[(size_t)b]);
  return pC;
}
