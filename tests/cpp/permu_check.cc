// tests/cpp/permu_check.cc — the reference's ordering experiment (correctTests/permuTest.cc) on this project's C++
// mirror: the product of a matrix with itself must not depend on how its rows and columns are numbered.
//   load -> rmclInit -> A' = PMPt(A) for a seeded random P -> C = A*A and C' = A'*A' on the device -> PtMP(C') ->
//   makeOrdered both -> compare -> print Same / Diffs.
// The reference times its CPU kernel around the two products; timing lives in tools/reorder_bench.py here.
//   usage: permu_check <snap file> [seed]       exit code 0 iff Same
#include <cstdio>
#include <cstdlib>

#include "COO.h"
#include "CSR.h"
#include "qrmcl.h"
#include "tools/util.h"

int main(int argc, char* argv[]) {
  if (argc < 2) { printf("usage: %s <snap file> [seed]\n", argv[0]); return 2; }
  const unsigned seed = argc > 2 ? (unsigned)strtoul(argv[2], 0, 10) : 7u;
  COO coo;
  coo.readSNAPFile(argv[1], true);
  CSR A = rmclInit(coo);
  coo.dispose();
  int* P = randomPermutationVector(A.rows, seed);
  int* Pt = permutationTranspose(P, A.rows);
  bool inverse = true;
  for (int i = 0; i < A.rows; ++i) inverse = inverse && Pt[P[i]] == i;
  CSR pAPt = A.PMPt(P);
  CSR C = A.hip_spmm(A);
  CSR pCPt = pAPt.hip_spmm(pAPt);
  CSR back = pCPt.PtMP(P);
  back.makeOrdered();
  C.makeOrdered();
  const bool same = inverse && pAPt.nnz == A.nnz && back.isParityEqual(C);
  printf("rows=%d nnzA=%d nnzC=%d seed=%u\n", A.rows, A.nnz, C.nnz, seed);
  printf("%s\n", same ? "Same" : "Diffs");
  A.dispose(); pAPt.dispose(); C.dispose(); pCPt.dispose(); back.dispose();
  free(P); free(Pt);
  return same ? 0 : 1;
}
