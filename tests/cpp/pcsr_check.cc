// tests/cpp/pcsr_check.cc — the reference's column-partition experiment (correctTests/pcsrTest.cc) on this project's C++
// mirror, on the device: the product computed block by block over a column split of B must be the whole product.
//   pcsr_check <snap file> [c]
//     load -> rmclInit -> A, B = A on the device -> C = A*B (gpuSpMMWrapper) -> pB = PCSR(B, c) (default 2) ->
//     pC = spmm(A, pB) (hip_pcsr_spmm) -> join -> both row-sorted on the device -> one hip_csr_diff report at
//     rel_tol = 1e-6 (the project's parity tolerance), abs_tol = 1e-7 (the reference's isEqual figure) -> prints
//     max_abs_err, the structural counts and Same / Diffs.  Same = rows_len_differ == only_a == only_b == beyond == 0.
//     The two products may add the same terms in another order, so the verdict is not bit equality; what the stricter
//     PCSR::isEqual (every |dv| <= 1e-7, no relative term) says is printed beside it.  The reference times its CPU kernel around the blockwise product; timing lives in tools/pcsr_bench.py.
//     Exit code 0 iff Same.
//   pcsr_check --shape-check
//     no device work: PCSR::isEqual must refuse another row count, column count or nnz before it touches a device
//     (tests/test_pcsr_abi.py); prints "refused" and exits 0 when all three are refused.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/spgemm_hip.h"
#include "COO.h"
#include "CSR.h"
#include "PCSR.h"
#include "gpus/gpu_csr_kernel.h"
#include "qrmcl.h"

static int shape_check() {
  // blocks and B hold no arrays: anything that reached the device would fail (and exit) instead of returning false
  PCSR p(3, 5, 2);
  p.blocks[0].init(0, 0, 0, 3, 3, 2);
  p.blocks[1].init(0, 0, 0, 3, 3, 3);
  const CSR tall(0, 0, 0, 4, 5, 5), wide(0, 0, 0, 3, 6, 5), fuller(0, 0, 0, 3, 5, 6);
  const bool refused = !p.isEqual(tall) && !p.isEqual(wide) && !p.isEqual(fuller);
  free(p.blocks);
  printf("%s\n", refused ? "refused" : "accepted");
  return refused ? 0 : 1;
}

int main(int argc, char* argv[]) {
  if (argc >= 2 && !strcmp(argv[1], "--shape-check")) return shape_check();
  if (argc < 2) { printf("usage: %s <snap file> [c] | --shape-check\n", argv[0]); return 2; }
  const int c = argc > 2 ? atoi(argv[2]) : 2;
  COO cooAt;
  cooAt.readSNAPFile(argv[1], true);
  CSR hA = rmclInit(cooAt);
  cooAt.dispose();
  CSR A = hA.toGpuCSR(), B = hA.toGpuCSR();
  CSR C = gpuSpMMWrapper(A, B);
  PCSR pB(B, c);
  B.deviceDispose();
  PCSR pC = spmm(A, pB);
  pB.dispose();

  CSR J = pC.join();
  if (hip_csr_sort_rows(0, J.rows, J.rowPtr, J.colInd, J.values) || hip_csr_sort_rows(0, C.rows, C.rowPtr, C.colInd, C.values)) {
    printf("%s\n", spgemm_hip_last_error());
    return 1;
  }
  spgemm_csr_diff d;
  if (hip_csr_diff(0, J.rows, J.cols, J.rowPtr, J.colInd, J.values, J.nnz, C.rowPtr, C.colInd, C.values, C.nnz, 1e-6, 1e-7, &d)) {
    printf("%s\n", spgemm_hip_last_error());
    return 1;
  }
  const bool mirror = pC.isEqual(C);
  printf("rows=%d nnzA=%d nnzC=%d c=%d stride=%d\n", hA.rows, hA.nnz, C.nnz, c, pC.stride());
  printf("max_abs_err=%e rows_len_differ=%d only_a=%lld only_b=%lld beyond=%lld\n", d.max_abs_err, d.rows_len_differ, d.only_a,
         d.only_b, d.beyond);
  printf("PCSR::isEqual: %s\n", mirror ? "equal" : "not equal");
  const bool same = J.nnz == C.nnz && d.rows_len_differ == 0 && d.only_a == 0 && d.only_b == 0 && d.beyond == 0;
  printf("%s\n", same ? "Same" : "Diffs");
  J.deviceDispose(); C.deviceDispose(); A.deviceDispose();
  pC.dispose();
  hA.dispose();
  return same ? 0 : 1;
}
