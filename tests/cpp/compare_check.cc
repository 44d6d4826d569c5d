// tests/cpp/compare_check.cc — the reference's end-of-run check (nrmcl.cc:26-28: Mt.makeOrdered(); oMt.makeOrdered();
// Mt.isEqual(oMt) -> Same / Diffs) on DEVICE CSRs through the C++ mirror: nothing is downloaded to compare.
//   compare_check <snap file> [iters]
//     RMCL(file, iters, GPU) -> Mt and its deepCopy -> toGpuCSR both -> hip_csr_sort_rows both -> gpuIsEqual -> "Same";
//     then one value of the copy is changed by 1e-3 -> "changed row R", gpuIsEqual's own line naming the row, "Diffs".
//     Exit code 0 iff the first check says Same, the second says Diffs and names row R, and gpuDiffers agrees with the
//     host CSR::differs on both pairs.
//   compare_check --host-stats <rowPtr file A> <rowPtr file B>
//     no device work: the mirror's host CSR::differsStats with the reference's percents (nlibs/qrmcl.cc:17) on two row
//     pointers read from text files ("m" then m + 1 integers); prints the counts on one line (tests/test_compare_abi.py).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spgemm_hip.h"
#include "COO.h"
#include "CSR.h"
#include "process_args.h"
#include "qrmcl.h"

static bool read_rowptr(const char* path, std::vector<int>* rp) {
  FILE* fp = fopen(path, "r");
  if (!fp) return false;
  int m = 0;
  bool ok = fscanf(fp, "%d", &m) == 1 && m >= 0;
  rp->assign(ok ? (size_t)m + 1 : 0, 0);
  for (size_t i = 0; ok && i < rp->size(); ++i) ok = fscanf(fp, "%d", &(*rp)[i]) == 1;
  fclose(fp);
  return ok;
}

static int host_stats(const char* fa, const char* fb) {
  std::vector<int> ra, rb;
  if (!read_rowptr(fa, &ra) || !read_rowptr(fb, &rb) || ra.size() != rb.size()) { printf("cannot read the row pointers\n"); return 2; }
  static const int cpercents[] = {-30, -20, -5, 0, 5, 20, 30, 100};
  const std::vector<QValue> percents(cpercents, cpercents + sizeof(cpercents) / sizeof(int));
  const int m = (int)ra.size() - 1;
  const CSR A(0, 0, ra.data(), m, m, ra[m]), B(0, 0, rb.data(), m, m, rb[m]);
  const std::vector<int> counts = A.differsStats(B, percents);
  for (size_t i = 0; i < counts.size(); ++i) printf("%d ", counts[i]);
  printf("\n");
  return 0;
}

static CSR sorted_on_device(const CSR& M) {
  CSR d = M.toGpuCSR();
  if (hip_csr_sort_rows(0, d.rows, d.rowPtr, d.colInd, d.values)) { printf("%s\n", spgemm_hip_last_error()); exit(EXIT_FAILURE); }
  return d;
}

int main(int argc, char* argv[]) {
  if (argc >= 4 && !strcmp(argv[1], "--host-stats")) return host_stats(argv[2], argv[3]);
  if (argc < 2) { printf("usage: %s <snap file> [iters] | --host-stats <rowPtr A> <rowPtr B>\n", argv[0]); return 2; }
  const int iters = argc > 2 ? atoi(argv[2]) : 3;
  CSR Mt = RMCL(argv[1], iters, GPU);
  CSR oMt = Mt.deepCopy();
  CSR dMt = sorted_on_device(Mt), dOMt = sorted_on_device(oMt);
  const bool same = dMt.gpuIsEqual(dOMt);
  const double moved0 = dMt.gpuDiffers(dOMt);
  printf("rows=%d nnz=%d differs=%e\n", Mt.rows, Mt.nnz, moved0);
  printf("%s\n", same ? "Same" : "Diffs");
  dOMt.deviceDispose();

  const int p = oMt.nnz / 2;
  int row = 0;
  while (row + 1 < oMt.rows && oMt.rowPtr[row + 1] <= p) ++row;
  oMt.values[p] += (QValue)1e-3;
  printf("changed row %d\n", row);
  dOMt = sorted_on_device(oMt);
  const bool still = dMt.gpuIsEqual(dOMt);
  const double moved = dMt.gpuDiffers(dOMt);
  Mt.makeOrdered();
  oMt.makeOrdered();
  const double want = Mt.differs(oMt);
  printf("differs: device %e host %e\n", moved, want);
  printf("%s\n", still ? "Same" : "Diffs");
  spgemm_csr_diff d;
  if (hip_csr_diff(0, dMt.rows, dMt.cols, dMt.rowPtr, dMt.colInd, dMt.values, dMt.nnz, dOMt.rowPtr, dOMt.colInd, dOMt.values,
                   dOMt.nnz, 0.0, 1e-7, &d)) { printf("%s\n", spgemm_hip_last_error()); return 1; }
  // one term (a - b)^2 of about 1e-6: the float host loop and the double device sum agree to float rounding
  const bool ok = same && moved0 == 0.0 && !still && d.beyond == 1 && d.first_beyond_row == row &&
                  std::fabs(moved - want) <= 1e-5 * want && want > 0.0;
  dMt.deviceDispose(); dOMt.deviceDispose();
  Mt.dispose(); oMt.dispose();
  return ok ? 0 : 1;
}
