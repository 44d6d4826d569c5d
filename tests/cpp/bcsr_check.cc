// tests/cpp/bcsr_check.cc — the two scenarios of the reference's tests/BCSR_test.cc on this project's C++ mirror, on the
// device: a 4 x 4 and a ragged 5 x 5 matrix, both tiled with r = c = 2.
//   bcsr_check
//     per scenario: A on the device -> BCSR(A, 2, 2) (hip_csr_to_bcsr) -> the three arrays downloaded and compared with
//     the expected ones -> nonzeroDensity -> isEqual(A) must hold, isEqual(A with one value changed) and isEqual(A with
//     one entry fewer) must not (the entry left out is given per scenario).  One line per check ("<scenario> <check>: ok" / "... FAILED"), "Pass" at the end.
//     Exit code 0 iff every check passed.
//   bcsr_check --shape-check
//     no device work: BCSR::isEqual must refuse another row or column count before it touches a device
//     (tests/test_bcsr_abi.py); prints "refused" and exits 0 when both are refused.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spgemm_hip.h"
#include "BCSR.h"
#include "CSR.h"

static int failures = 0;

static void check(const char* scenario, const char* what, bool ok) {
  printf("%s %s: %s\n", scenario, what, ok ? "ok" : "FAILED");
  if (!ok) ++failures;
}

// a host CSR over borrowed vectors, uploaded
static CSR upload(std::vector<int>& rp, std::vector<int>& ci, std::vector<QValue>& v, int rows, int cols) {
  const CSR h(v.data(), ci.data(), rp.data(), rows, cols, (int)ci.size());
  return h.toGpuCSR();
}

template <class T>
static bool device_equals(const T* d, const std::vector<T>& want) {
  std::vector<T> got(want.size());
  if (!want.empty() && spgemm_hip_memcpy_d2h(got.data(), d, sizeof(T) * want.size())) return false;
  return want.empty() || !memcmp(got.data(), want.data(), sizeof(T) * want.size());
}

static void scenario(const char* name, int rows, int cols, std::vector<int> rp, std::vector<int> ci, std::vector<QValue> v, int drop,
                     const std::vector<int>& wantRp, const std::vector<int>& wantCi, const std::vector<QValue>& wantV) {
  CSR dA = upload(rp, ci, v, rows, cols);
  BCSR b(dA, 2, 2);
  check(name, "shape", b.bm == (rows + 1) / 2 && b.bn == (cols + 1) / 2 && b.nnz == (int)ci.size() &&
                           b.nnzb == (int)wantCi.size());
  check(name, "rowPtr", device_equals(b.rowPtr, wantRp));
  check(name, "colInd", device_equals(b.colInd, wantCi));
  check(name, "values", device_equals(b.values, wantV));
  check(name, "density", fabs(b.nonzeroDensity() - 100.0 * ci.size() / (4.0 * wantCi.size())) < 1e-12);
  check(name, "equal to itself", b.isEqual(dA));
  std::vector<QValue> v2 = v;
  v2.back() += 3;                                            // the last entry, as the reference's test changes it
  CSR dChanged = upload(rp, ci, v2, rows, cols);
  check(name, "not equal after a value changed", !b.isEqual(dChanged));
  std::vector<int> rp3 = rp, ci3 = ci;
  std::vector<QValue> v3 = v;
  ci3.erase(ci3.begin() + drop);
  v3.erase(v3.begin() + drop);
  for (size_t i = 0; i < rp3.size(); ++i) if (rp3[i] > drop) --rp3[i];
  CSR dFewer = upload(rp3, ci3, v3, rows, cols);
  check(name, "not equal with one entry fewer", !b.isEqual(dFewer));
  dFewer.deviceDispose(); dChanged.deviceDispose(); dA.deviceDispose();
  b.dispose();
}

static int shape_check() {
  // no arrays anywhere: anything that reached the device would fail (and exit) instead of returning false
  const BCSR b(4, 4, 2, 2);
  const CSR tall(0, 0, 0, 5, 4, 0), wide(0, 0, 0, 4, 5, 0);
  const bool refused = !b.isEqual(tall) && !b.isEqual(wide);
  printf("%s\n", refused ? "refused" : "accepted");
  return refused ? 0 : 1;
}

int main(int argc, char* argv[]) {
  if (argc >= 2 && !strcmp(argv[1], "--shape-check")) return shape_check();
  // 4 x 4:   {1:2}   {1:3}   {0:4}   {1:1, 3:5}
  scenario("4x4", 4, 4, {0, 1, 2, 3, 5}, {1, 1, 0, 1, 3}, {2, 3, 4, 1, 5}, 3,
           {0, 1, 3}, {0, 0, 1}, {0, 2, 0, 3, 4, 0, 0, 1, 0, 0, 0, 5});
  // ragged 5 x 5:   {1:2}   {1:3, 4:3}   {0:4}   {1:1, 3:5}   {0:2}
  scenario("5x5", 5, 5, {0, 1, 3, 4, 6, 7}, {1, 1, 4, 0, 1, 3, 0}, {2, 3, 3, 4, 1, 5, 2}, 2,
           {0, 2, 4, 5}, {0, 2, 0, 1, 0}, {0, 2, 0, 3, 0, 0, 3, 0, 4, 0, 0, 1, 0, 0, 0, 5, 2, 0, 0, 0});
  printf("%s\n", failures ? "Fail" : "Pass");
  return failures ? 1 : 0;
}
