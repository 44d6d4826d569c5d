// tests/cpp/mcsr_check.cc — the scenario of the reference's tests/MCSR_test.cc:9-33 on this project's C++ mirror, on the
// device: its 7 x 7 matrix, MCSR(A, 1, 2, 4, 4).  The vectors are those of tests/golden/mcsr_kat.json.
//   mcsr_check
//     A on the device -> MCSR(A, 1, 2, 4, 4) (hip_csr_to_mcsr) -> the six arrays downloaded and compared with the expected
//     ones -> nonzeroDensity of the corner -> toCSR() must give A back bit for bit (r == 1, A's rows are column-sorted).
//     One line per check ("7x7 <check>: ok" / "... FAILED"), "Pass" at the end.  Exit code 0 iff every check passed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/spgemm_hip.h"
#include "CSR.h"
#include "MCSR.h"

static int failures = 0;

static void check(const char* what, bool ok) {
  printf("7x7 %s: %s\n", what, ok ? "ok" : "FAILED");
  if (!ok) ++failures;
}

template <class T>
static bool device_equals(const T* d, const std::vector<T>& want) {
  std::vector<T> got(want.size());
  if (!want.empty() && spgemm_hip_memcpy_d2h(got.data(), d, sizeof(T) * want.size())) return false;
  return want.empty() || !memcmp(got.data(), want.data(), sizeof(T) * want.size());
}

int main() {
  std::vector<int> rp = {0, 2, 4, 8, 9, 13, 14, 17};
  std::vector<int> ci = {0, 1, 2, 6, 1, 2, 3, 5, 4, 0, 3, 5, 6, 2, 1, 4, 6};
  std::vector<QValue> v = {1, 2, 3, 4, 4, 2, 3, 5, 2, 3, 1, 8, 1, 3, 2, 1, 3};
  const CSR hA(v.data(), ci.data(), rp.data(), 7, 7, (int)ci.size());
  CSR dA = hA.toGpuCSR();
  MCSR mA(dA, 1, 2, 4, 4);
  check("shape", mA.rows == 7 && mA.cols == 7 && mA.m == 4 && mA.n == 4 && mA.r == 1 && mA.c == 2 && mA.bm == 4 &&
                     mA.bn == 2 && mA.nnzb == 4 && mA.CSR::nnz == 11 && mA.BCSR::nnz == 6);
  check("remainder rowPtr", device_equals(mA.CSR::rowPtr, std::vector<int>{0, 0, 1, 2, 3, 7, 8, 11}));
  check("remainder colInd", device_equals(mA.CSR::colInd, std::vector<int>{6, 5, 4, 0, 3, 5, 6, 2, 1, 4, 6}));
  check("remainder values", device_equals(mA.CSR::values, std::vector<QValue>{4, 5, 2, 3, 1, 8, 1, 3, 2, 1, 3}));
  check("block rowPtr", device_equals(mA.BCSR::rowPtr, std::vector<int>{0, 1, 2, 4, 4}));
  check("block colInd", device_equals(mA.BCSR::colInd, std::vector<int>{0, 1, 0, 1}));
  check("tiles", device_equals(mA.BCSR::values, std::vector<QValue>{1, 2, 3, 0, 0, 4, 2, 3}));
  check("density", fabs(mA.nonzeroDensity() - 75.0) < 1e-12);
  CSR back = mA.toCSR();
  check("round trip shape", back.rows == 7 && back.cols == 7 && back.nnz == 17);
  check("round trip rowPtr", device_equals(back.rowPtr, rp));
  check("round trip colInd", device_equals(back.colInd, ci));
  check("round trip values", device_equals(back.values, v));
  back.deviceDispose();
  mA.dispose();
  dA.deviceDispose();
  printf("%s\n", failures ? "Fail" : "Pass");
  return failures ? 1 : 0;
}
