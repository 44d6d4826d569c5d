// edge_print_check -- the line formatter (csrc/edge_print.hpp) against the C library, on the host, stand-alone.
//
//   edge_print_check.x <seed>        runs (a), (b) and (c) below; exit status 0 only if every condition holds
//
// The reference for every line is snprintf: "%d\t%d\t%.6lf\n" (FIXED6), "%d %d %.9g\n" (ROUNDTRIP, a float, promoted as
// printf promotes it) and "%d %d %.17g\n" (ROUNDTRIP, a double).  Two conditions hold for every line:
//   exact   a line the formatter does not call slow has the reference's bytes and length, line_length says the same
//           length, and promote_float_bits is the bits of (double)f
//   fast    FIXED6: +-0 and every finite |x| < 1e15; ROUNDTRIP: +-0 and every finite 1e-15 <= |x| < 1e17 is NOT slow.  The
//           class is decided here with floating-point comparisons, not taken from the formatter.
//   (a) the crafted table, every value in both formats, as a double and (when it is one) as a float
//   (b) 2 000 000 doubles and 2 000 000 floats, each in both formats: half random bit patterns, half drawn log-uniformly
//       inside the required class of the format
//   (c) no fast line is longer than PRINT_LINE_MAX, and PRINT_LINE_MAX is at most 11 + 1 + 11 + 1 + 24 + 1
// Every output buffer is a heap block of exactly the line's length: a byte written behind it is a heap overflow the
// sanitizer build reports.
#include "../../sparse_matrix_with_flops_amd/csrc/edge_print.hpp"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {
using namespace edgeprint;

struct Tally { long long lines = 0, slow = 0, bad = 0, must_fast = 0, fast_missed = 0; int longest = 0; };

bool required_fast(double x, int fmt) {
  if (x == 0.0) return true;
  if (!std::isfinite(x)) return false;
  const double a = std::fabs(x);
  return fmt == FIXED6 ? a < 1e15 : (a >= 1e-15 && a < 1e17);
}

// one line: indices a, b; the value as double bits, P = 9 when it came from a float
void check(int a, int b, uint64_t bits, int fmt, int P, Tally& t, const char* what) {
  double x;
  memcpy(&x, &bits, 8);
  char want[512];
  const int wlen = fmt == FIXED6 ? snprintf(want, sizeof want, "%d\t%d\t%.6lf\n", a, b, x)
                 : P == 9       ? snprintf(want, sizeof want, "%d %d %.9g\n", a, b, x)
                                : snprintf(want, sizeof want, "%d %d %.17g\n", a, b, x);
  ++t.lines;
  const bool must = required_fast(x, fmt);
  if (must) ++t.must_fast;
  const int len = line_length(a, b, bits, fmt, P);
  if (len == PRINT_SLOW) {
    ++t.slow;
    char* one = (char*)malloc(1);
    if (print_line(one, a, b, bits, fmt, P) != PRINT_SLOW && ++t.bad <= 10) printf("length slow, line not (%s) %s", what, want);
    free(one);
    if (must && ++t.fast_missed <= 10) printf("SLOW, must be fast (%s) %s", what, want);
    return;
  }
  if (len <= 0 || len > PRINT_LINE_MAX) {
    if (++t.bad <= 10) printf("length %d out of (0, %d] (%s) %s", len, PRINT_LINE_MAX, what, want);
    return;
  }
  if (len > t.longest) t.longest = len;
  char* exact = (char*)malloc((size_t)len);
  const int got = print_line(exact, a, b, bits, fmt, P);
  if (got != len || len != wlen || memcmp(exact, want, (size_t)len) != 0) {
    if (++t.bad <= 10) printf("MISMATCH (%s) fmt=%d P=%d got %d bytes \"%.*s\" want %d bytes %s", what, fmt, P, got,
                              got > 0 ? got - 1 : 0, exact, wlen, want);
  }
  free(exact);
}

void check_double(int a, int b, double x, Tally& t, const char* what) {
  uint64_t bits;
  memcpy(&bits, &x, 8);
  check(a, b, bits, FIXED6, 17, t, what);
  check(a, b, bits, ROUNDTRIP, 17, t, what);
}

void check_float(int a, int b, float f, Tally& t, const char* what) {
  uint32_t fb;
  memcpy(&fb, &f, 4);
  const double x = (double)f;
  uint64_t want;
  memcpy(&want, &x, 8);
  const uint64_t bits = promote_float_bits(fb);
  // a nan's payload and quiet bit travel the same way through the hardware conversion on the machines this runs on
  if (bits != want && !(std::isnan(f) && ((bits ^ want) & ~(1ull << 51)) == 0)) {
    if (++t.bad <= 10) printf("PROMOTION (%s) float bits %08x: %016llx, (double)f is %016llx\n", what, fb,
                              (unsigned long long)bits, (unsigned long long)want);
    return;
  }
  check(a, b, bits, FIXED6, 9, t, what);
  check(a, b, bits, ROUNDTRIP, 9, t, what);
}

void both(double x, Tally& t, const char* what) {
  check_double(1, 2, x, t, what);
  check_double(1, 2, -x, t, what);
  const float f = (float)x;
  if (std::isnan(x) || (double)f == x || std::isinf(x)) { check_float(1, 2, f, t, what); check_float(1, 2, -f, t, what); }
}

struct Rng {                                          // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  double unit() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

void report(const char* part, const Tally& t) {
  printf("(%s) lines=%lld mismatches=%lld must_fast=%lld fast_missed=%lld slow=%lld longest=%d\n", part, t.lines, t.bad,
         t.must_fast, t.fast_missed, t.slow, t.longest);
}
}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  bool ok = true;

  // ---- (a) the crafted table -------------------------------------------------------------------------------------------
  Tally a;
  both(0.0, a, "zero");
  for (int k = 1; k < 128; k += 2) both(k / 128.0, a, "tie of %.6f: odd k / 128");           // 1/128 -> 0.007812, 3/128 -> 0.023438
  for (int k = 1; k < 64; k += 2) both(1000.0 + k / 128.0, a, "tie above 1000");
  both(0.5, a, "half"); both(1.5, a, "half"); both(2.5, a, "half"); both(0.0000005, a, "half of the last place");
  both(0.9999995, a, "carry into the integer"); both(0.99999949999, a, "below the carry"); both(9.9999995, a, "carry");
  both(999999.9999995, a, "carry"); both(99999999.99999999, a, "carry");
  both(9.9999999e16, a, "carry to 1e17");
  both((double)std::nextafter(1e17f, 0.0f), a, "largest float below 1e17");
  both(std::nextafter(1e17, 0.0), a, "largest double below 1e17");
  both(99999999.5, a, "%.9g carry to 1e+09 by a tie"); both(999999999.0, a, "nine nines"); both(999999999.5, a, "ten digits");
  both(1e-9, a, "-1e-9 -> -0.000000"); both(4.9e-7, a, "rounds to zero"); both(5.1e-7, a, "rounds to 0.000001");
  both(1.0, a, "one"); both(10.0, a, "ten"); both(100.0, a, "hundred"); both(123456789.0, a, "integer");
  both(1e5, a, "1e5"); both(1e-4, a, "fixed style ends"); both(9.9999e-5, a, "exponent style begins");
  both(1e-5, a, "1e-05"); both(0.1, a, "0.1"); both(0.2, a, "0.2"); both(1.0 / 3.0, a, "third"); both(2.0 / 3.0, a, "two thirds");
  both(1e8, a, "below P digits (float)"); both(1e9, a, "P digits (float)"); both(1e16, a, "below P digits"); both(123456.75, a, "fraction");
  for (int p = -15; p <= 16; ++p) {
    const double x = std::pow(10.0, p);
    both(x, a, "power of ten"); both(std::nextafter(x, 0.0), a, "below a power of ten"); both(std::nextafter(x, 1e300), a, "above a power of ten");
    both((double)std::nextafter((float)x, 0.0f), a, "float below a power of ten");
    both((double)std::nextafter((float)x, 1e38f), a, "float above a power of ten");
  }
  // both sides of each class bound
  both(1e15, a, "1e15: FIXED6 bound"); both(std::nextafter(1e15, 0.0), a, "below 1e15"); both(std::nextafter(1e15, 1e300), a, "above 1e15");
  both(999999986991104.0, a, "largest float below 1e15"); both(1000000054099968.0, a, "smallest float above 1e15");
  both(1e17, a, "1e17: ROUNDTRIP bound"); both(std::nextafter(1e17, 1e300), a, "above 1e17");
  both((double)std::nextafter(1e17f, 1e38f), a, "float above 1e17");
  both(1e-15, a, "1e-15: ROUNDTRIP bound"); both(std::nextafter(1e-15, 0.0), a, "below 1e-15"); both(std::nextafter(1e-15, 1.0), a, "above 1e-15");
  both((double)1e-15f, a, "the float 1e-15"); both((double)std::nextafter(1e-15f, 0.0f), a, "float below 1e-15");
  both((double)std::nextafter(1e-15f, 1.0f), a, "float above 1e-15");
  both(1e-16, a, "below the class"); both(1e18, a, "above the class"); both(1e22, a, "1e22"); both(1e300, a, "1e300"); both(1e-300, a, "1e-300");
  // denormals, the largest values, inf and nan: slow, or equal to snprintf if converted
  both(DBL_TRUE_MIN, a, "smallest double denormal"); both(DBL_MIN, a, "DBL_MIN"); both(std::nextafter(DBL_MIN, 0.0), a, "largest double denormal");
  both((double)FLT_TRUE_MIN, a, "smallest float denormal"); both((double)FLT_MIN, a, "FLT_MIN");
  both((double)std::nextafter(FLT_MIN, 0.0f), a, "largest float denormal"); both(3e-39, a, "a float denormal as a double");
  both((double)FLT_MAX, a, "FLT_MAX"); both(DBL_MAX, a, "DBL_MAX");
  both(INFINITY, a, "inf"); both(NAN, a, "nan");
  {
    const int idx[] = {0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000,
                       99999999, 100000000, 999999999, 1000000000, 2147483646, INT_MAX, -1, -9, -10, -2147483647, INT_MIN};
    for (int i : idx)
      for (int j : {0, 7, i, INT_MIN}) { check_double(i, j, 1.0, a, "index"); check_float(j, i, 0.25f, a, "index"); }
  }
  report("a", a);
  ok = ok && a.bad == 0 && a.fast_missed == 0 && a.must_fast > 0 && a.slow > 0;

  // ---- (b) generated values ---------------------------------------------------------------------------------------------
  Tally b;
  Rng r{seed};
  const int N = 2000000;
  for (int i = 0; i < N; ++i) {
    const int ia = (int)(uint32_t)r.next(), ib = (int)(r.next() % 100000);
    if (i & 1) {                                       // random bit patterns
      uint64_t bits = r.next();
      check(ia, ib, bits, FIXED6, 17, b, "random double");
      check(ib, ia, bits, ROUNDTRIP, 17, b, "random double");
      uint32_t fb = (uint32_t)r.next();
      float f;
      memcpy(&f, &fb, 4);
      check_float(ib, ia, f, b, "random float");
    } else {                                           // log-uniform inside the class: FIXED6 1e-8 .. 1e15, ROUNDTRIP 1e-15 .. 1e17
      const double sg = (r.next() & 1) ? -1.0 : 1.0;
      double x = sg * std::pow(10.0, -8.0 + 23.0 * r.unit());
      double y = sg * std::pow(10.0, -15.0 + 32.0 * r.unit());
      if (!(std::fabs(x) < 1e15)) x = sg * 1e14;
      if (!(std::fabs(y) >= 1e-15 && std::fabs(y) < 1e17)) y = sg;
      uint64_t xb, yb;
      memcpy(&xb, &x, 8); memcpy(&yb, &y, 8);
      check(ib, ia, xb, FIXED6, 17, b, "double in the class");
      check(ia, ib, yb, ROUNDTRIP, 17, b, "double in the class");
      uint32_t fx, fy;
      float f = (float)x, g = (float)y;
      memcpy(&fx, &f, 4); memcpy(&fy, &g, 4);
      check(ib, ia, promote_float_bits(fx), FIXED6, 9, b, "float in the class");
      check(ia, ib, promote_float_bits(fy), ROUNDTRIP, 9, b, "float in the class");
    }
  }
  report("b", b);
  ok = ok && b.bad == 0 && b.fast_missed == 0 && b.must_fast > 2 * (long long)N;

  // ---- (c) the line bound -----------------------------------------------------------------------------------------------
  Tally c;
  static_assert(PRINT_LINE_MAX <= 11 + 1 + 11 + 1 + 24 + 1, "the line bound");
  for (double x : {-999999999999999.875, -123456789012345.678, -1.2345678901234567e-5, -1.2345678901234567e-15,
                   -0.00012345678901234567, -9.8765432109876543e16, -12345678.9, -1.0 / 3.0}) {
    check_double(INT_MIN, INT_MIN, x, c, "longest line");
    check_float(INT_MIN, INT_MIN, (float)x, c, "longest line");
  }
  const int longest = std::max(std::max(a.longest, b.longest), c.longest);
  report("c", c);
  printf("    longest line %d bytes, PRINT_LINE_MAX %d\n", longest, PRINT_LINE_MAX);
  ok = ok && c.bad == 0 && c.fast_missed == 0 && longest <= PRINT_LINE_MAX;

  printf(ok ? "PASS\n" : "FAIL\n");
  return ok ? 0 : 1;
}
