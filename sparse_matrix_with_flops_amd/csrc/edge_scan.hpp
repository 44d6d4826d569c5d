// edge_scan.hpp -- the number scanner of one edge line "from to [value]", shared by the host and the device.
//
// Plain C++17: it compiles with g++ alone (tests/cpp/edge_scan_check.cc) and, under hipcc, for both sides; EDGE_SCAN_HD
// stands in for __host__ __device__.  Given the bytes of ONE line (without its '\n') edge_scan_line does what parse_edge
// in nlibs/COO.cc does with strtol / strtol / strtof on the line's C string: it returns the number of converted fields
// (0, 1, 2 or 3) with `from`, `to` and the bits of the float value -- or EDGE_SLOW: the line holds a number this scanner
// does not promise to convert like the C library, and goes to the host.
//
// The line as a C string: a NUL byte inside the line ends it.  Whitespace is the C locale's: ' ' \t \n \v \f \r.
// Integers (strtol, base 10): whitespace, an optional sign, at least one digit; up to 18 significant digits accumulate in
//   64 bits and are narrowed as (int)(long) narrows them; 19 or more are slow (strtol would clamp).
// Value (strtof): whitespace, an optional sign, digits with at most one '.', at least one digit; an exponent is consumed
//   only when e/E, an optional sign and at least one digit follow ("1e" and "1e+" are the value 1).  Slow by text: inf /
//   nan (any case) behind the sign, and a 0 followed by x/X (a hex float).
// Conversion: w = the digits without leading zeros, e10 = exponent - number of fraction digits.  w == 0 is +-0.0.
//   w > 2^53 or |e10| > 22 is slow.  Otherwise d = (double)w * 10^e10 or (double)w / 10^-e10: ONE correctly rounded IEEE
//   double operation on two exactly representable operands, so d is the double nearest the decimal.  If e10 != 0 and the
//   low 29 bits of d's mantissa are 1 << 28, d sits exactly on the middle between two floats and the decimal may lie on
//   either side of it: slow.  Otherwise the value is (float)d.
// Why that is strtof bit for bit: a float midpoint is itself a double, so unless d IS that midpoint, the decimal and d, its
// nearest double, lie on the same side of it and round to the same float.  With e10 == 0 d is the decimal itself and the
// conversion's ties-to-even is strtof's.  The float range holds by construction: 1 <= w <= 2^53 and |e10| <= 22 put d
// in [1e-22, 9.1e37], all normal floats.  (Needs IEEE double multiply / divide: the library is built without fast-math.)
#ifndef SMF_EDGE_SCAN_HPP_
#define SMF_EDGE_SCAN_HPP_

#include <stdint.h>
#include <string.h>

#ifndef EDGE_SCAN_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define EDGE_SCAN_HD __host__ __device__
#else
#define EDGE_SCAN_HD
#endif
#endif

namespace edgescan {

constexpr int EDGE_SLOW = -1;

EDGE_SCAN_HD inline bool is_space(unsigned c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
EDGE_SCAN_HD inline bool is_digit(unsigned c) { return c - '0' < 10u; }

// the line's byte i as the C string has it: 0 at and behind the end (a NUL inside ends every token by itself)
struct Line {
  const unsigned char* p;
  int len;
  EDGE_SCAN_HD unsigned at(int i) const { return i < len ? p[i] : 0u; }
};

// strtol(s + i, &end, 10) without its clamp.  -> 1: *out = the value as (int)(long), i moved behind the digits;
// 0: no conversion (i unchanged); EDGE_SLOW: 19 or more significant digits
EDGE_SCAN_HD inline int scan_int(const Line& s, int& i, int* out) {
  int j = i;
  while (is_space(s.at(j))) ++j;
  bool neg = false;
  if (s.at(j) == '+' || s.at(j) == '-') { neg = s.at(j) == '-'; ++j; }
  if (!is_digit(s.at(j))) return 0;
  while (s.at(j) == '0') ++j;
  unsigned long long acc = 0;
  int nd = 0;
  for (; is_digit(s.at(j)); ++j) {
    if (++nd > 18) return EDGE_SLOW;
    acc = acc * 10u + (s.at(j) - '0');
  }
  const long long v = neg ? -(long long)acc : (long long)acc;
  *out = (int)v;
  i = j;
  return 1;
}

EDGE_SCAN_HD inline unsigned lower(unsigned c) { return c | 0x20u; }

// strtof(s + i, &end) on the fast grammar.  -> 1: *bits = the float's bits; 0: no conversion; EDGE_SLOW
EDGE_SCAN_HD inline int scan_float(const Line& s, int i, uint32_t* bits) {
  constexpr double P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                              1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  int j = i;
  while (is_space(s.at(j))) ++j;
  bool neg = false;
  if (s.at(j) == '+' || s.at(j) == '-') { neg = s.at(j) == '-'; ++j; }
  const unsigned c0 = lower(s.at(j)), c1 = lower(s.at(j + 1)), c2 = lower(s.at(j + 2));
  if ((c0 == 'i' && c1 == 'n' && c2 == 'f') || (c0 == 'n' && c1 == 'a' && c2 == 'n')) return EDGE_SLOW;
  if (s.at(j) == '0' && c1 == 'x') return EDGE_SLOW;
  unsigned long long w = 0;
  int sig = 0, frac = 0, digits = 0;
  bool dot = false;
  for (;; ++j) {
    const unsigned c = s.at(j);
    if (c == '.' && !dot) { dot = true; continue; }
    if (!is_digit(c)) break;
    ++digits;
    if (dot) ++frac;
    if (sig > 0 || c != '0') {                       // 19 digits fit 64 bits; beyond that w > 2^53 anyway
      if (++sig <= 19) w = w * 10u + (c - '0');
    }
  }
  if (digits == 0) return 0;
  int ex = 0;
  if (lower(s.at(j)) == 'e') {
    int k = j + 1;
    bool eneg = false;
    if (s.at(k) == '+' || s.at(k) == '-') { eneg = s.at(k) == '-'; ++k; }
    if (is_digit(s.at(k))) {
      for (; is_digit(s.at(k)); ++k)
        if (ex < 100000) ex = ex * 10 + (int)(s.at(k) - '0');     // saturates far beyond what is converted here
      if (eneg) ex = -ex;
    }
  }
  const uint32_t sign = neg ? 0x80000000u : 0u;
  if (sig == 0) { *bits = sign; return 1; }                         // +-0.0 whatever the exponent
  if (sig > 19 || w > (1ull << 53)) return EDGE_SLOW;
  const long long e10 = (long long)ex - frac;
  if (e10 > 22 || e10 < -22) return EDGE_SLOW;
  const double d = e10 >= 0 ? (double)w * P10[e10] : (double)w / P10[-e10];
  uint64_t db;
  memcpy(&db, &d, sizeof(db));
  if (e10 != 0 && (db & 0x1fffffffull) == 0x10000000ull) return EDGE_SLOW;
  const float f = (float)d;
  uint32_t fb;
  memcpy(&fb, &f, sizeof(fb));
  *bits = fb | sign;
  return 1;
}

// One line (bytes [0, len), no '\n' among them).  -> fields converted: 0, 1, 2 (value absent: *vbits untouched) or 3;
// or EDGE_SLOW.  *from / *to are written once both integers are converted, as parse_edge does.
EDGE_SCAN_HD inline int edge_scan_line(const unsigned char* p, int len, int* from, int* to, uint32_t* vbits) {
  const Line s{p, len};
  int i = 0, a = 0, b = 0;
  int rc = scan_int(s, i, &a);
  if (rc <= 0) return rc;                            // 0 fields, or slow
  rc = scan_int(s, i, &b);
  if (rc < 0) return EDGE_SLOW;
  if (rc == 0) return 1;
  *from = a; *to = b;
  rc = scan_float(s, i, vbits);
  if (rc < 0) return EDGE_SLOW;
  return rc == 0 ? 2 : 3;
}

}  // namespace edgescan
#endif
