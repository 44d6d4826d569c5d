// edge_scan.hpp -- the number scanner of one edge line "from to [value]", shared by the host and the device.
//
// Plain C++17: it compiles with g++ alone (tests/cpp/edge_scan_check.cc) and, under hipcc, for both sides; EDGE_SCAN_HD
// stands in for __host__ __device__.  Given the bytes of ONE line (without its '\n') edge_scan_line does what parse_edge
// in nlibs/COO.cc does with strtol / strtol / strtof on the line's C string: it returns the number of converted fields
// (0, 1, 2 or 3) with `from`, `to` and the bits of the float value -- or EDGE_SLOW: the line holds a number this scanner
// does not promise to convert like the C library, and goes to the host.  edge_scan_line_f64 is the same line with a
// double value (strtod, the reference's FDOUBLE build): same tokens, another conversion -- its rule and the argument why
// it equals strtod stand at scan_double below.
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

// The decimal token strtof / strtod would consume at s + i, cut but not yet converted: sign, w = the first 19 significant
// digits, sig = how many significant digits there are, frac = digits behind the '.', ex = the (complete) exponent.
struct Decimal {
  bool neg;
  unsigned long long w;
  int sig, frac, ex;
};

// -> 1: *t filled; 0: no conversion (no digit); EDGE_SLOW: inf / nan / a hex float, slow by text
EDGE_SCAN_HD inline int scan_decimal(const Line& s, int i, Decimal* t) {
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
    if (sig > 0 || c != '0') {                       // 19 digits fit 64 bits; a token with more is slow in both formats
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
  t->neg = neg; t->w = w; t->sig = sig; t->frac = frac; t->ex = ex;
  return 1;
}

// strtof(s + i, &end) on the fast grammar.  -> 1: *bits = the float's bits; 0: no conversion; EDGE_SLOW
EDGE_SCAN_HD inline int scan_float(const Line& s, int i, uint32_t* bits) {
  constexpr double P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                              1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  Decimal t;
  const int rc = scan_decimal(s, i, &t);
  if (rc <= 0) return rc;
  const unsigned long long w = t.w;
  const uint32_t sign = t.neg ? 0x80000000u : 0u;
  if (t.sig == 0) { *bits = sign; return 1; }                       // +-0.0 whatever the exponent
  if (t.sig > 19 || w > (1ull << 53)) return EDGE_SLOW;
  const long long e10 = (long long)t.ex - t.frac;
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

// ---- the double value ---------------------------------------------------------------------------------------------------
// (u1:u0) / v for a v with its top bit set and u1 < v, so that the quotient fits 64 bits: the schoolbook division on
// 32-bit digits (Knuth's algorithm D for a two-digit divisor).  No device has a 128-bit divide; the host uses this one too.
EDGE_SCAN_HD inline uint64_t div128by64(uint64_t u1, uint64_t u0, uint64_t v, uint64_t* rem) {
  const uint64_t b = 1ull << 32, vn1 = v >> 32, vn0 = v & 0xffffffffull, un1 = u0 >> 32, un0 = u0 & 0xffffffffull;
  uint64_t q1 = u1 / vn1, rhat = u1 - q1 * vn1;
  while (q1 >= b || q1 * vn0 > b * rhat + un1) {
    --q1; rhat += vn1;
    if (rhat >= b) break;
  }
  const uint64_t un21 = u1 * b + un1 - q1 * v;                      // modulo 2^64, as the algorithm has it
  uint64_t q0 = un21 / vn1;
  rhat = un21 - q0 * vn1;
  while (q0 >= b || q0 * vn0 > b * rhat + un0) {
    --q0; rhat += vn1;
    if (rhat >= b) break;
  }
  *rem = un21 * b + un0 - q0 * v;
  return q1 * b + q0;
}

EDGE_SCAN_HD inline int clz64(uint64_t x) { return __builtin_clzll(x); }      // x != 0

struct Pow5 {                                                       // 5^0 .. 5^27, computed where it is compiled
  uint64_t v[28];
  constexpr Pow5() : v{} {
    uint64_t x = 1;
    for (int k = 0; k < 28; ++k) { v[k] = x; if (k < 27) x *= 5u; }
  }
};

// the double nearest (m + f) * 2^q, ties to even: m has its top bit set, 0 <= f < 1 and sticky says f != 0.  Normal
// results only (the callers' range).
EDGE_SCAN_HD inline uint64_t round_to_double(uint64_t m, bool sticky, int q) {
  uint64_t mant = m >> 11;                                          // 53 bits
  const uint64_t low = m & 0x7ffull, half = 0x400ull;
  if (low > half || (low == half && (sticky || (mant & 1ull)))) ++mant;
  int e = q + 63;                                                   // the value is 1.xxx * 2^e
  if (mant >> 53) { mant >>= 1; ++e; }
  return ((uint64_t)(e + 1023) << 52) | (mant & ((1ull << 52) - 1ull));
}

// strtod(s + i, &end) on the fast grammar.  -> 1: *bits = the double's 64 bits; 0: no conversion; EDGE_SLOW.
// Same tokens as scan_float.  w == 0 is +-0.0.  More than 19 significant digits or |e10| > 27 is slow.  Otherwise the
// decimal is w * 10^e10 = w * 5^e10 * 2^e10 with 1 <= w < 10^19 < 2^64 and 5^27 < 2^63, and it is rounded ONCE, in integers:
//   e10 >= 0: p = w * 5^e10 < 2^127 is the exact integer.  Shifted left until its top bit is bit 127, its upper 64 bits
//             are m and "the lower 64 are not zero" is the sticky bit.
//   e10 <  0: w' = w << a and d' = 5^-e10 << c, both with the top bit set; (w' << 63) = Q * d' + R by long division, with
//             2^62 <= Q < 2^64 because 1/2 < w'/d' < 2.  The decimal is (Q + R/d') * 2^(c - a + e10 - 63): m = Q (shifted
//             by one if it has 63 bits), and R != 0 is the sticky bit.
// In both cases m holds at least 62 true leading bits of the exact value and sticky says whether anything non-zero lies
// below them, which is all that round-to-nearest-even at 53 bits needs: the result is the correctly rounded double, and
// that is what strtod returns.  The value lies in [1e-27, 1e46): always a normal double, no overflow or underflow case.
// No floating-point operation takes part, so the build's FP flags cannot change a bit.
EDGE_SCAN_HD inline int scan_double(const Line& s, int i, uint64_t* bits) {
  constexpr Pow5 P5;
  static_assert(P5.v[27] == 7450580596923828125ull && P5.v[27] < (1ull << 63), "5^27 fits 63 bits");
  Decimal t;
  const int rc = scan_decimal(s, i, &t);
  if (rc <= 0) return rc;
  const uint64_t sign = t.neg ? 0x8000000000000000ull : 0ull;
  if (t.sig == 0) { *bits = sign; return 1; }                       // +-0.0 whatever the exponent
  if (t.sig > 19) return EDGE_SLOW;
  const long long e10 = (long long)t.ex - t.frac;
  if (e10 > 27 || e10 < -27) return EDGE_SLOW;
  const uint64_t w = t.w;
  if (e10 >= 0) {
    const unsigned __int128 p = (unsigned __int128)w * P5.v[e10];
    const uint64_t hi = (uint64_t)(p >> 64), lo = (uint64_t)p;
    const int lz = hi ? clz64(hi) : 64 + clz64(lo);
    const unsigned __int128 n = p << lz;
    *bits = sign | round_to_double((uint64_t)(n >> 64), (uint64_t)n != 0, (int)e10 + 64 - lz);
  } else {
    const int k = (int)-e10, a = clz64(w), c = clz64(P5.v[k]);
    const uint64_t wn = w << a, dn = P5.v[k] << c;
    uint64_t r;
    uint64_t q = div128by64(wn >> 1, wn << 63, dn, &r);             // wn >> 1 < 2^63 <= dn
    int e2 = c - a - k - 63;
    if (!(q >> 63)) { q <<= 1; --e2; }                              // the bit shifted in is 0; what lies below is in r
    *bits = sign | round_to_double(q, r != 0, e2);
  }
  return 1;
}

EDGE_SCAN_HD inline int scan_value(const Line& s, int i, uint32_t* bits) { return scan_float(s, i, bits); }
EDGE_SCAN_HD inline int scan_value(const Line& s, int i, uint64_t* bits) { return scan_double(s, i, bits); }

// One line (bytes [0, len), no '\n' among them).  -> fields converted: 0, 1, 2 (value absent: *vbits untouched) or 3;
// or EDGE_SLOW.  *from / *to are written once both integers are converted, as parse_edge does.  Bits = uint32_t: the
// value is a float (strtof); uint64_t: a double (strtod).
template <class Bits>
EDGE_SCAN_HD inline int edge_scan_line_as(const unsigned char* p, int len, int* from, int* to, Bits* vbits) {
  const Line s{p, len};
  int i = 0, a = 0, b = 0;
  int rc = scan_int(s, i, &a);
  if (rc <= 0) return rc;                            // 0 fields, or slow
  rc = scan_int(s, i, &b);
  if (rc < 0) return EDGE_SLOW;
  if (rc == 0) return 1;
  *from = a; *to = b;
  rc = scan_value(s, i, vbits);
  if (rc < 0) return EDGE_SLOW;
  return rc == 0 ? 2 : 3;
}

EDGE_SCAN_HD inline int edge_scan_line(const unsigned char* p, int len, int* from, int* to, uint32_t* vbits) {
  return edge_scan_line_as(p, len, from, to, vbits);
}

EDGE_SCAN_HD inline int edge_scan_line_f64(const unsigned char* p, int len, int* from, int* to, uint64_t* vbits) {
  return edge_scan_line_as(p, len, from, to, vbits);
}

}  // namespace edgescan
#endif
