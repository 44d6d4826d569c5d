// edge_print.hpp -- the number formatter of one edge line "row SEP col SEP value\n", shared by the host and the device: the
// inverse of edge_scan.hpp.
//
// Plain C++17: it compiles with g++ alone (tests/cpp/edge_print_check.cc) and, under hipcc, for both sides; EDGE_PRINT_HD
// stands in for __host__ __device__.  print_line writes what snprintf("%d<sep>%d<sep><value>\n") writes, byte for byte,
// and returns the length -- or PRINT_SLOW: the value is one this formatter does not promise to print like the C library,
// and goes to the host.  No floating-point operation takes part: a value arrives as the 64 bits of a double (a float is
// promoted first, in integers, as printf promotes it), so the build's FP flags cannot change a byte.
//
// Indices: %d of any int, INT_MIN included.
// FIXED6 = "%.6lf", separator '\t' (the line of CSR::output).  Fast: +-0 and every finite |x| < 1e15, denormals included.
//   x = m * 2^e with m < 2^53.  |x| < 1e15 < 2^50 gives e <= -3 for a normal x, so with s = -e >= 1
//     x * 10^6 = N / 2^s,  N = m * 10^6 < 2^73   (the exact integer, 128 bits)
//   and R = N >> s, rounded up when the s bits shifted out are above the half, or on it with R odd: ONE rounding to
//   nearest-even on the exact value, which is what glibc's printf does in the default rounding mode.  s >= 75 shifts all
//   of N out below the half: R = 0.  R < 1e21 + 1 is split by 10^6 with two 64-bit divisions.  The sign is kept when R = 0.
// ROUNDTRIP = "%.9g" for a float, "%.17g" for a double, separator ' ' (reading the text back gives the same bits).  Fast:
//   +-0 and every finite 1e-15 <= |x| < 1e17.  P = 9 or 17 significant digits.  With X' = floor(log10(2^floor(log2|x|))),
//   at most one below X = floor(log10|x|), k = P - 1 - X' puts |x| * 10^k into [10^(P-1), 10^(P+1)):
//     k >= 0 (k <= 32):  |x| * 10^k = m * 5^k * 2^(e+k), m * 5^k < 2^53 * 2^75 = 2^128: the exact integer; one shift right
//                        by -(e+k) with the bits shifted out as half / sticky rounds it (or a shift left, exact);
//     k <  0 (k >= -8, floats of 1e9 and more): |x| / 10^j = m * 2^(e-j) / 5^j, one 64-bit division whose remainder rounds.
//   If the integer part came out with P + 1 digits, X = X' + 1 and the same is done once more with k - 1.  A carry to 10^P
//   becomes 10^(P-1) with X + 1.  %g then prints fixed style for -4 <= X < P and exponent style otherwise, in both without
//   trailing zeros (and without the '.' when no fraction digit is left).
// Slow: inf, nan, and what lies outside those classes.
#ifndef SMF_EDGE_PRINT_HPP_
#define SMF_EDGE_PRINT_HPP_

#include <stdint.h>

#ifndef EDGE_PRINT_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define EDGE_PRINT_HD __host__ __device__
#else
#define EDGE_PRINT_HD
#endif
#endif

namespace edgeprint {

constexpr int PRINT_SLOW = -1;
constexpr int FIXED6 = 0, ROUNDTRIP = 1;             // SPGEMM_EDGE_FMT_FIXED6 / _ROUNDTRIP
constexpr int INDEX_MAX = 11;                        // "-2147483648"
constexpr int VALUE_MAX = 24;                        // FIXED6: '-' 16 digits (999999999999999.9999995 carries) '.' 6 digits;
                                                     // ROUNDTRIP: "-0.000" + 17 digits = 23, "-d." + 16 digits + "e-15" = 23
constexpr int PRINT_LINE_MAX = INDEX_MAX + 1 + INDEX_MAX + 1 + VALUE_MAX + 1;      // a fast line with its '\n': 49

constexpr uint64_t BITS_1E15 = 0x430c6bf526340000ull;        // 1e15 and 1e17 are doubles; the double nearest 1e-15 lies
constexpr uint64_t BITS_1E17 = 0x4376345785d8a000ull;        // above it (1.0000000000000000777e-15), so comparing bits with
constexpr uint64_t BITS_1EM15 = 0x3cd203af9ee75616ull;       // it decides 1e-15 <= |x| for every double x

typedef unsigned __int128 u128;

struct Pow5 {                                        // 5^0 .. 5^27 (5^27 < 2^63)
  uint64_t v[28];
  constexpr Pow5() : v{} {
    uint64_t x = 1;
    for (int k = 0; k < 28; ++k) { v[k] = x; if (k < 27) x *= 5u; }
  }
};
struct Pow10 {                                       // 10^0 .. 10^19
  uint64_t v[20];
  constexpr Pow10() : v{} {
    uint64_t x = 1;
    for (int k = 0; k < 20; ++k) { v[k] = x; if (k < 19) x *= 10u; }
  }
};

// the 64 bits of (double)f for the float with bits fb: what printf's promotion makes of it, in integers
EDGE_PRINT_HD inline uint64_t promote_float_bits(uint32_t fb) {
  const uint64_t sign = (uint64_t)(fb >> 31) << 63;
  const uint32_t ex = (fb >> 23) & 0xffu, fr = fb & 0x7fffffu;
  if (ex == 0xffu) return sign | (0x7ffull << 52) | ((uint64_t)fr << 29);          // inf, nan
  if (ex != 0u) return sign | ((uint64_t)(ex + 896u) << 52) | ((uint64_t)fr << 29);
  if (fr == 0u) return sign;
  const int sh = __builtin_clz(fr) - 8;                                             // a float denormal is a normal double
  return sign | ((uint64_t)(897 - sh) << 52) | ((uint64_t)((fr << sh) & 0x7fffffu) << 29);
}

EDGE_PRINT_HD inline int digits_u32(uint32_t u) {
  return u < 10u ? 1 : u < 100u ? 2 : u < 1000u ? 3 : u < 10000u ? 4 : u < 100000u ? 5 : u < 1000000u ? 6
       : u < 10000000u ? 7 : u < 100000000u ? 8 : u < 1000000000u ? 9 : 10;
}
EDGE_PRINT_HD inline int digits_u64(uint64_t u) {                                   // u < 10^19
  constexpr Pow10 P10;
  int n = 1;
  while (n < 19 && u >= P10.v[n]) ++n;
  return n;
}

EDGE_PRINT_HD inline int int_length(int v) {
  const uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
  return digits_u32(u) + (v < 0 ? 1 : 0);
}

// "%d"
EDGE_PRINT_HD inline int put_int(char* p, int v) {
  uint32_t u = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;
  int n = 0;
  if (v < 0) p[n++] = '-';
  const int nd = digits_u32(u);
  for (int i = nd - 1; i >= 0; --i) { p[n + i] = (char)('0' + u % 10u); u /= 10u; }
  return n + nd;
}

// nd digits of u at p, most significant first (leading zeros if u has fewer)
EDGE_PRINT_HD inline void put_digits(char* p, uint64_t u, int nd) {
  for (int i = nd - 1; i >= 0; --i) { p[i] = (char)('0' + (int)(u % 10u)); u /= 10u; }
}

// A value taken apart, before a byte is written (the length pass stops here).
//   FIXED6:    d = the integer part, nd = its digits, x = the six fraction digits as a number
//   ROUNDTRIP: d = the nd significant digits without trailing zeros, x = the decimal exponent; d == 0 is +-0 (nd = 1)
struct Decimal {
  bool neg;
  uint64_t d;
  int nd, x;
};

EDGE_PRINT_HD inline bool round_up(bool above_half, bool on_half, bool odd) { return above_half || (on_half && odd); }

// FIXED6.  -> false: slow
EDGE_PRINT_HD inline bool take_fixed6(uint64_t bits, Decimal* t) {
  const uint64_t mag = bits & 0x7fffffffffffffffull;
  if (mag >= BITS_1E15) return false;                                               // 1e15 and above, inf, nan
  t->neg = (bits >> 63) != 0;
  const int ex = (int)(mag >> 52);
  const uint64_t fr = mag & 0xfffffffffffffull;
  const uint64_t m = ex ? fr | (1ull << 52) : fr;
  const int s = 1075 - (ex ? ex : 1);                                               // x = m / 2^s, s >= 3 below 1e15
  uint64_t ip = 0, f6 = 0;
  if (m != 0 && s < 75) {
    const u128 N = (u128)m * 1000000u;
    u128 R = N >> s;
    const u128 rem = N & (((u128)1 << s) - 1u), half = (u128)1 << (s - 1);
    if (round_up(rem > half, rem == half, ((uint64_t)R & 1u) != 0)) ++R;
    // R < 2^70 by 10^6: long division on 32-bit digits
    const uint64_t lo = (uint64_t)R, d2 = (uint64_t)(R >> 64);
    const uint64_t n1 = (d2 << 32) | (lo >> 32), q1 = n1 / 1000000u, r1 = n1 % 1000000u;
    const uint64_t n0 = (r1 << 32) | (lo & 0xffffffffull), q0 = n0 / 1000000u;
    f6 = n0 % 1000000u;
    ip = (q1 << 32) + q0;
  }
  t->d = ip; t->nd = digits_u64(ip); t->x = (int)f6;
  return true;
}

// |x| * 10^k for x = m * 2^e, m < 2^53, -8 <= k <= 32: *q = its integer part (when that is below 2^64: the callers' range),
// *up = whether round-to-nearest-even adds one.  -> false: outside what the callers promise
EDGE_PRINT_HD inline bool scale_pow10(uint64_t m, int e, int k, uint64_t* q, bool* up) {
  constexpr Pow5 P5;
  if (k >= 0) {
    if (k > 32) return false;
    u128 N = (u128)m * P5.v[k > 27 ? 27 : k];
    if (k > 27) {                                                                   // times 5^(k-27) <= 5^5: below 2^128
      const uint64_t b = P5.v[k - 27];
      N = (u128)(uint64_t)N * b + ((u128)((uint64_t)(N >> 64) * b) << 64);
    }
    const int sh = e + k;
    if (sh >= 0) {
      if (sh > 63 || (N >> (64 - sh)) != 0) return false;
      *q = (uint64_t)N << sh; *up = false;
      return true;
    }
    const int s = -sh;
    if (s > 127) return false;
    const u128 Q = N >> s;
    if ((Q >> 64) != 0) return false;
    const u128 rem = N & (((u128)1 << s) - 1u), half = (u128)1 << (s - 1);
    *q = (uint64_t)Q;
    *up = round_up(rem > half, rem == half, ((uint64_t)Q & 1u) != 0);
    return true;
  }
  const int j = -k;
  if (j > 27) return false;
  uint64_t num = m, den = P5.v[j];
  const int sh = e - j;
  if (sh >= 0) {
    if (sh > 10) return false;                                                      // m << sh stays below 2^63
    num <<= sh;
  } else {
    if (-sh > 63 - 2 || (den >> (62 + sh)) != 0) return false;                      // den << -sh stays below 2^62
    den <<= -sh;
  }
  const uint64_t Q = num / den, r = num % den;
  *q = Q;
  *up = round_up(2u * r > den, 2u * r == den, (Q & 1u) != 0);
  return true;
}

// ROUNDTRIP with P significant digits (9: a promoted float, 17: a double).  -> false: slow
EDGE_PRINT_HD inline bool take_roundtrip(uint64_t bits, int P, Decimal* t) {
  constexpr Pow10 P10;
  const uint64_t mag = bits & 0x7fffffffffffffffull;
  t->neg = (bits >> 63) != 0;
  if (mag == 0) { t->d = 0; t->nd = 1; t->x = 0; return true; }
  if (mag < BITS_1EM15 || mag >= BITS_1E17) return false;                           // denormals, inf and nan among them
  const uint64_t m = (mag & 0xfffffffffffffull) | (1ull << 52);
  const int e = (int)(mag >> 52) - 1075, b = e + 52;                                // 2^b <= |x| < 2^(b+1), -50 <= b <= 56
  int X = (b * 78913) >> 18;                                                        // floor(b * log10(2)) for |b| < 1650
  uint64_t q = 0;
  bool up = false;
  if (!scale_pow10(m, e, P - 1 - X, &q, &up)) return false;
  if (q >= P10.v[P]) {                                                              // P + 1 digits: the exponent was one short
    ++X;
    if (!scale_pow10(m, e, P - 1 - X, &q, &up)) return false;
  }
  if (q < P10.v[P - 1] || q >= P10.v[P]) return false;                              // never: the estimate is at most one short
  if (up && ++q == P10.v[P]) { q = P10.v[P - 1]; ++X; }
  int nd = P;
  while (q % 10u == 0) { q /= 10u; --nd; }
  t->d = q; t->nd = nd; t->x = X;
  return true;
}

EDGE_PRINT_HD inline bool take_value(uint64_t bits, int fmt, int P, Decimal* t) {
  return fmt == FIXED6 ? take_fixed6(bits, t) : take_roundtrip(bits, P, t);
}

EDGE_PRINT_HD inline bool exponent_style(const Decimal& t, int P) { return t.x < -4 || t.x >= P; }

EDGE_PRINT_HD inline int value_length(const Decimal& t, int fmt, int P) {
  const int sg = t.neg ? 1 : 0;
  if (fmt == FIXED6) return sg + t.nd + 7;
  if (t.d == 0) return sg + 1;
  if (exponent_style(t, P)) return sg + t.nd + (t.nd > 1 ? 1 : 0) + 4;             // |X| <= 17: two exponent digits
  if (t.x < 0) return sg + 1 - t.x + t.nd;                                          // "0." and -X-1 zeros
  return sg + (t.nd > t.x + 1 ? t.nd + 1 : t.x + 1);
}

EDGE_PRINT_HD inline int put_value(char* p, const Decimal& t, int fmt, int P) {
  int n = 0;
  if (t.neg) p[n++] = '-';
  if (fmt == FIXED6) {
    put_digits(p + n, t.d, t.nd);
    n += t.nd;
    p[n++] = '.';
    put_digits(p + n, (uint64_t)t.x, 6);
    return n + 6;
  }
  if (t.d == 0) { p[n++] = '0'; return n; }
  if (exponent_style(t, P)) {
    uint64_t d = t.d;
    for (int i = t.nd - 1; i >= 1; --i) { p[n + 1 + i] = (char)('0' + (int)(d % 10u)); d /= 10u; }
    p[n] = (char)('0' + (int)d);
    n += 1;
    if (t.nd > 1) { p[n] = '.'; n += t.nd; }
    const int ax = t.x < 0 ? -t.x : t.x;
    p[n++] = 'e';
    p[n++] = t.x < 0 ? '-' : '+';
    p[n++] = (char)('0' + ax / 10);
    p[n++] = (char)('0' + ax % 10);
    return n;
  }
  if (t.x < 0) {
    p[n++] = '0'; p[n++] = '.';
    for (int i = 0; i < -t.x - 1; ++i) p[n++] = '0';
    put_digits(p + n, t.d, t.nd);
    return n + t.nd;
  }
  const int ni = t.x + 1;                                                           // digits in front of the '.'
  if (t.nd <= ni) {
    put_digits(p + n, t.d, t.nd);
    for (int i = t.nd; i < ni; ++i) p[n + i] = '0';
    return n + ni;
  }
  uint64_t d = t.d;
  for (int i = t.nd - 1; i >= ni; --i) { p[n + 1 + i] = (char)('0' + (int)(d % 10u)); d /= 10u; }
  p[n + ni] = '.';
  put_digits(p + n, d, ni);
  return n + t.nd + 1;
}

EDGE_PRINT_HD inline char separator(int fmt) { return fmt == FIXED6 ? '\t' : ' '; }

// The length of the line "a SEP b SEP value\n", or PRINT_SLOW.  P: 9 (the bits are a promoted float) or 17; unused by FIXED6.
EDGE_PRINT_HD inline int line_length(int a, int b, uint64_t bits, int fmt, int P) {
  Decimal t;
  if (!take_value(bits, fmt, P, &t)) return PRINT_SLOW;
  return int_length(a) + 1 + int_length(b) + 1 + value_length(t, fmt, P) + 1;
}

// Writes the line at p (room for PRINT_LINE_MAX bytes) and returns its length; PRINT_SLOW: nothing was written.
EDGE_PRINT_HD inline int print_line(char* p, int a, int b, uint64_t bits, int fmt, int P) {
  Decimal t;
  if (!take_value(bits, fmt, P, &t)) return PRINT_SLOW;
  const char sep = separator(fmt);
  int n = put_int(p, a);
  p[n++] = sep;
  n += put_int(p + n, b);
  p[n++] = sep;
  n += put_value(p + n, t, fmt, P);
  p[n++] = '\n';
  return n;
}

}  // namespace edgeprint
#endif
