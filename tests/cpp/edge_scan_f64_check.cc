// edge_scan_f64_check -- the double scanner (csrc/edge_scan.hpp: scan_double / edge_scan_line_f64) against the C library,
// on the host, stand-alone.
//
//   edge_scan_f64_check.x <seed>        runs (a) and (b) below; exit status 0 only if every condition holds
//
// The reference for every line is parse_edge of csrc/nlibs/COO.cc under FDOUBLE, restated here: strtol, strtol, strtod on
// the line's C string.  Two conditions hold for every line:
//   exact   a line the scanner does not call slow has the reference's field count, indices and the 64 value bits of strtod
//   fast    a value token with at most 19 significant digits (leading zeros not counted, trailing ones counted) and
//           |e10| <= 27 (e10 = exponent - fraction digits) is NOT slow.  The generator knows both numbers of what it
//           writes; they are not taken from the scanner.
//   (a) the crafted table: each row says whether the line must be fast, must be slow, or may be either
//   (b) 2 000 000 seeded random tokens: 1 to 21 significant digits, fixed and scientific notation, leading zeros, trailing
//       fraction zeros, e10 in [-30, 30], both signs
#include "../../sparse_matrix_with_flops_amd/csrc/edge_scan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
struct Parsed { int fields, from, to; uint64_t bits; };

Parsed reference(const std::string& line) {          // parse_edge (csrc/nlibs/COO.cc) with a double value
  Parsed r{0, 0, 0, 0};
  const char* s = line.c_str();
  char* e = nullptr;
  const long a = strtol(s, &e, 10);
  if (e == s) return r;
  const char* s2 = e;
  const long b = strtol(s2, &e, 10);
  if (e == s2) { r.fields = 1; return r; }
  r.from = (int)a; r.to = (int)b;
  const char* s3 = e;
  const double v = strtod(s3, &e);
  if (e == s3) { r.fields = 2; return r; }
  memcpy(&r.bits, &v, 8);
  r.fields = 3;
  return r;
}

enum Speed { FAST, SLOW, EITHER };
struct Tally { long long lines = 0, slow = 0, bad = 0, must_fast = 0, fast_missed = 0, wrong_slow = 0; };

void check(const std::string& line, Speed want, Tally& t, const char* what) {
  ++t.lines;
  if (want == FAST) ++t.must_fast;
  int from = 0, to = 0;
  uint64_t bits = 0;
  // an exact-size copy: a read behind the line's end is a heap overflow the sanitizer build reports
  std::vector<unsigned char> exact(line.begin(), line.end());
  const int got = edgescan::edge_scan_line_f64(exact.data(), (int)exact.size(), &from, &to, &bits);
  if (got == edgescan::EDGE_SLOW) {
    ++t.slow;
    if (want == FAST && ++t.fast_missed <= 10) printf("SLOW, must be fast (%s) \"%s\"\n", what, line.c_str());
    return;
  }
  if (want == SLOW && ++t.wrong_slow <= 10) printf("FAST, must be slow (%s) \"%s\"\n", what, line.c_str());
  const Parsed ref = reference(line);
  const bool same = got == ref.fields && (got < 2 || (from == ref.from && to == ref.to)) && (got < 3 || bits == ref.bits);
  if (!same && ++t.bad <= 10)
    printf("MISMATCH (%s) \"%s\": fields %d vs %d, from %d vs %d, to %d vs %d, bits %016llx vs %016llx\n", what, line.c_str(),
           got, ref.fields, from, ref.from, to, ref.to, (unsigned long long)bits, (unsigned long long)ref.bits);
}

struct Rng {
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Row { const char* value; Speed speed; };
const Row CRAFTED[] = {
    // plain values; "+.e1" has no digit, so the line has 2 fields
    {"0.1", FAST}, {".5", FAST}, {"5.", FAST}, {"-0.0", FAST}, {"0e999", FAST}, {"1e", FAST}, {"1e+", FAST}, {"+.e1", FAST},
    {"3.141592653589793", FAST}, {"0.30000000000000004", FAST}, {"-2.5E-3", FAST}, {"00012.500", FAST}, {"", FAST}, {".", FAST},
    // a float midpoint, and 17 digits: both slow for the float scanner, fast here
    {"16777217.0", FAST}, {"0.10000000000000001", FAST},
    // exact ties between two doubles: to even
    {"9007199254740993", FAST}, {"18014398509481986", FAST}, {"4503599627370496.5", FAST}, {"4503599627370497.5", FAST},
    {"9007199254740995", FAST}, {"9007199254740993.0000000001", EITHER}, {"0.5e-26", FAST},
    // the edges of the fast class
    {"1e27", FAST}, {"1e-27", FAST}, {"9999999999999999999e27", FAST}, {"1234567890123456789", FAST},
    {"9999999999999999999e-27", FAST}, {"1.234567890123456789e9", FAST}, {"18446744073709551615", EITHER},
    // outside it: slow or exact
    {"12345678901234567890", EITHER}, {"1e28", EITHER}, {"1e-28", EITHER}, {"2.2250738585072014e-308", EITHER},
    {"1.7976931348623157e308", EITHER}, {"5e-324", EITHER}, {"1e999", EITHER}, {"1.00000000000000000000", EITHER},
    // slow by text
    {"inf", SLOW}, {"-NaN", SLOW}, {"0x1p3", SLOW}, {"+Infinity", SLOW},
};

// one random value token and whether it lies in the required fast class
std::string random_token(Rng& rng, bool* fast) {
  const int nd = 1 + rng.below(21);
  std::string d;
  for (int i = 0; i < nd; ++i) d += (char)('0' + (i == 0 ? 1 + rng.below(9) : rng.below(10)));
  const int e10 = rng.below(61) - 30;
  const int n = (int)d.size();
  *fast = n <= 19 && e10 >= -27 && e10 <= 27;
  std::string tok = rng.below(2) ? "-" : (rng.below(4) ? "" : "+");
  tok += std::string((size_t)rng.below(3), '0');                              // leading zeros
  if (e10 <= 0 && rng.below(2)) {                                             // fixed notation: -e10 fraction digits
    const int f = -e10;
    if (f >= n) tok += (rng.below(2) ? "0." : ".") + std::string((size_t)(f - n), '0') + d;
    else tok += d.substr(0, (size_t)(n - f)) + (f || rng.below(2) ? "." : "") + d.substr((size_t)(n - f));
  } else {                                                                    // scientific: f fraction digits, exponent e10 + f
    const int f = rng.below(n + 1);
    tok += d.substr(0, (size_t)(n - f));
    if (f || rng.below(2)) tok += "." + d.substr((size_t)(n - f));
    const int ex = e10 + f;
    char buf[32];
    snprintf(buf, sizeof(buf), "%c%s%d", rng.below(2) ? 'e' : 'E', ex >= 0 && rng.below(2) ? "+" : "", ex);
    tok += buf;
  }
  return tok;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: %s <seed>\n", argv[0]); return 2; }
  Rng rng{strtoull(argv[1], nullptr, 10)};
  bool ok = true;

  Tally a;                                                       // (a) the crafted table
  for (const Row& r : CRAFTED) {
    check(std::string("1 2 ") + r.value, r.speed, a, "a");
    if (r.value[0] != '+' && r.value[0] != '-')
      check(std::string("3\t4 -") + r.value + "\r", r.speed, a, "a");           // signed, CR behind it
  }
  check("99999999999999999999 1 0.5", SLOW, a, "a");                           // an index the host clamps
  printf("(a) lines=%lld mismatches=%lld slow=%lld must_fast=%lld fast_missed=%lld wrong_slow=%lld\n", a.lines, a.bad, a.slow,
         a.must_fast, a.fast_missed, a.wrong_slow);
  ok = ok && a.bad == 0 && a.fast_missed == 0 && a.wrong_slow == 0;

  Tally b;                                                       // (b) random tokens
  for (int i = 0; i < 2000000; ++i) {
    bool fast = false;
    const std::string tok = random_token(rng, &fast);
    char head[48];
    snprintf(head, sizeof(head), "%d %d ", rng.below(100000), rng.below(100000));
    check(head + tok, fast ? FAST : EITHER, b, "b");
  }
  printf("(b) lines=%lld mismatches=%lld slow=%lld must_fast=%lld fast_missed=%lld wrong_slow=%lld\n", b.lines, b.bad, b.slow,
         b.must_fast, b.fast_missed, b.wrong_slow);
  ok = ok && b.bad == 0 && b.fast_missed == 0;
  printf(ok ? "PASS\n" : "FAIL\n");
  return ok ? 0 : 1;
}
