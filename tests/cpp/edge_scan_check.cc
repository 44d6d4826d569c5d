// edge_scan_check -- the shared number scanner (csrc/edge_scan.hpp) against the C library, on the host, stand-alone.
//
//   edge_scan_check.x <seed>            runs (a), (b), (c) below; exit status 0 only if every condition holds
//   edge_scan_check.x --table <file>    writes the crafted table of (c) with what strtol / strtol / strtof make of each
//                                       line: "<line as hex> <fields> <from> <to> <value bits> <expected slow>" per row
//
// The reference for every line is parse_edge of csrc/nlibs/COO.cc, restated here: strtol, strtol, strtof on the line's
// C string.  A line the scanner calls slow is not compared (the library hands it to exactly that host code).
//   (a) 1 M lines as tests/test_loader.py:_edge_file writes them, values %.7g of uniform [0,1) floats:
//       zero mismatches AND zero slow lines
//   (b) 1 M values: %.9g of floats over the whole exponent range used here, %.6e scaled by 10^[-30,30], %.17g doubles:
//       zero mismatches among the lines not flagged slow
//   (c) the crafted table: zero mismatches, and the slow flag of every row is the expected one
#include "../../sparse_matrix_with_flops_amd/csrc/edge_scan.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {
struct Parsed { int fields, from, to; uint32_t bits; };

Parsed reference(const std::string& line) {          // parse_edge (csrc/nlibs/COO.cc) on the line's C string
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
  const float v = strtof(s3, &e);
  if (e == s3) { r.fields = 2; return r; }
  memcpy(&r.bits, &v, 4);
  r.fields = 3;
  return r;
}

struct Tally { long long lines = 0, slow = 0, bad = 0; };

// -> true when the scanner called the line slow
bool check(const std::string& line, Tally& t, const char* what) {
  ++t.lines;
  int from = 0, to = 0;
  uint32_t bits = 0;
  // an exact-size copy: a read behind the line's end is a heap overflow the sanitizer build reports
  std::vector<unsigned char> exact(line.begin(), line.end());
  const int got = edgescan::edge_scan_line(exact.data(), (int)exact.size(), &from, &to, &bits);
  if (got == edgescan::EDGE_SLOW) { ++t.slow; return true; }
  const Parsed want = reference(line);
  const bool same = got == want.fields && (got < 2 || (from == want.from && to == want.to)) && (got < 3 || bits == want.bits);
  if (!same) {
    if (++t.bad <= 10)
      printf("MISMATCH (%s) \"%s\": fields %d vs %d, from %d vs %d, to %d vs %d, bits %08x vs %08x\n", what, line.c_str(), got,
             want.fields, from, want.from, to, want.to, bits, want.bits);
  }
  return false;
}

struct Rng {
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }          // uniform [0,1) float
  double unitd() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char* f, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}

struct Row { std::string line; bool slow; };
std::vector<Row> crafted() {
  const std::string v = "1 2 ";
  std::vector<Row> t = {
      // bad or few fields
      {"1 2", false}, {"1", false}, {"1 x", false}, {"1.5 2", false}, {"", false}, {"  \t \r", false},
      // odd index text
      {"1 2.5 7", false}, {"+5 -6 1", false}, {"007 08 1", false}, {"4294967297 0", false}, {"99999999999999999999 1", true},
      // trailing text after the value
      {"1 2 3abc", false}, {"1 2 abc", false},
      // signs, dots, bare exponents
      {v + "-0", false}, {v + "+.5", false}, {v + "5.", false}, {v + ".", false}, {v + "1e", false}, {v + "1e+", false},
      {v + "1E-5", false}, {v + "0e999", false},
      // slow by text
      {v + "0x10", true}, {v + "inf", true}, {v + "-Infinity", true}, {v + "nan", true},
      // slow by range
      {v + "1e-45", true}, {v + "1e39", true}, {v + "3.4028236e38", true}, {v + "0.000000000000000000000001", true},
      {v + "1.00000000000000000000", true},
      // float midpoints: 2^24 + 1 as an integer is exact in double and ties to even; with a fraction part it is scaled
      {v + "16777217", false}, {v + "16777217.0", true}, {v + "16777217.0000001", false},
      // byte level
      {std::string("3 4\0005 6", 7), false}, {"1\t\t2\t.5", false}, {"1\v2\v\v3", false}, {"\f1\f2 \f4", false},
      {"1 2 3\r", false}, {"\r1\r2\r\r7.5\r", false},
  };
  return t;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "--table")) {
    FILE* f = fopen(argv[2], "w");
    if (!f) { printf("cannot write %s\n", argv[2]); return 2; }
    for (const Row& r : crafted()) {
      const Parsed p = reference(r.line);
      if (r.line.empty()) fputs("-", f);
      for (unsigned char c : r.line) fprintf(f, "%02x", c);
      fprintf(f, " %d %d %d %u %d\n", p.fields, p.from, p.to, p.bits, r.slow ? 1 : 0);
    }
    fclose(f);
    return 0;
  }
  if (argc != 2) { printf("usage: %s <seed> | --table <file>\n", argv[0]); return 2; }
  Rng rng{strtoull(argv[1], nullptr, 10)};
  bool ok = true;

  Tally a;                                                       // (a) the loader test's edge lines
  for (int i = 0; i < 1000000; ++i) {
    const int fr = (int)(rng.next() % 50000), to = (int)(rng.next() % 50000);
    const float val = rng.unit();
    const char* eol = (i & 1024) ? "\r" : "";                     // a CRLF file leaves the '\r' in the line
    std::string line;
    if (i % 3 == 0) line = fmt("%d %d %.7g%s", fr, to, val, eol);
    else if (i % 7 == 0) line = fmt("  %d\t%d  %s", fr, to, eol);
    else line = fmt("%d %d%s", fr, to, eol);
    check(line, a, "a");
  }
  printf("(a) lines=%lld mismatches=%lld slow=%lld\n", a.lines, a.bad, a.slow);
  ok = ok && a.bad == 0 && a.slow == 0;

  Tally b;                                                       // (b) values of every width
  for (int i = 0; i < 1000000; ++i) {
    std::string val;
    switch (i % 4) {
      case 0: val = fmt("%.9g", ldexpf(rng.unit() + 0.5f, (int)(rng.next() % 120) - 60)); break;
      case 1: val = fmt("%.9g", -rng.unit()); break;
      case 2: val = fmt("%.6e", (rng.unitd() + 0.1) * pow(10.0, (double)((int)(rng.next() % 61) - 30))); break;
      default: val = fmt("%.17g", rng.unitd() * 1000.0); break;
    }
    check(fmt("%d %d %s", (int)(rng.next() % 1000), (int)(rng.next() % 1000), val.c_str()), b, "b");
  }
  printf("(b) lines=%lld mismatches=%lld slow=%lld\n", b.lines, b.bad, b.slow);
  ok = ok && b.bad == 0;

  Tally c;                                                       // (c) the crafted table
  int wrongFlag = 0;
  for (const Row& r : crafted()) {
    const bool slow = check(r.line, c, "c");
    if (slow != r.slow) { ++wrongFlag; printf("SLOW FLAG \"%s\": %d, expected %d\n", r.line.c_str(), (int)slow, (int)r.slow); }
  }
  printf("(c) lines=%lld mismatches=%lld slow=%lld wrong_slow_flags=%d\n", c.lines, c.bad, c.slow, wrongFlag);
  ok = ok && c.bad == 0 && wrongFlag == 0;
  printf(ok ? "PASS\n" : "FAIL\n");
  return ok ? 0 : 1;
}
