// edges_check.cc -- the C++ mirror's text -> device CSR call, COO::readSNAPFileToGpuCSR (the parse on the device).
//   edges_check.x load  <file> <isTrans 0|1> <cooFlags> <out.bin>
//       out.bin: int32 rows, cols, nnz, then rowPtr[rows + 1], colInd[nnz] (int32), values[nnz] (float32)
//       (tests/test_gpu_edges_parse.py compares it with the oracle's load)
//   edges_check.x bench <file> <isTrans 0|1> <cooFlags> <warmups> <runs>
//       arm A = COO::readSNAPFile + toGpuCSR(cooFlags) (the host threads parse), arm B = readSNAPFileToGpuCSR; first the
//       parity gate (hip_csr_diff at zero tolerances, both CSRs equal or exit status 1 and no times), then `warmups`
//       untimed rounds, then `runs` rounds with the arms taking turns; wall clock ending in a device synchronise.
//       One JSON object on the last line of the output (tools/edges_bench.py).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "COO.h"

namespace {
CSR arm_host(const char* file, bool isTrans, int flags) {
  COO coo;
  coo.readSNAPFile(file, isTrans);
  CSR d = coo.toGpuCSR(flags);
  coo.dispose();
  return d;
}
CSR arm_device(const char* file, bool isTrans, int flags) { return COO::readSNAPFileToGpuCSR(file, isTrans, flags); }

template <class F> double timed_ms(F&& f) {
  const auto t0 = std::chrono::steady_clock::now();
  f();
  spgemm_hip_device_synchronize();
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
void list(std::string& out, const char* name, const std::vector<double>& v) {
  out += std::string("\"") + name + "\": [";
  for (size_t i = 0; i < v.size(); ++i) { char b[32]; snprintf(b, sizeof(b), "%s%.4f", i ? ", " : "", v[i]); out += b; }
  out += "]";
}
}  // namespace

int main(int argc, char* argv[]) {
  if (argc == 6 && !strcmp(argv[1], "load")) {
    CSR d = COO::readSNAPFileToGpuCSR(argv[2], atoi(argv[3]) != 0, atoi(argv[4]));
    CSR h = d.toCpuCSR();
    d.deviceDispose();
    FILE* fp = fopen(argv[5], "wb");
    if (!fp) return 3;
    const int hdr[3] = {h.rows, h.cols, h.nnz};
    fwrite(hdr, sizeof(int), 3, fp);
    fwrite(h.rowPtr, sizeof(int), (size_t)h.rows + 1, fp);
    if (h.nnz > 0) {
      fwrite(h.colInd, sizeof(int), (size_t)h.nnz, fp);
      fwrite(h.values, sizeof(QValue), (size_t)h.nnz, fp);
    }
    fclose(fp);
    const spgemm_edge_stats& st = COO::lastGpuParse;
    printf("device parse: lines=%lld entries=%d slow=%d first_bad=%lld total=%.3f ms\n", st.lines, st.entries, st.slow_lines,
           st.first_bad_line, st.ms_total);
    h.dispose();
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "bench")) {
    const char* file = argv[2];
    const bool isTrans = atoi(argv[3]) != 0;
    const int flags = atoi(argv[4]), warmups = atoi(argv[5]), runs = atoi(argv[6]);
    CSR a = arm_host(file, isTrans, flags), b = arm_device(file, isTrans, flags);
    spgemm_csr_diff diff;
    const bool sameShape = a.rows == b.rows && a.cols == b.cols && a.nnz == b.nnz;
    if (!sameShape || hip_csr_diff(NULL, a.rows, a.cols, b.rowPtr, b.colInd, b.values, b.nnz, a.rowPtr, a.colInd, a.values, a.nnz,
                                   0.0, 0.0, &diff)) {
      printf("parity gate: %s\n", sameShape ? spgemm_hip_last_error() : "shapes differ");
      return 1;
    }
    if (diff.rows_len_differ || diff.only_a || diff.only_b || diff.beyond) {
      printf("parity gate: the two CSRs differ (rows_len_differ=%d only_a=%lld only_b=%lld beyond=%lld)\n", diff.rows_len_differ,
             diff.only_a, diff.only_b, diff.beyond);
      return 1;
    }
    const int rows = a.rows, nnz = a.nnz;
    a.deviceDispose(); b.deviceDispose();
    std::vector<double> msA, msB, up, split, parse, slow, total, hostParse;
    spgemm_edge_stats st = {};
    for (int i = 0; i < warmups + runs; ++i) {
      CSR x, y;
      const double ta = timed_ms([&] { x = arm_host(file, isTrans, flags); });
      const double hp = COO::lastParseMs;
      x.deviceDispose();
      const double tb = timed_ms([&] { y = arm_device(file, isTrans, flags); });
      y.deviceDispose();
      if (i < warmups) continue;
      st = COO::lastGpuParse;
      msA.push_back(ta); msB.push_back(tb); hostParse.push_back(hp);
      up.push_back(st.ms_upload); split.push_back(st.ms_split); parse.push_back(st.ms_parse); slow.push_back(st.ms_slow);
      total.push_back(st.ms_total);
    }
    std::string out = "{";
    char head[256];
    snprintf(head, sizeof(head), "\"rows\": %d, \"nnz\": %d, \"lines\": %lld, \"entries\": %d, \"slow_lines\": %d, \"host_threads\": %d, ",
             rows, nnz, st.lines, st.entries, st.slow_lines, COO::lastParseThreads);
    out += head;
    list(out, "host_arm_ms", msA); out += ", ";
    list(out, "host_arm_read_parse_ms", hostParse); out += ", ";
    list(out, "device_arm_ms", msB); out += ", ";
    list(out, "ms_upload", up); out += ", ";
    list(out, "ms_split", split); out += ", ";
    list(out, "ms_parse", parse); out += ", ";
    list(out, "ms_slow", slow); out += ", ";
    list(out, "ms_total", total);
    out += "}";
    printf("%s\n", out.c_str());
    return 0;
  }
  printf("usage: %s load <file> <isTrans> <cooFlags> <out.bin> | bench <file> <isTrans> <cooFlags> <warmups> <runs>\n", argv[0]);
  return 2;
}
