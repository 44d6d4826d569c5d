// edges_write_check.cc -- the C++ mirror's device CSR -> edge-list file call, gpuWriteCSRWrapper (the lines are formatted
// on the device).
//   edges_write_check.x check <file.snap> <out.txt> <fmt 0|1> <header 1|2>
//       load -> rmclInit -> device -> one gpuRmclIterDevice step -> gpuWriteCSRWrapper(out.txt) -> the host loader
//       (COO::readSNAPFile + makeOrdered + toCSR) reads out.txt back -> isEqual with toCpuCSR of the device matrix.
//       Prints "Same" and exits 0, or "Diffs" and exits 1.  (tests/test_gpu_edges_write.py runs it with fmt 1: a
//       ROUNDTRIP text gives the floats back bit for bit; FIXED6 keeps six decimals and isEqual allows 1e-7.)
//   edges_write_check.x bench <csr.bin> <out.txt> <fmt 0|1> <warmups> <runs>
//       csr.bin: int32 rows, cols, nnz, then rowPtr[rows + 1], colInd[nnz] (int32), values[nnz] (float32); it is put on
//       the device once.  arm A = the way a result left before the device writer: toCpuCSR + one fprintf per entry into
//       out.txt behind the size line; arm B = gpuWriteCSRWrapper(out.txt.device, fmt, 1).  First the parity gate (the two
//       files are equal byte for byte, or exit status 1 and no times), then `warmups` untimed rounds, then `runs` rounds
//       with the arms taking turns, wall clock each; arm B's phases from spgemm_edge_write_stats.  One JSON object on the
//       last line of the output (tools/edges_write_bench.py).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "COO.h"
#include "gpus/gpu_csr_kernel.h"
#include "qrmcl.h"

namespace {
double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// Mt after one device iteration from the file's R-MCL start matrix, as a DEVICE CSR
CSR clustered_on_device(const char* file) {
  COO coo;
  coo.readSNAPFile(file);
  CSR M0 = rmclInit(coo);
  coo.dispose();
  CSR dM0 = M0.toGpuCSR();
  M0.dispose();
  CSR dMt = gpuRmclIterDevice(1, dM0, dM0);
  dM0.deviceDispose();
  return dMt;
}

bool host_write(const CSR& dA, const char* path, int fmt) {
  CSR h = dA.toCpuCSR();
  FILE* fp = fopen(path, "w");
  if (!fp) return false;
  fprintf(fp, "%d %d %d\n", h.rows, h.cols, h.nnz);
  for (int r = 0; r < h.rows; ++r)
    for (int p = h.rowPtr[r]; p < h.rowPtr[r + 1]; ++p) {
      if (fmt == SPGEMM_EDGE_FMT_FIXED6) fprintf(fp, "%d\t%d\t%.6lf\n", r, h.colInd[p], (double)h.values[p]);
      else fprintf(fp, "%d %d %.9g\n", r, h.colInd[p], (double)h.values[p]);
    }
  const bool ok = fclose(fp) == 0;
  h.dispose();
  return ok;
}

std::vector<char> slurp(const std::string& path) {
  std::vector<char> out;
  FILE* fp = fopen(path.c_str(), "rb");
  if (!fp) return out;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, fp)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(fp);
  return out;
}
}  // namespace

int main(int argc, char* argv[]) {
  if (argc == 6 && !strcmp(argv[1], "check")) {
    const int fmt = atoi(argv[4]), header = atoi(argv[5]);
    CSR dMt = clustered_on_device(argv[2]);
    gpuWriteCSRWrapper(dMt, argv[3], fmt, header);
    CSR want = dMt.toCpuCSR();
    dMt.deviceDispose();
    COO back;
    back.readSNAPFile(argv[3], false);
    back.makeOrdered();
    CSR got = back.toCSR();
    back.dispose();
    const bool same = got.isEqual(want);
    printf("rows=%d nnz=%d read back rows=%d nnz=%d\n%s\n", want.rows, want.nnz, got.rows, got.nnz, same ? "Same" : "Diffs");
    got.dispose();
    want.dispose();
    return same ? 0 : 1;
  }
  if (argc == 7 && !strcmp(argv[1], "bench")) {
    const int fmt = atoi(argv[4]), warmups = atoi(argv[5]), runs = atoi(argv[6]);
    const std::string out = argv[3], dev = out + ".device";
    FILE* fp = fopen(argv[2], "rb");
    int hdr[3];
    if (!fp || fread(hdr, sizeof(int), 3, fp) != 3) return 3;
    CSR h;
    h.rows = hdr[0]; h.cols = hdr[1]; h.nnz = hdr[2];
    h.rowPtr = (int*)malloc(sizeof(int) * ((size_t)h.rows + 1));
    h.colInd = (int*)malloc(sizeof(int) * (size_t)(h.nnz > 0 ? h.nnz : 1));
    h.values = (QValue*)malloc(sizeof(QValue) * (size_t)(h.nnz > 0 ? h.nnz : 1));
    if (fread(h.rowPtr, sizeof(int), (size_t)h.rows + 1, fp) != (size_t)h.rows + 1 ||
        fread(h.colInd, sizeof(int), (size_t)h.nnz, fp) != (size_t)h.nnz ||
        fread(h.values, sizeof(QValue), (size_t)h.nnz, fp) != (size_t)h.nnz) return 3;
    fclose(fp);
    CSR d = h.toGpuCSR();
    h.dispose();
    spgemm_edge_write_stats st;
    auto device_write = [&] {
      if (hip_write_edge_file(NULL, dev.c_str(), d.rows, d.cols, d.rowPtr, d.colInd, d.values, fmt, 0, 1, &st)) {
        printf("hip_write_edge_file: %s\n", spgemm_hip_last_error());
        exit(1);
      }
    };
    if (!host_write(d, out.c_str(), fmt)) return 3;
    device_write();
    const std::vector<char> a = slurp(out), b = slurp(dev);
    if (a.empty() || a != b) { printf("parity gate: the two files differ (%zu and %zu bytes)\n", a.size(), b.size()); return 1; }
    const char* keys[] = {"host_arm_ms", "device_arm_ms", "ms_length", "ms_scan", "ms_write", "ms_slow", "ms_download", "ms_file", "ms_total"};
    std::vector<std::vector<double>> t(9);
    for (int i = 0; i < warmups + runs; ++i) {
      auto t0 = std::chrono::steady_clock::now();
      if (!host_write(d, out.c_str(), fmt)) return 3;
      const double ta = ms_since(t0);
      t0 = std::chrono::steady_clock::now();
      device_write();
      const double tb = ms_since(t0);
      if (i < warmups) continue;
      const double v[9] = {ta, tb, st.ms_length, st.ms_scan, st.ms_write, st.ms_slow, st.ms_download, st.ms_file, st.ms_total};
      for (int k = 0; k < 9; ++k) t[k].push_back(v[k]);
    }
    remove(dev.c_str());
    remove(out.c_str());
    std::string js = "{";
    char head[256];
    snprintf(head, sizeof head, "\"rows\": %d, \"nnz\": %d, \"bytes\": %zu, \"slabs\": %d, \"slow_entries\": %lld", d.rows, d.nnz,
             a.size(), st.slabs, st.slow_entries);
    js += head;
    for (int k = 0; k < 9; ++k) {
      js += std::string(", \"") + keys[k] + "\": [";
      for (size_t i = 0; i < t[k].size(); ++i) { char x[32]; snprintf(x, sizeof x, "%s%.4f", i ? ", " : "", t[k][i]); js += x; }
      js += "]";
    }
    printf("%s}\n", js.c_str());
    d.deviceDispose();
    return 0;
  }
  printf("usage: %s check <file> <out> <fmt> <header> | bench <csr.bin> <out> <fmt> <warmups> <runs>\n", argv[0]);
  return 2;
}
