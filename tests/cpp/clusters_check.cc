// tests/cpp/clusters_check.cc — clusters of an R-MCL result through this project's C++ mirror, on the device.
//   clusters_check.x <edge list> [iterations, default 10]
//   load, rmclInit, to the device, gpuRmclIterDevice, gpuRmclClusters; the result is downloaded and the same clusters are
//   made on the host: per row the column of the largest value (the smaller column on a tie, the row itself when nothing
//   wins), a union-find over i -- parent[i] that hangs the larger root under the smaller, clusters numbered by ascending
//   smallest member.  Also gpuConnectedComponents of the result's pattern against the same union-find over its entries.
//   Prints the counts, then "Same" or "Diffs"; exit code 0 iff Same.
//   clusters_check.x bench flow|graph <binary CSR> <warmup> <reps>      (tools/clusters_bench.py)
//   the file: rows, cols, nnz, then rowPtr, colInd (int32) and values (float32).  The host way (download, argmax per row
//   for `flow`, union-find, numbering) and the device entries take turns, each under the host clock around the blocking
//   call; `flow` times the four entries on a flow matrix, `graph` the components and the labels -> clusters step on a
//   pattern.  The two ways must agree or the run fails.  One JSON line with the milliseconds of every repetition.
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/spgemm_hip.h"
#include "COO.h"
#include "CSR.h"
#include "gpus/gpu_csr_kernel.h"
#include "qrmcl.h"

struct UnionFind {
  std::vector<int> f;
  explicit UnionFind(int m) : f((size_t)m) { for (int i = 0; i < m; ++i) f[(size_t)i] = i; }
  int find(int x) {
    int r = x;
    while (f[(size_t)r] != r) r = f[(size_t)r];
    while (f[(size_t)x] != r) { const int next = f[(size_t)x]; f[(size_t)x] = r; x = next; }
    return r;
  }
  void join(int a, int b) {
    a = find(a); b = find(b);
    if (a != b) f[(size_t)(a > b ? a : b)] = a > b ? b : a;     // a root is the smallest vertex of its tree
  }
  std::vector<int> labels() {
    std::vector<int> l(f.size());
    for (size_t v = 0; v < f.size(); ++v) l[v] = find((int)v);
    return l;
  }
};

// per vertex the number of its cluster, clusters numbered by ascending smallest member (= ascending root)
static std::vector<int> number_clusters(const std::vector<int>& label, int* k) {
  std::vector<int> rank(label.size()), cluster(label.size());
  int n = 0;
  for (size_t v = 0; v < label.size(); ++v) rank[v] = label[v] == (int)v ? n++ : -1;
  for (size_t v = 0; v < label.size(); ++v) cluster[v] = rank[(size_t)label[v]];
  *k = n;
  return cluster;
}

// the host way on a downloaded matrix: flow = true takes the argmax edge of every row, else every stored entry
static std::vector<int> host_clusters(const CSR& M, bool flow, std::vector<int>* label, int* k) {
  UnionFind uf(M.rows);
  for (int i = 0; i < M.rows; ++i) {
    QValue bv = -INFINITY;
    int bc = INT_MAX;
    for (int p = M.rowPtr[i]; p < M.rowPtr[i + 1]; ++p) {
      const QValue v = M.values[p];
      const int c = M.colInd[p];
      if (!flow) uf.join(i, c);
      else if (v > bv || (v == bv && c < bc)) { bv = v; bc = c; }
    }
    if (flow && bc != INT_MAX) uf.join(i, bc);
  }
  *label = uf.labels();
  return number_clusters(*label, k);
}

static void die_on(int rc, const char* what) {
  if (rc) { printf("%s: %s\n", what, spgemm_hip_last_error()); exit(EXIT_FAILURE); }
}

static double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

static std::vector<int> download(const int* d, size_t n) {
  std::vector<int> h(n);
  if (n) die_on(spgemm_hip_memcpy_d2h(h.data(), d, sizeof(int) * n), "download");
  return h;
}

static int bench(const char* kind, const char* path, int warmup, int reps) {
  const bool flow = !strcmp(kind, "flow");
  FILE* f = fopen(path, "rb");
  int hdr[3];
  if (!f || fread(hdr, sizeof(int), 3, f) != 3) { printf("cannot read %s\n", path); return 2; }
  const int m = hdr[0], nnz = hdr[2];
  std::vector<int> rp((size_t)m + 1), ci((size_t)nnz);
  std::vector<QValue> va((size_t)nnz);
  if (fread(rp.data(), sizeof(int), rp.size(), f) != rp.size() || fread(ci.data(), sizeof(int), ci.size(), f) != ci.size() ||
      fread(va.data(), sizeof(float), va.size(), f) != va.size()) { printf("short file %s\n", path); return 2; }
  fclose(f);
  CSR hM;
  hM.rowPtr = rp.data(); hM.colInd = ci.data(); hM.values = va.data(); hM.rows = hM.cols = m; hM.nnz = nnz;
  CSR dM = hM.toGpuCSR();
  int *dParent = 0, *dIota = 0, *dLabel = 0;
  die_on(spgemm_hip_malloc((void**)&dParent, sizeof(int) * ((size_t)m + 1)), "malloc");
  die_on(spgemm_hip_malloc((void**)&dIota, sizeof(int) * ((size_t)m + 1)), "malloc");
  die_on(spgemm_hip_malloc((void**)&dLabel, sizeof(int) * ((size_t)m + 1)), "malloc");
  std::vector<int> iota((size_t)m + 1);
  for (int i = 0; i <= m; ++i) iota[(size_t)i] = i;
  die_on(spgemm_hip_memcpy_h2d(dIota, iota.data(), sizeof(int) * iota.size()), "upload");
  std::vector<double> tHost, tAttr, tComp, tL2c, tChain;
  int rounds = 0, k = 0, hostK = 0, ncomp = 0;
  bool same = true;
  for (int it = 0; it < warmup + reps; ++it) {
    const bool keep = it >= warmup;
    // what a user does today: the matrix to the host, then the host loop
    auto t = std::chrono::steady_clock::now();
    CSR down = dM.toCpuCSR();
    std::vector<int> hostLabel;
    const std::vector<int> hostCluster = host_clusters(down, flow, &hostLabel, &hostK);
    if (keep) tHost.push_back(ms_since(t));
    down.dispose();
    const int *cIA = dM.rowPtr, *cJA = dM.colInd;
    int cnnz = nnz;
    if (flow) {
      t = std::chrono::steady_clock::now();
      die_on(hip_rmcl_attractors(NULL, m, m, nnz, dM.rowPtr, dM.colInd, dM.values, dParent), "hip_rmcl_attractors");
      if (keep) tAttr.push_back(ms_since(t));
      cIA = dIota; cJA = dParent; cnnz = m;
    }
    t = std::chrono::steady_clock::now();
    die_on(hip_csr_connected_components(NULL, m, m, cnnz, cIA, cJA, dLabel, &ncomp, &rounds), "hip_csr_connected_components");
    if (keep) tComp.push_back(ms_since(t));
    int *dC = 0, *dP = 0, *dMem = 0;
    t = std::chrono::steady_clock::now();
    die_on(hip_labels_to_clusters(NULL, m, dLabel, &k, &dC, &dP, &dMem), "hip_labels_to_clusters");
    if (keep) tL2c.push_back(ms_since(t));
    same = same && k == hostK && download(dLabel, (size_t)m) == hostLabel && download(dC, (size_t)m) == hostCluster;
    spgemm_hip_free(dC); spgemm_hip_free(dP); spgemm_hip_free(dMem);
    if (flow) {
      t = std::chrono::steady_clock::now();
      die_on(hip_rmcl_clusters(NULL, m, m, nnz, dM.rowPtr, dM.colInd, dM.values, &k, &dC, &dP, &dMem), "hip_rmcl_clusters");
      if (keep) tChain.push_back(ms_since(t));
      same = same && k == hostK && download(dC, (size_t)m) == hostCluster;
      spgemm_hip_free(dC); spgemm_hip_free(dP); spgemm_hip_free(dMem);
    }
  }
  spgemm_hip_free(dParent); spgemm_hip_free(dIota); spgemm_hip_free(dLabel);
  dM.deviceDispose();
  if (!same) { printf("Diffs\n"); return 1; }
  const auto list = [](const std::vector<double>& v) {
    std::string s = "[";
    char buf[32];
    for (size_t i = 0; i < v.size(); ++i) { snprintf(buf, sizeof(buf), "%s%.4f", i ? ", " : "", v[i]); s += buf; }
    return s + "]";
  };
  printf("{\"rows\": %d, \"nnz\": %d, \"clusters\": %d, \"components\": %d, \"rounds\": %d, \"host_ms\": %s, "
         "\"components_ms\": %s, \"labels_to_clusters_ms\": %s, \"attractors_ms\": %s, \"rmcl_clusters_ms\": %s}\n",
         m, nnz, k, ncomp, rounds, list(tHost).c_str(), list(tComp).c_str(), list(tL2c).c_str(), list(tAttr).c_str(),
         list(tChain).c_str());
  return 0;
}

int main(int argc, char* argv[]) {
  if (argc == 6 && !strcmp(argv[1], "bench")) return bench(argv[2], argv[3], atoi(argv[4]), atoi(argv[5]));
  if (argc < 2 || argc > 3) { printf("usage: clusters_check.x <edge list> [iterations]\n"); return 2; }
  const int iters = argc == 3 ? atoi(argv[2]) : 10;
  COO cooAt;
  cooAt.readSNAPFile(argv[1], true);
  CSR Mt = rmclInit(cooAt);
  cooAt.dispose();
  CSR dMt = Mt.toGpuCSR();
  CSR dOut = gpuRmclIterDevice(iters, dMt, dMt);
  int k = 0;
  const std::vector<int> cluster = gpuRmclClusters(dOut, &k);
  const std::vector<int> comp = gpuConnectedComponents(dOut);
  CSR out = dOut.toCpuCSR();

  // what a user did before: the flow matrix on the host, argmax per row, union-find
  int wantK = 0, unused = 0;
  std::vector<int> flowLabel, wantComp;
  const std::vector<int> want = host_clusters(out, true, &flowLabel, &wantK);
  host_clusters(out, false, &wantComp, &unused);
  long differ = k != wantK, differComp = 0;
  for (size_t v = 0; v < want.size(); ++v) {
    differ += cluster[v] != want[v];
    differComp += comp[v] != wantComp[v];
  }
  printf("m=%d nnz(Mt)=%d iterations=%d clusters=%d (host %d)\n", out.rows, out.nnz, iters, k, wantK);
  printf("cluster numbers that differ: %ld, component labels that differ: %ld\n", differ, differComp);
  const bool same = differ == 0 && differComp == 0;
  printf("%s\n", same ? "Same" : "Diffs");
  out.dispose(); dOut.deviceDispose(); dMt.deviceDispose(); Mt.dispose();
  return same ? 0 : 1;
}
