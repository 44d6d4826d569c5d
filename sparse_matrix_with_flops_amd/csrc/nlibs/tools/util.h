// tools/util.h — mirror of the permutation helpers of the reference's nlibs/tools/util.h:29-30 (util.cc:151-168).
// The inverse is computed on the device (hip_permutation_transpose), which also rejects a P that is no permutation.
#ifndef SMF_TOOLS_UTIL_H_
#define SMF_TOOLS_UTIL_H_
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <utility>
#include "../../../../include/spgemm_hip.h"

// int* permutationTranspose(const int P[], const int len) (nlibs/tools/util.cc:162-168): malloc()ed Pt, Pt[P[i]] = i
inline int* permutationTranspose(const int P[], const int len) {
  const size_t bytes = sizeof(int) * (size_t)(len > 0 ? len : 1);
  int* Pt = (int*)malloc(bytes);
  int *dP = 0, *dPt = 0;
  if (!Pt || spgemm_hip_malloc((void**)&dP, bytes) || spgemm_hip_malloc((void**)&dPt, bytes) ||
      (len > 0 && spgemm_hip_memcpy_h2d(dP, P, sizeof(int) * (size_t)len)) || hip_permutation_transpose(0, len, dP, dPt) ||
      (len > 0 && spgemm_hip_memcpy_d2h(Pt, dPt, sizeof(int) * (size_t)len))) {
    printf("permutationTranspose: %s\n", Pt ? spgemm_hip_last_error() : "out of host memory");
    exit(EXIT_FAILURE);
  }
  spgemm_hip_free(dP);
  spgemm_hip_free(dPt);
  return Pt;
}

// int* randomPermutationVector(const int len) (nlibs/tools/util.cc:151-160) with the seed as an argument, so that a run
// can be repeated: malloc()ed uniform random permutation of 0..len-1
inline int* randomPermutationVector(const int len, const unsigned seed = 1) {
  int* P = (int*)malloc(sizeof(int) * (size_t)(len > 0 ? len : 1));
  if (!P) { printf("randomPermutationVector: out of host memory\n"); exit(EXIT_FAILURE); }
  std::iota(P, P + len, 0);
  std::mt19937 gen(seed);
  for (int i = len - 1; i > 0; --i) std::swap(P[i], P[std::uniform_int_distribution<int>(0, i)(gen)]);
  return P;
}
#endif
