// The epoch shuffle's permutation as device functions, shared by input_prep.hip (its own
// launch, and fused into K10) and the optimizer launch's perm-job blocks (fused_opt_body.h).
#pragma once
#include "common.h"

namespace mnistx {
namespace {

// ------------------------------------------------------------------ epoch shuffle
// Stateless per-epoch permutation: position p of the (endless) sample stream maps
// to dataset row F_e(p mod N), e = p / N, where F_e is a 4-round keyed Feistel
// bijection on [0, 4^h) >= N restricted to [0, N) by cycle walking.  Replaces a
// device randperm (a radix sort: 0.23 ms per 1.08M-entry permutation, 0.70 ms at
// 8 ranks' 8.4M) with ~2 us of integer math per step, and makes the data order a
// pure function of (seed, position): resume seeks instead of replaying.
// data/device_loader.py::perm_positions is the bit-identical torch version.
DEV uint32_t mix32(uint32_t x) {
  x = (x ^ (x >> 16)) * 0x7feb352du;
  x = (x ^ (x >> 15)) * 0x846ca68bu;
  return x ^ (x >> 16);
}
DEV uint64_t feistel4(uint64_t x, const uint32_t* key, int h) {
  const uint64_t mask = (1ull << h) - 1;
  uint64_t L = x >> h, R = x & mask;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint64_t nR = L ^ ((uint64_t)mix32((uint32_t)R ^ key[r]) & mask);
    L = R;
    R = nR;
  }
  return (L << h) | R;
}
// lab_src / lab_out (optional): the labels of the chosen rows gathered in the same
// launch (the resident-dataset input modes need only the index and the labels).
DEV void perm_one(int i, int64_t* __restrict__ out, int64_t start, int n, int64_t N, uint32_t seed, int h,
                  const int32_t* __restrict__ lab_src, int32_t* __restrict__ lab_out) {
  if (i >= n) return;
  const int64_t p = start + i;
  const int64_t e = p / N;
  uint64_t x = (uint64_t)(p - e * N);
  const uint32_t ek = mix32((uint32_t)e ^ 0x9e3779b9u) ^ seed;
  uint32_t key[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) key[r] = mix32(ek + 0x85ebca77u * (uint32_t)(r + 1));
  do { x = feistel4(x, key, h); } while (x >= (uint64_t)N);
  out[i] = (int64_t)x;
  if (lab_out) lab_out[i] = lab_src[x];
}

}  // namespace
}  // namespace mnistx
