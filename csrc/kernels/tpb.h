// Block size and grid-size helper of the bandwidth-bound units (input_prep, pool_lrn,
// softmax_ce, splitk_reduce, optimizer).  Together these replace the reference ops of
// SURVEY.md §2.3 N6-N14 (mnist_input.py:37-39,149-172,224-231,252-267,288-290).
#pragma once
#include <stdint.h>

namespace mnistx {
namespace {

constexpr int TPB = 256;

inline int nblocks(int64_t n, int per_block = TPB, int cap = 1 << 20) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}

}  // namespace
}  // namespace mnistx
