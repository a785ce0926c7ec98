// Counter-based randomness for dropout: Philox4x32-10 (Random123 constants).  A keep bit is a
// pure function of (seed, global step, layer, batch row, feature), so there is no RNG state, no
// mask tensor in HBM and nothing to checkpoint; a backward pass recomputes the bits.  One call
// yields the eight 16-bit draws of features 8g .. 8g + 7 of one row:
//   counter = (t & 0xffffffff, t >> 32, m, (L << 16) | g),  key = (seed & 0xffffffff, seed >> 32)
//   draw(f) = (w[(f & 7) >> 1] >> (16 * (f & 1))) & 0xffff,  keep(f) = draw(f) < thr
// with t read from the device-side global step (FlatParams.step) the LR schedule reads.
// ops/dropout.py is the host reference of exactly this.  Plain 32-bit integer math only
// (v_mul_hi_u32 / v_mul_lo_u32, xor, add).
#pragma once
#include "common.h"

namespace mnistx {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

DEV u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(PHILOX_M0, c[0]), l0 = PHILOX_M0 * c[0];
    const uint32_t h1 = __umulhi(PHILOX_M1, c[2]), l1 = PHILOX_M1 * c[2];
    c = u32x4{h1 ^ c[1] ^ k0, l1, h0 ^ c[3] ^ k1, l0};
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return c;
}

// what a launch fixes: the step (read once per thread), the key, the layer word, the threshold
struct DropKey {
  uint32_t t0, t1, k0, k1, lw, thr;
};
DEV DropKey drop_key(const int64_t* __restrict__ step, uint64_t seed, int layer, uint32_t thr) {
  const uint64_t t = (uint64_t)*step;
  return DropKey{(uint32_t)t, (uint32_t)(t >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)layer << 16, thr};
}

// the 8 draws of row m, features 8g .. 8g + 7, as 4 words (two draws each, low half first)
DEV u32x4 drop_draws(const DropKey& k, uint32_t m, uint32_t g) {
  return philox4x32_10(u32x4{k.t0, k.t1, m, k.lw | g}, k.k0, k.k1);
}

// keep bit of the low / high draw of one word
DEV bool keep_lo(uint32_t w, uint32_t thr) { return (w & 0xffffu) < thr; }
DEV bool keep_hi(uint32_t w, uint32_t thr) { return (w >> 16) < thr; }

}  // namespace mnistx
