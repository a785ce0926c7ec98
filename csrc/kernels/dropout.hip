// Stand-alone dropout for every path the fused LeNet-5 head does not cover (the reference CNN's
// local3 / local4, the mlp model, fuse_head=False, the library modules): inverted dropout in place
// on a [nb, ld] bf16 buffer, the keep bits from the counter-based generator of dropout_rng.h.  No
// mask tensor exists: the backward kernel recomputes the bits of the same (seed, step, layer).
//
// One thread per 16-byte chunk (8 features = one Philox call).  A block is CW chunk columns by
// 256 / CW rows (CW a power of two, so thread -> (row, chunk) is shifts only); rows wider than
// 256 chunks are walked in steps of CW.  The Philox rounds are ~100 VALU instructions (40 of them
// 32-bit multiplies) per 16 bytes read and written.
#include "common.h"
#include "dropout_rng.h"
#include "launchers.h"

namespace mnistx {
namespace {

constexpr int DNT = 256;

// x * inv_keep prepared for ONE rounding to bf16.  The exact product of a bf16 and an fp32 has up to
// 32 significant bits; its fp32 rounding followed by the bf16 rounding differs from rounding the exact
// product once only when the fp32 value landed exactly on a bf16 tie.  The fma gives the exact
// residual, and a tie that is not one moves an fp32 ulp towards the exact product.
DEV float scale_once(float x, float inv_keep) {
  const float p = x * inv_keep;
  const float e = fmaf(x, inv_keep, -p);
  uint32_t b = __float_as_uint(p);
  if ((b & 0xffffu) == 0x8000u && e != 0.f) b += ((e < 0.f) == (p < 0.f)) ? 1u : 0xffffffffu;
  return __uint_as_float(b);
}

// x[m][8g .. 8g + 7] of one chunk: keep ? bf16_rne(x * inv_keep) : +0 by a select, so a dropped NaN
// or infinity is +0.
DEV u32x4 drop_chunk(u32x4 v, const u32x4& w, uint32_t thr, float inv_keep) {
  u32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float lo = keep_lo(w[j], thr) ? scale_once(bf2f(v[j] & 0xffffu), inv_keep) : 0.f;
    const float hi = keep_hi(w[j], thr) ? scale_once(__uint_as_float(v[j] & 0xffff0000u), inv_keep) : 0.f;
    o[j] = pack2(lo, hi);
  }
  return o;
}

DEV void dropout_walk(bf16_t* __restrict__ x, int64_t nb, int n, int ld, const int64_t* __restrict__ step, uint64_t seed,
                      int layer, uint32_t thr, float inv_keep, int cw_log2) {
  const int tid = threadIdx.x, cw = 1 << cw_log2;
  const int64_t m = (int64_t)blockIdx.x * (DNT >> cw_log2) + (tid >> cw_log2);
  if (m >= nb) return;
  const DropKey k = drop_key(step, seed, layer, thr);
  const int chunks = (n + 7) >> 3;
  for (int g = tid & (cw - 1); g < chunks; g += cw) {
    u32x4* p = (u32x4*)(x + m * ld + 8 * g);
    const u32x4 w = drop_draws(k, (uint32_t)m, (uint32_t)g);
    const u32x4 o = drop_chunk(*p, w, thr, inv_keep);
    if (n - 8 * g >= 8) {
      *p = o;
    } else {   // the row's partial chunk: the real features alone are stored
      for (int j = 0; j < n - 8 * g; ++j) x[m * ld + 8 * g + j] = (bf16_t)(o[j >> 1] >> (16 * (j & 1)));
    }
  }
}

__global__ __launch_bounds__(DNT) void dropout_fwd_k(bf16_t* __restrict__ x, int64_t nb, int n, int ld,
                                                     const int64_t* __restrict__ step, uint64_t seed, int layer,
                                                     uint32_t thr, float inv_keep, int cw_log2) {
  dropout_walk(x, nb, n, ld, step, seed, layer, thr, inv_keep, cw_log2);
}

// the same walk over the gradient: dy = keep ? bf16_rne(dy * inv_keep) : +0, the bits recomputed
__global__ __launch_bounds__(DNT) void dropout_bwd_k(bf16_t* __restrict__ dy, int64_t nb, int n, int ld,
                                                     const int64_t* __restrict__ step, uint64_t seed, int layer,
                                                     uint32_t thr, float inv_keep, int cw_log2) {
  dropout_walk(dy, nb, n, ld, step, seed, layer, thr, inv_keep, cw_log2);
}

// the keep bits as bytes, [nb][n] (rows of n bytes: byte stores)
__global__ __launch_bounds__(DNT) void dropout_mask_k(uint8_t* __restrict__ out, int64_t nb, int n,
                                                      const int64_t* __restrict__ step, uint64_t seed, int layer,
                                                      uint32_t thr, int cw_log2) {
  const int tid = threadIdx.x, cw = 1 << cw_log2;
  const int64_t m = (int64_t)blockIdx.x * (DNT >> cw_log2) + (tid >> cw_log2);
  if (m >= nb) return;
  const DropKey k = drop_key(step, seed, layer, thr);
  const int chunks = (n + 7) >> 3;
  for (int g = tid & (cw - 1); g < chunks; g += cw) {
    const u32x4 w = drop_draws(k, (uint32_t)m, (uint32_t)g);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (8 * g + j < n) out[m * n + 8 * g + j] = ((j & 1) ? keep_hi(w[j >> 1], thr) : keep_lo(w[j >> 1], thr)) ? 1 : 0;
  }
}

// chunk columns per block: the power of two covering a row's chunks, 256 at the most
int cw_log2_of(int n) {
  const int chunks = (n + 7) / 8;
  int l = 0;
  while ((1 << l) < chunks && l < 8) ++l;
  return l;
}

bool drop_geometry_ok(int64_t nb, int n, int ld, int layer, uint32_t thr) {
  return nb >= 0 && nb < ((int64_t)1 << 31) && n >= 0 && n <= DROP_MAX_N && ld >= n && ld % 8 == 0 && layer >= 0 &&
         layer < DROP_MAX_LAYER && thr >= 1 && thr <= 65535;
}

template <typename K>
hipError_t launch_walk(K kern, bf16_t* x, int64_t nb, int n, int ld, const int64_t* step, uint64_t seed, int layer,
                       uint32_t thr, float inv_keep, hipStream_t st) {
  if (!drop_geometry_ok(nb, n, ld, layer, thr) || !step) return hipErrorInvalidValue;
  if (nb == 0 || n == 0) return hipSuccess;
  const int l = cw_log2_of(n), rows = DNT >> l;
  hipLaunchKernelGGL(kern, dim3((unsigned)((nb + rows - 1) / rows)), dim3(DNT), 0, st, x, nb, n, ld, step, seed, layer,
                     thr, inv_keep, l);
  return hipGetLastError();
}

}  // namespace

hipError_t dropout_fwd(bf16_t* x, int64_t nb, int n, int ld, const int64_t* step, uint64_t seed, int layer,
                       uint32_t thr, float inv_keep, hipStream_t st) {
  return launch_walk(dropout_fwd_k, x, nb, n, ld, step, seed, layer, thr, inv_keep, st);
}

hipError_t dropout_bwd(bf16_t* dy, int64_t nb, int n, int ld, const int64_t* step, uint64_t seed, int layer,
                       uint32_t thr, float inv_keep, hipStream_t st) {
  return launch_walk(dropout_bwd_k, dy, nb, n, ld, step, seed, layer, thr, inv_keep, st);
}

hipError_t dropout_mask(uint8_t* out, int64_t nb, int n, const int64_t* step, uint64_t seed, int layer, uint32_t thr,
                        hipStream_t st) {
  if (!drop_geometry_ok(nb, n, (n + 7) / 8 * 8, layer, thr) || !step) return hipErrorInvalidValue;
  if (nb == 0 || n == 0) return hipSuccess;
  const int l = cw_log2_of(n), rows = DNT >> l;
  hipLaunchKernelGGL(dropout_mask_k, dim3((unsigned)((nb + rows - 1) / rows)), dim3(DNT), 0, st, out, nb, n, step,
                     seed, layer, thr, l);
  return hipGetLastError();
}

}  // namespace mnistx
