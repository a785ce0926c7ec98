// Mixup and CutMix of a training batch, in place on the loader's output buffer [nb, 784, C] bf16
// (whatever wrote it: prep_images, prep_images_perm, augment_images or its elastic form), plus the
// second label and the weight of every row for the MIX form of the softmax cross-entropy kernels.
//
// The partner of batch entry b is entry nb - 1 - b (the batch flip).  The draw of entry b is a pure
// function of (seed, p), p = pos0 + b its global stream position: one Philox4x32-10 call
// (dropout_rng.h), every floating-point line one rounded fp32 operation (no contraction: mix_draw)
//   counter = (p & 0xffffffff, p >> 32, 0, 0x41554702),  key = (seed & 0xffffffff, seed >> 32)
//   apply = (w0 >> 16) < thr_p;   cut = cutmix on and (mixup off or (w0 & 1))
//   mixup:  u = float(w1 >> 8) * 2^-24, pos = u * 1024, k = int(pos), fr = pos - k       (all exact)
//           d = T[k + 1] - T[k];  lam = T[k] + fr * d
//   cutmix: side = S[w1 >> 22];  cx = umulhi(w2, 28);  cy = umulhi(w3, 28)
//           x0 = max(cx - side / 2, 0);  x1 = min(cx - side / 2 + side, 28)   (same in y)
//           area = (x1 - x0) (y1 - y0);  lam = float(784 - area) / 784.0f
// T (1025 fp32 quantiles of Beta(a, a) on its upper half) and S (1024 box sides) are the HOST's
// tables (data/mix.py lam_table / side_table): the device knows nothing about Beta and takes no
// square root.  An entry is unmixed when apply is false, when it is its own partner or when its box
// is empty: its bytes are not touched, lam = 1, its second label is its own.  Otherwise, with xa the
// entry's value and xb the partner's as the buffer held them before the launch:
//   mixup:   om = 1 - lam;  t = om * xb;  out = bf16_rne(fmaf(lam, xa, t))
//   cutmix:  out = xb inside the box (a bitwise copy, all channels of a pixel), xa outside
// data/mix.py is the host reference of exactly this (params bit for bit, mixed in float64).
//
// A thread owns the same 16-byte chunk of entry b and of entry nb - 1 - b, b < nb / 2: it loads
// both, forms both outputs from the two loaded vectors and stores both, so in place needs no second
// buffer and no ordering between threads.  A block walks groups of MIX_G pairs; one lane per entry
// draws (Philox, the table lookups) and hands kind, lam and box to the pair's threads through LDS,
// as the affine augmentation does.  The pair's first thread writes labels2 and lam of both entries.
// A pair with both sides unmixed (and the middle entry of an odd batch) moves no image bytes.
#include "common.h"
#include "dropout_rng.h"
#include "launchers.h"

namespace mnistx {
namespace {

constexpr int MIX_NT = 256;
constexpr int MIX_G = 16;                   // pairs per block iteration
constexpr uint32_t MIX_TAG = 0x41554702u;   // counter word 3: continues the augmentation's tags
constexpr int MIX_UNMIXED = 0, MIX_MIXUP = 1, MIX_CUTMIX = 2;

struct MixDraw {
  int kind;
  float lam;
  int x0, x1, y0, y1;
};

// The draw of stream position p.  T / S: the mixup / CutMix table, nullptr = that form is off.  Both
// kernels call this; contraction is off so that every line is the single rounded fp32 operation the
// host reference performs.
DEV MixDraw mix_draw(uint64_t p, uint64_t seed, uint32_t thr_p, const float* __restrict__ T,
                     const int32_t* __restrict__ S) {
#pragma clang fp contract(off)
  const u32x4 w = philox4x32_10(u32x4{(uint32_t)p, (uint32_t)(p >> 32), 0u, MIX_TAG}, (uint32_t)seed,
                                (uint32_t)(seed >> 32));
  MixDraw d{MIX_UNMIXED, 1.f, 0, 0, 0, 0};
  if (!((w[0] >> 16) < thr_p)) return d;
  const bool cut = S && (!T || (w[0] & 1u));
  if (!cut) {
    const float u = (float)(w[1] >> 8) * 5.9604644775390625e-8f;   // 2^-24
    const float pos = u * 1024.f;
    const int k = (int)pos;
    const float fr = pos - (float)k;
    const float t0 = T[k], t1 = T[k + 1];
    const float dd = t1 - t0;
    const float inc = fr * dd;
    d.kind = MIX_MIXUP;
    d.lam = t0 + inc;
    return d;
  }
  const int side = S[w[1] >> 22];
  const int cx = (int)__umulhi(w[2], 28u), cy = (int)__umulhi(w[3], 28u);
  const int x0 = max(cx - side / 2, 0), x1 = min(cx - side / 2 + side, 28);
  const int y0 = max(cy - side / 2, 0), y1 = min(cy - side / 2 + side, 28);
  const int area = (x1 - x0) * (y1 - y0);
  if (area == 0) return d;
  d.kind = MIX_CUTMIX;
  d.lam = (float)(784 - area) / 784.f;   // one IEEE division
  d.x0 = x0;
  d.x1 = x1;
  d.y0 = y0;
  d.y1 = y1;
  return d;
}

// One 16-byte chunk (elements 8 c .. 8 c + 7 of an image of C channels) of a mixed entry: va its own
// values, vb the partner's; prm = (kind, the bits of lam, x0 | x1 << 8 | y0 << 16 | y1 << 24, -).
template <int C>
DEV u32x4 mix_chunk(const u32x4& va, const u32x4& vb, const u32x4& prm, int c) {
#pragma clang fp contract(off)
  u32x4 o;
  if ((int)prm[0] == MIX_MIXUP) {
    const float lam = __uint_as_float(prm[1]);
    const float om = 1.f - lam;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t0 = om * bf2f(vb[j] & 0xffffu), t1 = om * __uint_as_float(vb[j] & 0xffff0000u);
      o[j] = pack2(fmaf(lam, bf2f(va[j] & 0xffffu), t0), fmaf(lam, __uint_as_float(va[j] & 0xffff0000u), t1));
    }
    return o;
  }
  const int x0 = prm[2] & 0xff, x1 = (prm[2] >> 8) & 0xff, y0 = (prm[2] >> 16) & 0xff, y1 = prm[2] >> 24;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t w = va[j];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int pix = (8 * c + 2 * j + k) / C, row = pix / 28, col = pix - 28 * row;
      const bool in = col >= x0 && col < x1 && row >= y0 && row < y1;
      const uint32_t m = k ? 0xffff0000u : 0x0000ffffu;
      w = in ? ((w & ~m) | (vb[j] & m)) : w;
    }
    o[j] = w;
  }
  return o;
}

template <int C>
__global__ __launch_bounds__(MIX_NT) void mix_images_k(bf16_t* __restrict__ img, const int32_t* __restrict__ labels,
                                                       int32_t* __restrict__ labels2, float* __restrict__ lam, int nb,
                                                       int64_t pos0, uint64_t seed, uint32_t thr_p,
                                                       const float* __restrict__ T, const int32_t* __restrict__ S) {
  constexpr int CH = 784 * C / 8;           // 16-byte chunks of an entry
  __shared__ u32x4 prm[2 * MIX_G];          // [2 g]: entry u, [2 g + 1]: its partner nb - 1 - u
  const int tid = threadIdx.x;
  const int nunits = (nb + 1) / 2;          // the pairs, and the middle entry of an odd batch (its own partner)
  const int ngroups = (nunits + MIX_G - 1) / MIX_G;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int u0 = grp * MIX_G;
    const int ng = nunits - u0 < MIX_G ? nunits - u0 : MIX_G;
    if (tid < 2 * ng) {   // one lane per entry
      const int u = u0 + (tid >> 1), b = (tid & 1) ? nb - 1 - u : u;
      MixDraw d = mix_draw((uint64_t)pos0 + (uint64_t)b, seed, thr_p, T, S);
      if (u == nb - 1 - u) d = MixDraw{MIX_UNMIXED, 1.f, 0, 0, 0, 0};
      prm[tid] = u32x4{(uint32_t)d.kind, __float_as_uint(d.lam),
                       (uint32_t)d.x0 | ((uint32_t)d.x1 << 8) | ((uint32_t)d.y0 << 16) | ((uint32_t)d.y1 << 24), 0u};
    }
    __syncthreads();
    for (int t = tid; t < ng * CH; t += MIX_NT) {
      const int g = t / CH, c = t - g * CH;
      const int b = u0 + g, pb = nb - 1 - b;
      const u32x4 pa = prm[2 * g], pp = prm[2 * g + 1];
      if (c == 0) {   // the pair's first thread: the second labels and the weights of both entries
        const int32_t la = labels[b], lp = labels[pb];
        labels2[b] = pa[0] ? lp : la;
        lam[b] = __uint_as_float(pa[1]);
        labels2[pb] = pp[0] ? la : lp;
        lam[pb] = __uint_as_float(pp[1]);
      }
      if (pa[0] | pp[0]) {
        u32x4* qa = (u32x4*)(img + ((int64_t)b * CH + c) * 8);
        u32x4* qb = (u32x4*)(img + ((int64_t)pb * CH + c) * 8);
        const u32x4 va = *qa, vb = *qb;
        if (pa[0]) *qa = mix_chunk<C>(va, vb, pa, c);
        if (pp[0]) *qb = mix_chunk<C>(vb, va, pp, c);
      }
    }
    __syncthreads();   // the next group's draws overwrite what this one read
  }
}

// what mix_images_k draws for positions pos0 .. pos0 + n - 1 (the partner plays no part): int32 [n, 6]
// = (kind, the bits of lam, x0, x1, y0, y1)
__global__ __launch_bounds__(MIX_NT) void mix_params_k(int32_t* __restrict__ out, int n, int64_t pos0, uint64_t seed,
                                                       uint32_t thr_p, const float* __restrict__ T,
                                                       const int32_t* __restrict__ S) {
  const int i = blockIdx.x * MIX_NT + threadIdx.x;
  if (i >= n) return;
  const MixDraw d = mix_draw((uint64_t)pos0 + (uint64_t)i, seed, thr_p, T, S);
  int32_t* o = out + 6 * (int64_t)i;
  o[0] = d.kind;
  o[1] = (int32_t)__float_as_uint(d.lam);
  o[2] = d.x0;
  o[3] = d.x1;
  o[4] = d.y0;
  o[5] = d.y1;
}

bool mix_keys_ok(int64_t pos0, int64_t seed, int64_t thr_p, const float* T, const int32_t* S) {
  return pos0 >= 0 && seed >= 0 && thr_p >= 0 && thr_p <= 65536 && (T || S);
}

}  // namespace

hipError_t mix_images(bf16_t* images, const int32_t* labels, int32_t* labels2, float* lam, int nb, int C, int64_t pos0,
                      int64_t seed, int64_t thr_p, const float* T, const int32_t* S, hipStream_t st) {
  if (!mix_keys_ok(pos0, seed, thr_p, T, S) || nb < 0 || !images || !labels || !labels2 || !lam ||
      (uintptr_t)images % 16 || (C != 1 && C != 3))
    return hipErrorInvalidValue;
  if (nb == 0) return hipSuccess;
  const int ngroups = ((nb + 1) / 2 + MIX_G - 1) / MIX_G;
  const dim3 grid(cap_grid(ngroups < 4096 ? ngroups : 4096));   // a grid-stride walk past that
  if (C == 1)
    hipLaunchKernelGGL(mix_images_k<1>, grid, dim3(MIX_NT), 0, st, images, labels, labels2, lam, nb, pos0,
                       (uint64_t)seed, (uint32_t)thr_p, T, S);
  else
    hipLaunchKernelGGL(mix_images_k<3>, grid, dim3(MIX_NT), 0, st, images, labels, labels2, lam, nb, pos0,
                       (uint64_t)seed, (uint32_t)thr_p, T, S);
  return hipGetLastError();
}

hipError_t mix_params(int32_t* out, int n, int64_t pos0, int64_t seed, int64_t thr_p, const float* T, const int32_t* S,
                      hipStream_t st) {
  if (!mix_keys_ok(pos0, seed, thr_p, T, S) || n < 0 || !out) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(mix_params_k, dim3((n + MIX_NT - 1) / MIX_NT), dim3(MIX_NT), 0, st, out, n, pos0, (uint64_t)seed,
                     (uint32_t)thr_p, T, S);
  return hipGetLastError();
}

}  // namespace mnistx
