// Training augmentation of the K10 input slot: random shift, rotation and zoom of each 28x28 image
// of the batch, gathered from the resident uint8 dataset, normalised (x/255 - 0.5) and written to
// the executor's input buffer in one launch -- the slot prep_images_k fills without augmentation.
//
// The transformation of batch entry b is a pure function of (seed, p), p = pos0 + b the entry's
// global stream position (the position the Feistel shuffle maps to a dataset row), so there is no
// RNG state and nothing to checkpoint.  One Philox4x32-10 call per image (dropout_rng.h):
//   counter = (p & 0xffffffff, p >> 32, 0, 0x41554700),  key = (seed & 0xffffffff, seed >> 32)
//   tx = float(umulhi(w0, 2S+1)) - S,  ty likewise from w1            integers in [-S, S]
//   u(w) = float(w >> 8) * 2^-24                                      [0, 1), exact
//   theta = (R * (2 u(w2) - 1)) * float32(pi / 180),  s = 1 + Z * (2 u(w3) - 1)
// every operation one rounded fp32 operation (no contraction: aug_draw).  Inverse map of output
// pixel (row i, column j), shared by the channels of a pixel:
//   u = j - 13.5, v = i - 13.5, r = 1 / s
//   sx = (c u + sn v) r + 13.5 - tx,  sy = (c v - sn u) r + 13.5 - ty
//   val = bilinear interpolation of the raw image at (sx, sy), taps outside the image worth 0
//   out = fmaf(val, 1/255, -0.5)
// data/augment.py is the host reference of exactly this (params bit for bit, warp in float64).
//
// A block stages AUG_G images at a time in LDS, each behind a zero border wide enough that no tap
// needs a bounds test: pixel (x, y) of an image lives at pixel slot (y + 1) * 32 + x + 4 (times
// Csrc bytes), x, y in [-1, 29].  Slots 0..3 of a row are its left border and, read as x = 28, 29
// of the row above, that row's right border.  sx, sy are clamped to [-1, 28], which changes no
// value (outside it every tap with a non-zero weight is a border tap).  The source rows are 7 Csrc
// dwords and land dword-aligned, so staging is one 16-byte global load and four ds_write_b32 per
// lane; the borders are zeroed once per block, staging overwrites the interior alone.
// The per-image parameters (Philox, sincosf, 1 / s) are computed by ONE lane per image and handed
// to the image's lanes through LDS: gfx950 has no scalar floating point, and recomputing them in
// every wave costs what the LR schedule's per-wave cosf did.  Stores are 16 bytes per lane.
// The grid is one resident round of blocks, each walking its groups in a software pipeline (the
// loads and the draw of the next group run under the interpolation of the current one): with the
// index -> row -> LDS -> interpolate chain serial per group the kernel was bound by load latency.
#include "common.h"
#include "dropout_rng.h"
#include "launchers.h"

namespace mnistx {
namespace {

constexpr int AUG_NT = 256;
constexpr int AUG_G = 8;                     // images staged per block iteration
constexpr uint32_t AUG_TAG = 0x41554700u;    // counter word 3: no dropout layer word (L << 16 | g, L < 65536,
                                             // g <= 65535) reaches it with a real layer index
constexpr float AUG_DEG = 0.017453292519943295f;   // float32(pi / 180)

struct AugDraw {
  float tx, ty, theta, s;
};

// The draw of stream position p.  Both kernels call this; contraction is off so that every line is
// the single rounded fp32 operation the host reference performs.
DEV AugDraw aug_draw(uint64_t p, uint64_t seed, int S, float R, float Z) {
#pragma clang fp contract(off)
  const u32x4 w = philox4x32_10(u32x4{(uint32_t)p, (uint32_t)(p >> 32), 0u, AUG_TAG}, (uint32_t)seed,
                                (uint32_t)(seed >> 32));
  const uint32_t span = 2u * (uint32_t)S + 1u;
  AugDraw d;
  d.tx = (float)__umulhi(w[0], span) - (float)S;
  d.ty = (float)__umulhi(w[1], span) - (float)S;
  const float u2 = (float)(w[2] >> 8) * 5.9604644775390625e-8f;   // 2^-24
  const float u3 = (float)(w[3] >> 8) * 5.9604644775390625e-8f;
  const float t2 = 2.f * u2 - 1.f;   // exact
  const float t3 = 2.f * u3 - 1.f;
  const float deg = R * t2;
  d.theta = deg * AUG_DEG;
  const float zz = Z * t3;
  d.s = 1.f + zz;
  return d;
}

template <typename OutT>
DEV void store_vec(OutT* dst, const float* o);
template <>
DEV void store_vec<bf16_t>(bf16_t* dst, const float* o) {
  *(u32x4*)dst = u32x4{pack2(o[0], o[1]), pack2(o[2], o[3]), pack2(o[4], o[5]), pack2(o[6], o[7])};
}
template <>
DEV void store_vec<float>(float* dst, const float* o) {
  *(f32x4*)dst = f32x4{o[0], o[1], o[2], o[3]};
}

// CS / CD: source / destination channels (1 -> 3 replicates channel 0, as prep_images_k does).
template <typename OutT, int CS, int CD>
__global__ __launch_bounds__(AUG_NT) void augment_images_k(const uint8_t* __restrict__ src,
                                                            const int64_t* __restrict__ idx,
                                                            const int32_t* __restrict__ lab_src, int nb, int64_t pos0,
                                                            uint64_t seed, int S, float R, float Z,
                                                            OutT* __restrict__ out, int32_t* __restrict__ lab_out) {
  constexpr int IMG = 1024 * CS;             // LDS bytes of one bordered image (32 rows of 32 pixel slots)
  constexpr int ROWDW = 7 * CS;              // dwords of a source row
  constexpr int NIN = 49 * CS;               // 16-byte vectors of a source image
  constexpr int EPV = 16 / (int)sizeof(OutT);   // output elements per 16-byte store
  constexpr int NOUT = 784 * CD / EPV;       // 16-byte vectors of an output image
  constexpr int NSLOT = (AUG_G * NIN + AUG_NT - 1) / AUG_NT;   // source vectors a thread stages per group
  constexpr int PLANE0 = AUG_NT - 64;        // the parameter lanes: the first AUG_G lanes of the last wave,
                                             // which has the fewest output vectors to compute
  // one LDS object: the images, then 4 floats per image (c / s, sn / s, 13.5 - tx, 13.5 - ty)
  __shared__ __attribute__((aligned(16))) uint8_t lds[AUG_G * IMG + AUG_G * 16];
  f32x4* prm = (f32x4*)(lds + AUG_G * IMG);
  const int tid = threadIdx.x;
  for (int i = tid; i < AUG_G * IMG / 16; i += AUG_NT) ((u32x4*)lds)[i] = u32x4{0u, 0u, 0u, 0u};
  const int ngroups = (nb + AUG_G - 1) / AUG_G;
  const bool plane = tid >= PLANE0 && tid < PLANE0 + AUG_G;
  // Software pipeline over the block's groups: while group n is computed out of LDS, the source
  // vectors of group n + 1 are in flight to registers (px), the dataset rows of group n + 2 are in
  // flight (rows), and the parameter lanes draw group n + 1.  Entries past the batch are clamped to
  // its last entry, so no load sits under a branch; what they fetch is never written anywhere.
  int64_t rows[NSLOT], prow = 0;
  u32x4 px[NSLOT];
  f32x4 q = f32x4{0.f, 0.f, 0.f, 0.f};
  int32_t lab = 0;
  auto entry = [&](int grp, int g) {
    const int b = grp * AUG_G + g;
    return b < nb ? b : nb - 1;
  };
  auto load_rows = [&](int grp) {
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) rows[s] = idx[entry(grp, (tid + AUG_NT * s) / NIN)];
    if (plane) prow = idx[entry(grp, tid - PLANE0)];
  };
  auto load_src = [&]() {
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int v = tid + AUG_NT * s, w = v - (v / NIN) * NIN;
      px[s] = *(const u32x4*)(src + rows[s] * (int64_t)(784 * CS) + 16 * w);
    }
  };
  auto draw = [&](int grp) {   // one lane per image: the draw, the trigonometry, the label
    if (plane) {
      const AugDraw d = aug_draw((uint64_t)pos0 + (uint64_t)entry(grp, tid - PLANE0), seed, S, R, Z);
      float sn, c;
      sincosf(d.theta, &sn, &c);
      const float r = 1.f / d.s;
      q = f32x4{c * r, sn * r, 13.5f - d.tx, 13.5f - d.ty};
      lab = lab_src[prow];
    }
  };
  const int stride = gridDim.x;
  load_rows(blockIdx.x);
  load_src();
  draw(blockIdx.x);
  load_rows(blockIdx.x + stride);
  __syncthreads();   // the zeroed borders
  for (int grp = blockIdx.x; grp < ngroups; grp += stride) {
    const int b0 = grp * AUG_G;
    const int ng = nb - b0 < AUG_G ? nb - b0 : AUG_G;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int v = tid + AUG_NT * s, g = v / NIN, w = v - g * NIN;
      if (v < ng * NIN) {
        uint8_t* img = lds + g * IMG;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int d = 4 * w + k, r = d / ROWDW, kk = d - r * ROWDW;
          *(uint32_t*)(img + (r + 1) * (32 * CS) + 4 * CS + 4 * kk) = px[s][k];
        }
      }
    }
    if (plane && tid - PLANE0 < ng) {
      prm[tid - PLANE0] = q;
      lab_out[b0 + tid - PLANE0] = lab;
    }
    __syncthreads();
    load_src();                      // group grp + stride, rows loaded an iteration ago
    draw(grp + stride);
    load_rows(grp + 2 * stride);
    for (int v = tid; v < ng * NOUT; v += AUG_NT) {
      const int g = v / NOUT, w = v - g * NOUT;
      const f32x4 q = prm[g];
      const uint8_t* img = lds + g * IMG;
      float o[EPV];
#pragma unroll
      for (int j = 0; j < EPV; ++j) {
        const int e = w * EPV + j, pix = e / CD, c = e - pix * CD;
        const int cs = c < CS ? c : 0;
        const int i = pix / 28, jx = pix - 28 * i;
        const float u = (float)jx - 13.5f, vv = (float)i - 13.5f;
        float sx = q[0] * u + q[1] * vv + q[2];
        float sy = q[0] * vv - q[1] * u + q[3];
        sx = fminf(fmaxf(sx, -1.f), 28.f);
        sy = fminf(fmaxf(sy, -1.f), 28.f);
        const float x0 = floorf(sx), y0 = floorf(sy);
        const float fx = sx - x0, fy = sy - y0;
        // The taps of a row are bytes a and a + CS (CS <= 3): both lie in the four bytes from a on,
        // funnel-shifted out of the two aligned dwords around a.  Byte (and the unaligned 16-bit
        // reads the compiler merges them into) reads of scattered addresses ran the LDS at a
        // fraction of its dword rate and bounded the kernel.
        const uint32_t a = (uint32_t)((((int)y0 + 1) * 32 + (int)x0 + 4) * CS + cs);
        const uint32_t* wd = (const uint32_t*)(img + (a & ~3u));
        const uint32_t r0 = __builtin_amdgcn_alignbyte(wd[1], wd[0], a & 3u);
        const uint32_t r1 = __builtin_amdgcn_alignbyte(wd[8 * CS + 1], wd[8 * CS], a & 3u);
        const float v00 = (float)(r0 & 0xffu), v01 = (float)((r0 >> (8 * CS)) & 0xffu);
        const float v10 = (float)(r1 & 0xffu), v11 = (float)((r1 >> (8 * CS)) & 0xffu);
        const float top = v00 + fx * (v01 - v00), bot = v10 + fx * (v11 - v10);
        o[j] = fmaf(top + fy * (bot - top), 1.f / 255.f, -0.5f);
      }
      store_vec<OutT>(out + ((int64_t)(b0 + g) * NOUT + w) * EPV, o);
    }
    __syncthreads();   // the next group's staging overwrites what this one read
  }
}

// (tx, ty, theta, s) of positions pos0 .. pos0 + n - 1 as the image kernel draws them: [n, 4] fp32
__global__ __launch_bounds__(AUG_NT) void augment_params_k(float* __restrict__ out, int n, int64_t pos0, uint64_t seed,
                                                            int S, float R, float Z) {
  const int i = blockIdx.x * AUG_NT + threadIdx.x;
  if (i >= n) return;
  const AugDraw d = aug_draw((uint64_t)(pos0 + i), seed, S, R, Z);
  *(f32x4*)(out + 4 * (int64_t)i) = f32x4{d.tx, d.ty, d.theta, d.s};
}

bool aug_keys_ok(int64_t pos0, int64_t seed, int S, float R, float Z) {
  return pos0 >= 0 && seed >= 0 && S >= 0 && S <= AUG_MAX_SHIFT && R >= 0.f && R <= AUG_MAX_ROTATE && Z >= 0.f &&
         Z <= AUG_MAX_SCALE;   // a NaN fails its comparisons
}

// Blocks that fill every CU exactly once (occupancy API, cached per kernel): the pipelined walk
// wants one resident round and no partial second one.
template <auto KER>
int resident_grid() {
  static int n = 0;
  if (n == 0) {
    int per_cu = 0, dev = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KER, AUG_NT, 0) == hipSuccess &&
        hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && per_cu > 0)
      n = per_cu * cus;
    else
      n = 1024;
  }
  return n;
}

template <auto KER, typename OutT>
hipError_t launch_one(const uint8_t* src, const int64_t* idx, const int32_t* lab_src, int nb, int64_t pos0,
                      uint64_t seed, int S, float R, float Z, OutT* out, int32_t* lab_out, hipStream_t st) {
  const int ngroups = (nb + AUG_G - 1) / AUG_G, res = resident_grid<KER>();
  hipLaunchKernelGGL(KER, dim3(cap_grid(ngroups < res ? ngroups : res)), dim3(AUG_NT), 0, st, src, idx, lab_src, nb,
                     pos0, seed, S, R, Z, out, lab_out);
  return hipGetLastError();
}

template <typename OutT>
hipError_t launch_images(const uint8_t* src, const int64_t* idx, const int32_t* lab_src, int nb, int Csrc, int Cdst,
                         int64_t pos0, uint64_t seed, int S, float R, float Z, OutT* out, int32_t* lab_out,
                         hipStream_t st) {
  if (Csrc == 1 && Cdst == 1)
    return launch_one<augment_images_k<OutT, 1, 1>>(src, idx, lab_src, nb, pos0, seed, S, R, Z, out, lab_out, st);
  if (Csrc == 3 && Cdst == 3)
    return launch_one<augment_images_k<OutT, 3, 3>>(src, idx, lab_src, nb, pos0, seed, S, R, Z, out, lab_out, st);
  if (Csrc == 1 && Cdst == 3)
    return launch_one<augment_images_k<OutT, 1, 3>>(src, idx, lab_src, nb, pos0, seed, S, R, Z, out, lab_out, st);
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t augment_images(const uint8_t* src, const int64_t* idx, const int32_t* lab_src, int nb, int Csrc, int Cdst,
                          int64_t pos0, int64_t seed, int S, float R, float Z, void* out, bool out_f32,
                          int32_t* lab_out, hipStream_t st) {
  if (!aug_keys_ok(pos0, seed, S, R, Z) || nb < 0 || !src || !idx || !lab_src || !out || !lab_out ||
      (uintptr_t)src % 16 || (uintptr_t)out % 16)
    return hipErrorInvalidValue;
  if (nb == 0) return hipSuccess;
  return out_f32 ? launch_images<float>(src, idx, lab_src, nb, Csrc, Cdst, pos0, (uint64_t)seed, S, R, Z, (float*)out,
                                        lab_out, st)
                 : launch_images<bf16_t>(src, idx, lab_src, nb, Csrc, Cdst, pos0, (uint64_t)seed, S, R, Z,
                                         (bf16_t*)out, lab_out, st);
}

hipError_t augment_params(float* out, int n, int64_t pos0, int64_t seed, int S, float R, float Z, hipStream_t st) {
  if (!aug_keys_ok(pos0, seed, S, R, Z) || n < 0 || !out || (uintptr_t)out % 16) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(augment_params_k, dim3((n + AUG_NT - 1) / AUG_NT), dim3(AUG_NT), 0, st, out, n, pos0,
                     (uint64_t)seed, S, R, Z);
  return hipGetLastError();
}

}  // namespace mnistx
