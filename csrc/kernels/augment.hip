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
//
// The elastic form (compiled by augment_elastic.hip alone, so that this file's code object is what
// it was without it) displaces the inverse map by the field D_f = alpha * (G r_f G^T), f = 0 for
// x and 1 for y, indexed by the OUTPUT pixel and shared by its channels:
//   e = f * 784 + 28 i + j,  g = e >> 3:  counter = (p lo, p hi, g, 0x41554701), dropout's unpacking
//   r_f[i, j] = (float(draw) - 32767.5) * 2^-15,  G the 28 x 28 band matrix of the host's half table
//   sx' = sx + D_0[i, j],  sy' = sy + D_1[i, j]
// (zero extension: r = 0 outside the image).  Per group of AUG_GE images the block fills the draw
// planes in LDS as (r_0, r_1) fp32 pairs, the 196 Philox calls of an image spread over its lanes,
// smooths them horizontally into a second plane and vertically back into the first, scaled by alpha;
// the interpolation loop reads the pair of its pixel and adds it, nothing else in it changes.  A
// smoothing task is half a line: its 28 inputs sit in registers and its 14 outputs are the dense
// 14 x 28 product with the table, which travels as a kernel argument (SGPRs) padded with zeros to
// 28 entries -- a zero weight adds an exact zero, so the sum is the truncated one for every K, and
// every index is static.  The second half of a line runs the same code on the mirrored line (G is
// symmetric), so no wave diverges; a pair per lane makes every step one v_pk_fma_f32.  Tables with
// K <= EL_BAND (sigma <= 4, the recipe's) take a second copy of the pass that leaves the taps and
// inputs beyond that band out (273 instead of 392 steps per task): a uniform branch on the table.
#include "common.h"
#include "dropout_rng.h"
#include "launchers.h"

namespace mnistx {
namespace {

constexpr int AUG_NT = 256;
constexpr int AUG_G = 8;                     // images staged per block iteration
constexpr int AUG_GE = 4;                    // ... of the elastic form: two fp32-pair planes per image keep it
                                             // under 64 KB of LDS, two blocks to a CU
constexpr uint32_t AUG_ELASTIC_TAG = 0x41554701u;   // counter word 3 of the field's draws (word 2: the draw group)
constexpr int EL_CALLS = 196;                // Philox calls per image: 2 * 784 draws, eight per call
constexpr int EL_BAND = 12;                  // tables with K <= 12 (sigma <= 4) run a band-limited copy of the smoothing
constexpr int EL_TASKS = 56;                 // smoothing tasks per image and pass: 28 lines, two halves
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

typedef float f32x2 __attribute__((ext_vector_type(2)));

// the half table w_0 .. w_K of the smoothing Gaussian, zeros behind it: by value in the kernel arguments
struct ElTable {
  float w[28];
  int K;      // the table's length - 1, from the host: chooses the band-limited copy of the smoothing
};

// what the elastic form of the image kernel adds to its state: the two LDS planes and its arguments
struct ElState {
  f32x2* fld;   // the draws, then the field D
  f32x2* hpl;   // the horizontally smoothed draws
  float alpha;
  ElTable tb;
};

// The (r_0, r_1) planes of ng images at stream positions p0 .. p0 + ng - 1: r[g * 784 + pixel].
DEV void el_fill(f32x2* r, int ng, uint64_t p0, uint64_t seed, int tid, int nt) {
  for (int t = tid; t < ng * EL_CALLS; t += nt) {
    const int g = t / EL_CALLS, c = t - g * EL_CALLS;
    const uint64_t p = p0 + (uint64_t)g;
    const u32x4 w = philox4x32_10(u32x4{(uint32_t)p, (uint32_t)(p >> 32), (uint32_t)c, AUG_ELASTIC_TAG}, (uint32_t)seed,
                                  (uint32_t)(seed >> 32));
    const int f = c >= EL_CALLS / 2 ? 1 : 0;   // 784 = 8 * 98: a call's eight draws lie in one plane
    float* dst = (float*)(r + g * 784 + 8 * (c - (EL_CALLS / 2) * f)) + f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {              // exact: |draw - 32767.5| < 2^15 has 17 significant bits
      dst[4 * k] = ((float)(w[k] & 0xffffu) - 32767.5f) * 3.0517578125e-05f;
      dst[4 * k + 2] = ((float)(w[k] >> 16) - 32767.5f) * 3.0517578125e-05f;
    }
  }
}

// One separable pass over ng images: out = in * G along the rows (VERT false) or G * in along the
// columns (VERT true, times scale).  in and out are different planes.  KB: the band the caller
// knows the table to fit in (w_k = 0 for k > KB); taps and inputs beyond it are not issued.
template <bool VERT, int KB>
DEV void el_smooth(const f32x2* in, f32x2* outp, int ng, int tid, int nt, const ElTable& tb, float scale) {
  constexpr int ES = VERT ? 28 : 1;
  for (int t = tid; t < ng * EL_TASKS; t += nt) {
    const int g = t / EL_TASKS, rem = t - g * EL_TASKS, line = rem >> 1, half = rem & 1;
    const int base = g * 784 + (VERT ? line : 28 * line);
    const int first = half ? base + 27 * ES : base, step = half ? -ES : ES;   // the second half: the mirrored line
    constexpr int NX = 14 + KB < 28 ? 14 + KB : 28;   // the inputs the 14 outputs reach
    f32x2 x[NX];
#pragma unroll
    for (int m = 0; m < NX; ++m) x[m] = in[first + m * step];
#pragma unroll
    for (int j = 0; j < 14; ++j) {
      f32x2 acc = f32x2{0.f, 0.f};
#pragma unroll
      for (int m = 0; m < NX; ++m) {
        const int k = j > m ? j - m : m - j;
        if (k > KB) continue;
        const float wk = tb.w[k];
        acc = __builtin_elementwise_fma(f32x2{wk, wk}, x[m], acc);
      }
      if constexpr (VERT) acc *= scale;
      outp[first + j * step] = acc;
    }
  }
}
DEV void el_hpass(const f32x2* r, f32x2* h, int ng, int tid, int nt, const ElTable& tb) {
  if (tb.K <= EL_BAND)   // uniform: the table is a kernel argument
    el_smooth<false, EL_BAND>(r, h, ng, tid, nt, tb, 1.f);
  else
    el_smooth<false, 27>(r, h, ng, tid, nt, tb, 1.f);
}
DEV void el_vpass(const f32x2* h, f32x2* d, int ng, int tid, int nt, const ElTable& tb, float alpha) {
  if (tb.K <= EL_BAND)
    el_smooth<true, EL_BAND>(h, d, ng, tid, nt, tb, alpha);
  else
    el_smooth<true, 27>(h, d, ng, tid, nt, tb, alpha);
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
// The elastic form is this kernel text compiled with MNISTX_AUG_ELASTIC_TU set (augment_elastic.hip):
// the switch is the translation unit's, so that without it the kernels are, instruction for
// instruction, what they were before the elastic form existed (as the EL = false instantiations of
// a body shared through a template parameter they came out with other index arithmetic).  The
// elastic kernel has two more parameters, hence the two macros; inside the body the switch is the
// constant AUG_EL over an ElState.
#ifdef MNISTX_AUG_ELASTIC_TU
#define AUG_IMAGES_K augment_elastic_images_k
#define AUG_ELASTIC_PARAMS , float alpha, ElTable tb
constexpr bool AUG_EL = true;
#else
#define AUG_IMAGES_K augment_images_k
#define AUG_ELASTIC_PARAMS
constexpr bool AUG_EL = false;
#endif
template <typename OutT, int CS, int CD>
__global__ __launch_bounds__(AUG_NT) void AUG_IMAGES_K(const uint8_t* __restrict__ src,
                                                        const int64_t* __restrict__ idx,
                                                        const int32_t* __restrict__ lab_src, int nb, int64_t pos0,
                                                        uint64_t seed, int S, float R, float Z,
                                                        OutT* __restrict__ out,
                                                        int32_t* __restrict__ lab_out AUG_ELASTIC_PARAMS) {
  constexpr int AUG_G = AUG_EL ? AUG_GE : mnistx::AUG_G;
  constexpr int IMG = 1024 * CS;             // LDS bytes of one bordered image (32 rows of 32 pixel slots)
  constexpr int ROWDW = 7 * CS;              // dwords of a source row
  constexpr int NIN = 49 * CS;               // 16-byte vectors of a source image
  constexpr int EPV = 16 / (int)sizeof(OutT);   // output elements per 16-byte store
  constexpr int NOUT = 784 * CD / EPV;       // 16-byte vectors of an output image
  constexpr int NSLOT = (AUG_G * NIN + AUG_NT - 1) / AUG_NT;   // source vectors a thread stages per group
  constexpr int PLANE0 = AUG_NT - 64;        // the parameter lanes: the first AUG_G lanes of the last wave,
                                             // which has the fewest output vectors to compute
  // one LDS object: the images, then 4 floats per image (c / s, sn / s, 13.5 - tx, 13.5 - ty)
  // ... and in the elastic form two planes of (x, y) fp32 pairs per image
  __shared__ __attribute__((aligned(16))) uint8_t lds[AUG_G * IMG + AUG_G * 16 + (AUG_EL ? AUG_G * 2 * 784 * 8 : 0)];
  f32x4* prm = (f32x4*)(lds + AUG_G * IMG);
#ifdef MNISTX_AUG_ELASTIC_TU
  const ElState el{(f32x2*)(lds + AUG_G * IMG + AUG_G * 16), (f32x2*)(lds + AUG_G * IMG + AUG_G * 16) + AUG_G * 784, alpha,
                   tb};
#else
  const ElState el{};   // read under if constexpr (AUG_EL) alone
#endif
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
    if constexpr (AUG_EL) el_fill(el.fld, ng, (uint64_t)pos0 + (uint64_t)b0, seed, tid, AUG_NT);
    __syncthreads();
    load_src();                      // group grp + stride, rows loaded an iteration ago
    draw(grp + stride);
    load_rows(grp + 2 * stride);
    if constexpr (AUG_EL) {
      el_hpass(el.fld, el.hpl, ng, tid, AUG_NT, el.tb);
      __syncthreads();
      el_vpass(el.hpl, el.fld, ng, tid, AUG_NT, el.tb, el.alpha);
      __syncthreads();
    }
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
        if constexpr (AUG_EL) {
          const f32x2 d = el.fld[g * 784 + pix];
          sx += d[0];
          sy += d[1];
        }
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

#ifdef MNISTX_AUG_ELASTIC_TU
// The draws of positions pos0 .. pos0 + n - 1 as the image kernel fills them, back as integers
// (exact: r * 2^15 + 32767.5): int32 [n, 2, 784].  FIELD: the field D it adds instead, fp32.
template <bool FIELD>
__global__ __launch_bounds__(AUG_NT) void augment_elastic_probe_k(void* __restrict__ out, int n, int64_t pos0,
                                                                   uint64_t seed, float alpha, ElTable tb) {
  __shared__ __attribute__((aligned(16))) f32x2 pl[(FIELD ? 2 : 1) * AUG_GE * 784];
  const int tid = threadIdx.x;
  const int ngroups = (n + AUG_GE - 1) / AUG_GE;
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int b0 = grp * AUG_GE;
    const int ng = n - b0 < AUG_GE ? n - b0 : AUG_GE;
    el_fill(pl, ng, (uint64_t)pos0 + (uint64_t)b0, seed, tid, AUG_NT);
    __syncthreads();
    if constexpr (FIELD) {
      el_hpass(pl, pl + AUG_GE * 784, ng, tid, AUG_NT, tb);
      __syncthreads();
      el_vpass(pl + AUG_GE * 784, pl, ng, tid, AUG_NT, tb, alpha);
      __syncthreads();
    }
    for (int v = tid; v < ng * 1568; v += AUG_NT) {
      const int g = v / 1568, e = v - g * 1568, f = e >= 784 ? 1 : 0;
      const float x = ((const float*)pl)[2 * (g * 784 + e - 784 * f) + f];
      const int64_t o = (int64_t)(b0 + g) * 1568 + e;
      if constexpr (FIELD)
        ((float*)out)[o] = x;
      else
        ((int32_t*)out)[o] = (int32_t)(x * 32768.f + 32767.5f);
    }
    __syncthreads();   // the next group's fill overwrites what this one read
  }
}

#else
// (tx, ty, theta, s) of positions pos0 .. pos0 + n - 1 as the image kernel draws them: [n, 4] fp32
__global__ __launch_bounds__(AUG_NT) void augment_params_k(float* __restrict__ out, int n, int64_t pos0, uint64_t seed,
                                                            int S, float R, float Z) {
  const int i = blockIdx.x * AUG_NT + threadIdx.x;
  if (i >= n) return;
  const AugDraw d = aug_draw((uint64_t)(pos0 + i), seed, S, R, Z);
  *(f32x4*)(out + 4 * (int64_t)i) = f32x4{d.tx, d.ty, d.theta, d.s};
}
#endif

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

#ifndef MNISTX_AUG_ELASTIC_TU
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

#else
// augment_elastic.hip: the elastic instantiations alone, as a translation unit -- and so a code
// object -- of their own, as mlp_head_smooth.hip is of mlp_head.hip.
template <auto KER, typename OutT>
hipError_t launch_one(const uint8_t* src, const int64_t* idx, const int32_t* lab_src, int nb, int64_t pos0,
                      uint64_t seed, int S, float R, float Z, OutT* out, int32_t* lab_out, float alpha,
                      const ElTable& tb, hipStream_t st) {
  const int ngroups = (nb + AUG_GE - 1) / AUG_GE, res = resident_grid<KER>();
  hipLaunchKernelGGL(KER, dim3(cap_grid(ngroups < res ? ngroups : res)), dim3(AUG_NT), 0, st, src, idx, lab_src, nb,
                     pos0, seed, S, R, Z, out, lab_out, alpha, tb);
  return hipGetLastError();
}

template <typename OutT>
hipError_t launch_images(const uint8_t* src, const int64_t* idx, const int32_t* lab_src, int nb, int Csrc, int Cdst,
                         int64_t pos0, uint64_t seed, int S, float R, float Z, OutT* out, int32_t* lab_out, float alpha,
                         const ElTable& tb, hipStream_t st) {
  if (Csrc == 1 && Cdst == 1)
    return launch_one<augment_elastic_images_k<OutT, 1, 1>>(src, idx, lab_src, nb, pos0, seed, S, R, Z, out, lab_out,
                                                            alpha, tb, st);
  if (Csrc == 3 && Cdst == 3)
    return launch_one<augment_elastic_images_k<OutT, 3, 3>>(src, idx, lab_src, nb, pos0, seed, S, R, Z, out, lab_out,
                                                            alpha, tb, st);
  if (Csrc == 1 && Cdst == 3)
    return launch_one<augment_elastic_images_k<OutT, 1, 3>>(src, idx, lab_src, nb, pos0, seed, S, R, Z, out, lab_out,
                                                            alpha, tb, st);
  return hipErrorInvalidValue;
}

// the host's half table behind zeros; false: not a table the kernels take
bool el_table(const float* w, int nw, float alpha, ElTable& tb) {
  if (!w || nw < AUG_MIN_ELASTIC_TAPS || nw > AUG_MAX_ELASTIC_TAPS || !(alpha >= 0.f && alpha <= AUG_MAX_ELASTIC_ALPHA))
    return false;
  for (int k = 0; k < 28; ++k) tb.w[k] = k < nw ? w[k] : 0.f;
  tb.K = nw - 1;
  for (int k = 0; k < nw; ++k)
    if (!(w[k] >= 0.f && w[k] <= 1.f)) return false;   // a NaN fails its comparisons
  return true;
}

template <bool FIELD>
hipError_t launch_probe(void* out, int n, int64_t pos0, int64_t seed, float alpha, const ElTable& tb, hipStream_t st) {
  if (pos0 < 0 || seed < 0 || n < 0 || n >= (1 << 20) || !out) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const int ngroups = (n + AUG_GE - 1) / AUG_GE;
  hipLaunchKernelGGL(augment_elastic_probe_k<FIELD>, dim3(cap_grid(ngroups < 1024 ? ngroups : 1024)), dim3(AUG_NT), 0,
                     st, out, n, pos0, (uint64_t)seed, alpha, tb);
  return hipGetLastError();
}
#endif

}  // namespace

#ifndef MNISTX_AUG_ELASTIC_TU
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

#else
hipError_t augment_images_elastic(const uint8_t* src, const int64_t* idx, const int32_t* lab_src, int nb, int Csrc,
                                  int Cdst, int64_t pos0, int64_t seed, int S, float R, float Z, float alpha,
                                  const float* w, int nw, void* out, bool out_f32, int32_t* lab_out, hipStream_t st) {
  ElTable tb;
  if (!aug_keys_ok(pos0, seed, S, R, Z) || !el_table(w, nw, alpha, tb) || nb < 0 || !src || !idx || !lab_src || !out ||
      !lab_out || (uintptr_t)src % 16 || (uintptr_t)out % 16)
    return hipErrorInvalidValue;
  if (nb == 0) return hipSuccess;
  return out_f32 ? launch_images<float>(src, idx, lab_src, nb, Csrc, Cdst, pos0, (uint64_t)seed, S, R, Z, (float*)out,
                                        lab_out, alpha, tb, st)
                 : launch_images<bf16_t>(src, idx, lab_src, nb, Csrc, Cdst, pos0, (uint64_t)seed, S, R, Z,
                                         (bf16_t*)out, lab_out, alpha, tb, st);
}

hipError_t augment_elastic_draws(int32_t* out, int n, int64_t pos0, int64_t seed, hipStream_t st) {
  return launch_probe<false>(out, n, pos0, seed, 0.f, ElTable{}, st);   // the draws read no table
}

hipError_t augment_elastic_field(float* out, int n, int64_t pos0, int64_t seed, float alpha, const float* w, int nw,
                                 hipStream_t st) {
  ElTable tb;
  if (!el_table(w, nw, alpha, tb)) return hipErrorInvalidValue;
  return launch_probe<true>(out, n, pos0, seed, alpha, tb, st);
}
#endif

}  // namespace mnistx
