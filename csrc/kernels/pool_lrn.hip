// Max-pool fwd/bwd (K6), LRN fwd/bwd (K7), the fused LRN -> pool pair and its packed
// 14 x 14 x 64 form.  Bandwidth-bound: 16-byte vectorised over 8 bf16 channels (NHWC with
// channels padded to 8).
#include "common.h"
#include "launchers.h"
#include "lrn_math.h"
#include "tpb.h"

#include <cstdlib>

namespace mnistx {
namespace {

// ------------------------------------------------------------------ K6 max-pool 2x2/2 SAME
__global__ void maxpool_fwd_k(const bf16_t* __restrict__ x, int Nb, int H, int W, int C, int OH, int OW,
                              bf16_t* __restrict__ y, uint8_t* __restrict__ arg) {
  const int CV = C / 8;
  const int64_t total = (int64_t)Nb * OH * OW * CV;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int cv = (int)(t % CV);
    int64_t r = t / CV;
    const int ow = (int)(r % OW);
    r /= OW;
    const int oh = (int)(r % OH);
    const int n = (int)(r / OH);
    float best[8];
    uint32_t bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; bi[j] = 0; }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int ih = 2 * oh + (d >> 1), iw = 2 * ow + (d & 1);
      if (ih < H && iw < W) {
        const u32x4 v = *(const u32x4*)(x + (((int64_t)n * H + ih) * W + iw) * C + cv * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = u4_get(v, j);
          if (f > best[j]) { best[j] = f; bi[j] = d; }
        }
      }
    }
    u32x4 o;
    uint32_t a0 = 0, a1 = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      u4_set(o, j, f2bf(best[j]));
      if (j < 4) a0 |= bi[j] << (8 * j);
      else a1 |= bi[j] << (8 * (j - 4));
    }
    const int64_t off = (((int64_t)n * OH + oh) * OW + ow) * C + cv * 8;
    *(u32x4*)(y + off) = o;
    *(u32x2*)(arg + off) = u32x2{a0, a1};
  }
}

__global__ void maxpool_bwd_k(const bf16_t* __restrict__ dy, const uint8_t* __restrict__ arg,
                              const bf16_t* __restrict__ y, int relu_mask, int Nb, int H, int W, int C, int OH,
                              int OW, bf16_t* __restrict__ dx) {
  const int CV = C / 8;
  const int64_t total = (int64_t)Nb * OH * OW * CV;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int cv = (int)(t % CV);
    int64_t r = t / CV;
    const int ow = (int)(r % OW);
    r /= OW;
    const int oh = (int)(r % OH);
    const int n = (int)(r / OH);
    const int64_t off = (((int64_t)n * OH + oh) * OW + ow) * C + cv * 8;
    u32x4 g = *(const u32x4*)(dy + off);
    const u32x2 a = *(const u32x2*)(arg + off);
    if (relu_mask) {
      const u32x4 yv = *(const u32x4*)(y + off);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (!(u4_get(yv, j) > 0.f)) u4_set(g, j, 0);
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int ih = 2 * oh + (d >> 1), iw = 2 * ow + (d & 1);
      if (ih < H && iw < W) {
        u32x4 o = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t aj = ((j < 4 ? a[0] : a[1]) >> (8 * (j & 3))) & 0xff;
          if (aj == (uint32_t)d) u4_set(o, j, (bf16_t)((g[j >> 1] >> (16 * (j & 1))) & 0xffff));
        }
        *(u32x4*)(dx + (((int64_t)n * H + ih) * W + iw) * C + cv * 8) = o;
      }
    }
  }
}

// ------------------------------------------------------------------ K7 LRN (TF semantics)
// y[c] = x[c] * (bias + alpha * sum_{|c'-c|<=R} x[c']^2)^-beta
// Channel-parallel: each lane owns 8 channels (one 16-byte vector) of a pixel, the
// C/8 lanes of a pixel sit side by side inside one 16-lane DPP row, and the R
// channels a window needs from the neighbouring vectors come over DPP row shifts
// (zeroed at the pixel's first / last vector).  Loads and stores are fully
// coalesced 16-byte vectors and a lane needs ~40 VGPRs (the one-pixel-per-lane form
// held all C channels three times over: 2 waves/SIMD, 2-3x the HBM floor).
template <int C, int R>
__global__ __launch_bounds__(TPB) void lrn_fwd_k(const bf16_t* __restrict__ x, int64_t P, float bias, float alpha,
                                                 float beta, bf16_t* __restrict__ y) {
  constexpr int G = C / 8;
  const int64_t total = P * G;   // one 8-channel vector per lane; whole pixels per wave
  const int c8 = threadIdx.x % G;
  // uniform trip count: every lane takes part in the DPP exchanges
  for (int64_t base = (int64_t)blockIdx.x * TPB; base < total; base += (int64_t)gridDim.x * TPB) {
    const int64_t t = base + threadIdx.x;
    const bool ok = t < total;
    const u32x4 xv = *(const u32x4*)(x + (ok ? t : 0) * 8);   // unconditional (clamped) load
    const u32x4 o = lrn_fwd8<G, R>(xv, c8, bias, alpha, beta);
    if (ok) *(u32x4*)(y + t * 8) = o;
  }
}

// dx[c] = dy[c] s[c]^-b - 2ab x[c] sum_{|c'-c|<=R} dy[c'] x[c'] s[c']^(-b-1)
template <int C, int R, bool B075 = false>
__global__ __launch_bounds__(TPB) void lrn_bwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                 int64_t P, float bias, float alpha, float beta, int relu_mask,
                                                 bf16_t* __restrict__ dx) {
  constexpr int G = C / 8;
  const int64_t total = P * G;
  const int c8 = threadIdx.x % G;
  for (int64_t base = (int64_t)blockIdx.x * TPB; base < total; base += (int64_t)gridDim.x * TPB) {
    const int64_t t = base + threadIdx.x;
    const bool ok = t < total;
    const u32x4 xv = *(const u32x4*)(x + (ok ? t : 0) * 8);    // unconditional (clamped) loads
    const u32x4 gv = *(const u32x4*)(dy + (ok ? t : 0) * 8);
    const u32x4 o = lrn_bwd8<G, R, B075>(xv, gv, c8, bias, alpha, beta, relu_mask);
    if (ok) *(u32x4*)(dx + t * 8) = o;
  }
}

// ------------------------------------------------------------------ K7+K6 fused: LRN -> 2x2/2 max-pool
// The reference CNN's norm2 -> pool2 (mnist_input.py:168-172) as one pass: lane
// group = one pool window, lane = 8 channels of it; the LRN of the window's 4 pixels
// is computed in registers and only the pooled maximum (+ argmax byte) is written,
// so the full-resolution LRN output never goes to HBM (and is never re-read by the
// pool).  Pooling compares the bf16-rounded LRN values in window order, exactly
// like lrn_fwd + maxpool_fwd.  Backward: unpool dP through the argmax into the 4
// pixels' dY in registers and apply the LRN gradient directly (no dY image).
// LRNP_U pool windows per lane per iteration, the loads of both issued first: 142 -> 132 us
// at B = 16384 (the same unrolling of lrn_fwd_k, 4 vectors per lane, measured no change)
constexpr int LRNP_U = 2;
template <int C, int R>
__global__ __launch_bounds__(TPB) void lrn_pool_fwd_k(const bf16_t* __restrict__ x, int Nb, int H, int W, float bias,
                                                      float alpha, float beta, bf16_t* __restrict__ y,
                                                      uint8_t* __restrict__ arg) {
  constexpr int G = C / 8;
  const int OH = H / 2, OW = W / 2;
  const int64_t total = (int64_t)Nb * OH * OW * G;
  const int c8 = threadIdx.x % G;
  const int64_t step = (int64_t)gridDim.x * TPB;
  for (int64_t base = (int64_t)blockIdx.x * TPB; base < total; base += LRNP_U * step) {
    // the windows' 4 pixel vectors: unconditional loads (clamped index), all in flight
    // before any math -- a load under `ok ?` made each wait for its own latency
    u32x4 xq[LRNP_U][4];
#pragma unroll
    for (int k = 0; k < LRNP_U; ++k) {
      const int64_t t = base + k * step + threadIdx.x;
      const int64_t win = t < total ? t / G : 0;
      const int ow = (int)(win % OW);
      const int64_t r = win / OW;
      const int oh = (int)(r % OH);
      const int64_t n = r / OH;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int ih = 2 * oh + (d >> 1), iw = 2 * ow + (d & 1);
        xq[k][d] = *(const u32x4*)(x + ((n * H + ih) * W + iw) * C + c8 * 8);
      }
    }
#pragma unroll
    for (int k = 0; k < LRNP_U; ++k) {
      const int64_t t = base + k * step + threadIdx.x;
      float best[8];
      uint32_t bi[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; bi[j] = 0; }
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        float v[8], sq[8], s[8];
        unpack8(xq[k][d], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) sq[j] = v[j] * v[j];
        lane_window_sums<G, R>(sq, c8, s);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = bf2f(f2bf(lrn_out(v[j], s[j], bias, alpha, beta)));
          if (f > best[j]) { best[j] = f; bi[j] = d; }
        }
      }
      if (t < total) {
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack2(best[2 * j], best[2 * j + 1]);
        const int64_t off = (t / G) * C + c8 * 8;
        *(u32x4*)(y + off) = o;
        *(u32x2*)(arg + off) = u32x2{bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24),
                                     bi[4] | (bi[5] << 8) | (bi[6] << 16) | (bi[7] << 24)};
      }
    }
  }
}

template <int C, int R, bool B075 = false>
__global__ __launch_bounds__(TPB) void lrn_pool_bwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dP,
                                                      const uint8_t* __restrict__ arg, int Nb, int H, int W,
                                                      float bias, float alpha, float beta, int relu_mask,
                                                      bf16_t* __restrict__ dx) {
  constexpr int G = C / 8;
  const int OH = H / 2, OW = W / 2;
  const int64_t total = (int64_t)Nb * OH * OW * G;
  const int c8 = threadIdx.x % G;
  for (int64_t base = (int64_t)blockIdx.x * TPB; base < total; base += (int64_t)gridDim.x * TPB) {
    const int64_t t = base + threadIdx.x;
    const bool ok = t < total;
    const int64_t win = ok ? t / G : 0;
    const int ow = (int)(win % OW);
    const int64_t r = win / OW;
    const int oh = (int)(r % OH);
    const int64_t n = r / OH;
    const int64_t poff = win * C + c8 * 8;
    // unconditional loads (clamped index: win = 0 past the end), all issued up front
    const u32x4 pv = *(const u32x4*)(dP + poff);
    const u32x2 av = *(const u32x2*)(arg + poff);
    u32x4 xq[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int ih = 2 * oh + (d >> 1), iw = 2 * ow + (d & 1);
      xq[d] = *(const u32x4*)(x + ((n * H + ih) * W + iw) * C + c8 * 8);
    }
    float pg[8];
    unpack8(pv, pg);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int ih = 2 * oh + (d >> 1), iw = 2 * ow + (d & 1);
      const int64_t xoff = ((n * H + ih) * W + iw) * C + c8 * 8;
      float v[8], g[8];
      unpack8(xq[d], v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t aj = ((j < 4 ? av[0] : av[1]) >> (8 * (j & 3))) & 0xffu;
        g[j] = aj == (uint32_t)d ? pg[j] : 0.f;          // max-unpool
      }
      const u32x4 o = lrn_bwd8_vals<G, R, B075>(v, g, c8, bias, alpha, beta, relu_mask);
      if (ok) *(u32x4*)(dx + xoff) = o;
    }
  }
}

// The reference CNN's norm2 -> pool2 (64 channels, 14 x 14, radius 4, post-ReLU input) on
// packed fp32.  lrn_pool_fwd_k / lrn_pool_bwd_k spend most of their issue slots on VALU work
// (profiles/r6/lrnpk/): 32-bit index math with the geometry as constants (no 64-bit divides),
// the element-wise LRN math of two vectors per lane as v_pk ops, and -- forward, input >= 0 --
// the 4-way max + first-argmax as an integer max of keys (bf16 bits << 16 | 3 - d: larger value,
// then earlier pixel, wins), instead of a compare and two selects per pixel.  Bitwise
// lrn_pool_fwd_k / lrn_pool_bwd_k (tests/test_kernels_gpu.py test_lrn_pool_packed).
constexpr int LP14_C = 64, LP14_G = 8, LP14_HW = 14, LP14_OW = 7, LP14_NWIN = 49;
template <int R>
__global__ __launch_bounds__(TPB) void lrn_pool14_fwd_k(const bf16_t* __restrict__ x, int Nb, float bias, float alpha,
                                                        float beta, bf16_t* __restrict__ y, uint8_t* __restrict__ arg) {
  constexpr int C = LP14_C, G = LP14_G, HW = LP14_HW;
  const unsigned total = (unsigned)Nb * LP14_NWIN * G;
  const int c8 = threadIdx.x % G;
  const unsigned step = gridDim.x * TPB;
  for (unsigned base = blockIdx.x * TPB; base < total; base += 2 * step) {
    u32x4 xq[2][4];
    unsigned wk[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned t = base + k * step + threadIdx.x;
      const unsigned win = t < total ? t / G : 0u;
      wk[k] = win;
      const unsigned n = win / LP14_NWIN, rem = win - n * LP14_NWIN, oh = rem / LP14_OW, ow = rem - oh * LP14_OW;
      const bf16_t* p = x + ((int64_t)((n * HW + 2 * oh) * HW + 2 * ow)) * C + c8 * 8;
      xq[k][0] = *(const u32x4*)p;
      xq[k][1] = *(const u32x4*)(p + C);
      xq[k][2] = *(const u32x4*)(p + HW * C);
      xq[k][3] = *(const u32x4*)(p + HW * C + C);
    }
    int best[2][8];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      f2 v[8], sq[8], s[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = f2{u4_get(xq[0][d], j), u4_get(xq[1][d], j)};
        sq[j] = v[j] * v[j];
      }
      lane_window_sums2<G, R>(sq, c8, s);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f2 yv = lrn_out2(v[j], s[j], bias, alpha, beta);
        const uint32_t pk = pack2(yv.x, yv.y);   // window 0's bf16 low, window 1's high
        const int k0 = (int)((pk << 16) | (uint32_t)(3 - d)), k1 = (int)((pk & 0xffff0000u) | (uint32_t)(3 - d));
        best[0][j] = d == 0 ? k0 : max(best[0][j], k0);
        best[1][j] = d == 0 ? k1 : max(best[1][j], k1);
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const unsigned t = base + k * step + threadIdx.x;
      if (t < total) {
        u32x4 o;
        uint32_t cw[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = ((uint32_t)best[k][2 * j] >> 16) | ((uint32_t)best[k][2 * j + 1] & 0xffff0000u);
#pragma unroll
        for (int j = 0; j < 8; ++j) cw[j >> 2] |= (((uint32_t)best[k][j] & 3u) ^ 3u) << (8 * (j & 3));
        const int64_t off = (int64_t)wk[k] * C + c8 * 8;
        *(u32x4*)(y + off) = o;
        *(u32x2*)(arg + off) = u32x2{cw[0], cw[1]};
      }
    }
  }
}

template <int R>
__global__ __launch_bounds__(TPB) void lrn_pool14_bwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dP,
                                                        const uint8_t* __restrict__ arg, int Nb, float bias, float alpha,
                                                        float beta, int relu_mask, bf16_t* __restrict__ dx) {
  constexpr int C = LP14_C, G = LP14_G, HW = LP14_HW;
  const unsigned total = (unsigned)Nb * LP14_NWIN * G;
  const int c8 = threadIdx.x % G;
  for (unsigned base = blockIdx.x * TPB; base < total; base += gridDim.x * TPB) {
    const unsigned t = base + threadIdx.x;
    const bool ok = t < total;
    const unsigned win = ok ? t / G : 0u;
    const unsigned n = win / LP14_NWIN, rem = win - n * LP14_NWIN, oh = rem / LP14_OW, ow = rem - oh * LP14_OW;
    const int64_t poff = (int64_t)win * C + c8 * 8;
    const u32x4 pv = *(const u32x4*)(dP + poff);
    const u32x2 av = *(const u32x2*)(arg + poff);
    const int64_t x0 = ((int64_t)((n * HW + 2 * oh) * HW + 2 * ow)) * C + c8 * 8;
    u32x4 xq[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) xq[d] = *(const u32x4*)(x + x0 + ((d >> 1) * HW + (d & 1)) * C);
    float pg[8];
    unpack8(pv, pg);
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // pixels 2h, 2h + 1 (one row of the window) as the two halves
      f2 v[8], g[8], o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint32_t aj = ((j < 4 ? av[0] : av[1]) >> (8 * (j & 3))) & 0xffu;
        v[j] = f2{u4_get(xq[2 * h], j), u4_get(xq[2 * h + 1], j)};
        g[j] = f2{aj == (uint32_t)(2 * h) ? pg[j] : 0.f, aj == (uint32_t)(2 * h + 1) ? pg[j] : 0.f};
      }
      lrn_bwd2_b075<G, R>(v, g, c8, bias, alpha, beta, relu_mask, o);
      if (ok) {
        *(u32x4*)(dx + x0 + (h * HW) * C) =
            u32x4{pack2(o[0].x, o[1].x), pack2(o[2].x, o[3].x), pack2(o[4].x, o[5].x), pack2(o[6].x, o[7].x)};
        *(u32x4*)(dx + x0 + (h * HW + 1) * C) =
            u32x4{pack2(o[0].y, o[1].y), pack2(o[2].y, o[3].y), pack2(o[4].y, o[5].y), pack2(o[6].y, o[7].y)};
      }
    }
  }
}

}  // namespace

hipError_t maxpool_fwd(const bf16_t* x, int Nb, int H, int W, int C, int OH, int OW, bf16_t* y, uint8_t* arg,
                       hipStream_t st) {
  const int64_t total = (int64_t)Nb * OH * OW * (C / 8);
  hipLaunchKernelGGL(maxpool_fwd_k, dim3(nblocks(total, TPB, 16384)), dim3(TPB), 0, st, x, Nb, H, W, C, OH, OW, y,
                     arg);
  return hipGetLastError();
}

hipError_t maxpool_bwd(const bf16_t* dy, const uint8_t* arg, const bf16_t* y, int relu_mask, int Nb, int H, int W,
                       int C, int OH, int OW, bf16_t* dx, hipStream_t st) {
  const int64_t total = (int64_t)Nb * OH * OW * (C / 8);
  hipLaunchKernelGGL(maxpool_bwd_k, dim3(nblocks(total, TPB, 16384)), dim3(TPB), 0, st, dy, arg, y, relu_mask, Nb,
                     H, W, C, OH, OW, dx);
  return hipGetLastError();
}

#define LRN_CASE(KER, CC, RR, ...) \
  if (C == CC && r == RR) { hipLaunchKernelGGL((KER<CC, RR>), grid, dim3(TPB), 0, st, __VA_ARGS__); return hipGetLastError(); }
#define LRN_ALL(KER, ...)                                                                                     \
  LRN_CASE(KER, 8, 4, __VA_ARGS__) LRN_CASE(KER, 16, 4, __VA_ARGS__) LRN_CASE(KER, 32, 4, __VA_ARGS__)         \
  LRN_CASE(KER, 64, 4, __VA_ARGS__) LRN_CASE(KER, 32, 2, __VA_ARGS__) LRN_CASE(KER, 64, 2, __VA_ARGS__)        \
  LRN_CASE(KER, 32, 5, __VA_ARGS__) LRN_CASE(KER, 64, 5, __VA_ARGS__)

hipError_t lrn_fwd(const bf16_t* x, int P, int C, int r, float bias, float alpha, float beta, bf16_t* y,
                   hipStream_t st) {
  dim3 grid(nblocks((int64_t)P * (C / 8), TPB, 16384));   // one lane per 8-channel vector
  LRN_ALL(lrn_fwd_k, x, (int64_t)P, bias, alpha, beta, y)
  return hipErrorInvalidValue;  // (C, depth_radius) combination not instantiated
}

bool lrn_pool_supported(int H, int W, int C, int r) {
  return H % 2 == 0 && W % 2 == 0 && (C == 32 || C == 64) && r == 4;
}
// the packed 14 x 14 x 64 kernels (MNISTX_LRN_PK=0: the generic ones)
static int g_lrn_pk = [] { const char* e = getenv("MNISTX_LRN_PK"); return (e && e[0] == '0') ? 0 : 1; }();
void lrn_set_packed(int on) { g_lrn_pk = on; }
static bool lrn_pk14(int H, int W, int C, int r, int Nb) {
  return g_lrn_pk && H == LP14_HW && W == LP14_HW && C == LP14_C && r == 4 && (int64_t)Nb * LP14_NWIN * LP14_G < (1ll << 31);
}

hipError_t lrn_pool_fwd(const bf16_t* x, int Nb, int H, int W, int C, int r, float bias, float alpha, float beta,
                        bf16_t* y, uint8_t* arg, hipStream_t st, int nonneg) {
  if (!lrn_pool_supported(H, W, C, r)) return hipErrorInvalidValue;
  if (nonneg && lrn_pk14(H, W, C, r, Nb)) {
    if (Nb <= 0) return hipSuccess;
    dim3 grid(nblocks(((int64_t)Nb * LP14_NWIN * LP14_G + 1) / 2, TPB, 16384));
    hipLaunchKernelGGL((lrn_pool14_fwd_k<4>), grid, dim3(TPB), 0, st, x, Nb, bias, alpha, beta, y, arg);
    return hipGetLastError();
  }
  dim3 grid(nblocks(((int64_t)Nb * (H / 2) * (W / 2) * (C / 8) + LRNP_U - 1) / LRNP_U, TPB, 16384));
  if (C == 64) hipLaunchKernelGGL((lrn_pool_fwd_k<64, 4>), grid, dim3(TPB), 0, st, x, Nb, H, W, bias, alpha, beta, y, arg);
  else hipLaunchKernelGGL((lrn_pool_fwd_k<32, 4>), grid, dim3(TPB), 0, st, x, Nb, H, W, bias, alpha, beta, y, arg);
  return hipGetLastError();
}
hipError_t lrn_pool_bwd(const bf16_t* x, const bf16_t* dP, const uint8_t* arg, int Nb, int H, int W, int C, int r,
                        float bias, float alpha, float beta, int relu_mask, bf16_t* dx, hipStream_t st) {
  if (!lrn_pool_supported(H, W, C, r)) return hipErrorInvalidValue;
  dim3 grid(nblocks((int64_t)Nb * (H / 2) * (W / 2) * (C / 8), TPB, 16384));
  if (beta == 0.75f && lrn_pk14(H, W, C, r, Nb)) {
    if (Nb <= 0) return hipSuccess;
    hipLaunchKernelGGL((lrn_pool14_bwd_k<4>), grid, dim3(TPB), 0, st, x, dP, arg, Nb, bias, alpha, beta, relu_mask, dx);
    return hipGetLastError();
  }
#define LRN_PB(CC, BB) \
  hipLaunchKernelGGL((lrn_pool_bwd_k<CC, 4, BB>), grid, dim3(TPB), 0, st, x, dP, arg, Nb, H, W, bias, alpha, beta, relu_mask, dx)
  const bool b075 = beta == 0.75f;   // the reference's beta (lrn_math.h pow_beta)
  if (C == 64) {
    if (b075) LRN_PB(64, true);
    else LRN_PB(64, false);
  } else {
    if (b075) LRN_PB(32, true);
    else LRN_PB(32, false);
  }
#undef LRN_PB
  return hipGetLastError();
}

hipError_t lrn_bwd(const bf16_t* x, const bf16_t* dy, int P, int C, int r, float bias, float alpha, float beta,
                   int relu_mask, bf16_t* dx, hipStream_t st) {
  dim3 grid(nblocks((int64_t)P * (C / 8), TPB, 16384));
  if (beta == 0.75f && r == 4 && (C == 32 || C == 64)) {   // the reference CNN's layers: pow_beta<true>
    if (C == 32) hipLaunchKernelGGL((lrn_bwd_k<32, 4, true>), grid, dim3(TPB), 0, st, x, dy, (int64_t)P, bias, alpha, beta, relu_mask, dx);
    else hipLaunchKernelGGL((lrn_bwd_k<64, 4, true>), grid, dim3(TPB), 0, st, x, dy, (int64_t)P, bias, alpha, beta, relu_mask, dx);
    return hipGetLastError();
  }
  LRN_ALL(lrn_bwd_k, x, dy, (int64_t)P, bias, alpha, beta, relu_mask, dx)
  return hipErrorInvalidValue;
}

}  // namespace mnistx
