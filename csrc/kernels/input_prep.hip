// Input of the MNIST step on gfx950: the per-epoch shuffle as a kernel of its own (the
// permutation itself is perm.h) and input prep (K10), uint8 rows -> normalised bf16 NHWC.
#include "common.h"
#include "launchers.h"
#include "perm.h"
#include "tpb.h"

namespace mnistx {
namespace {

__global__ void perm_positions_k(int64_t* __restrict__ out, int64_t start, int n, int64_t N, uint32_t seed, int h,
                                 const int32_t* __restrict__ lab_src, int32_t* __restrict__ lab_out) {
  perm_one(blockIdx.x * blockDim.x + threadIdx.x, out, start, n, N, seed, h, lab_src, lab_out);
}

// ------------------------------------------------------------------ K10 input prep
// out[b, p, c] = src[idx[b], p, c_src] / 255 - 0.5   (mnist_input.py:39)
__global__ void prep_images_k(const uint8_t* __restrict__ src, const int64_t* __restrict__ idx,
                              const int32_t* __restrict__ lab_src, int B, int HW, int Csrc, int Cdst,
                              bf16_t* __restrict__ out, int32_t* __restrict__ lab_out) {
  const int64_t per_img = (int64_t)HW * Cdst;  // multiple of 8 (HW = 784)
  const int64_t nvec = (int64_t)B * per_img / 8;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = v * 8;
    const int64_t b = e / per_img;
    const int64_t w = e - b * per_img;
    const uint8_t* img = src + idx[b] * (int64_t)HW * Csrc;
    u32x4 o;
    if (Csrc == Cdst) {
      const uint8_t* s = img + w;
      uint32_t lo = *(const uint32_t*)s, hi = *(const uint32_t*)(s + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float a = u8_norm((lo >> (8 * j)) & 0xff);
        float c = u8_norm((hi >> (8 * j)) & 0xff);
        u4_set(o, j, f2bf(a));
        u4_set(o, j + 4, f2bf(c));
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t ww = w + j;
        const int64_t p = ww / Cdst;
        const int c = (int)(ww - p * Cdst);
        const int cs = c < Csrc ? c : 0;  // 1 -> 3 channel replication
        u4_set(o, j, f2bf(u8_norm(img[p * Csrc + cs])));
      }
    }
    *(u32x4*)(out + e) = o;
  }
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (lab_out && t < B) lab_out[t] = lab_src[idx[t]];
}

// Hot path of K10 (28x28x1 -> 28x28x1): 16 pixels per thread = one 16-byte gather
// load and two 16-byte bf16 stores, 49 vectors per image, 32-bit index math with a
// constant divisor (the generic kernel above does a 64-bit divide per 8 pixels).
// One thread per image also copies the label.
constexpr int PREP_V = 784 / 16;
__global__ __launch_bounds__(256) void prep_images_784_k(const uint8_t* __restrict__ src,
                                                          const int64_t* __restrict__ idx,
                                                          const int32_t* __restrict__ lab_src, int B,
                                                          bf16_t* __restrict__ out, int32_t* __restrict__ lab_out) {
  const int nvec = B * PREP_V;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += gridDim.x * blockDim.x) {
    const int b = v / PREP_V, w = v - b * PREP_V;
    const int64_t row = idx[b];
    const u32x4 px = *(const u32x4*)(src + row * 784 + 16 * w);
    u32x4 o0, o1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      o0[2 * j] = pack2(u8_norm(px[j] & 0xff), u8_norm((px[j] >> 8) & 0xff));
      o0[2 * j + 1] = pack2(u8_norm((px[j] >> 16) & 0xff), u8_norm(px[j] >> 24));
      o1[2 * j] = pack2(u8_norm(px[2 + j] & 0xff), u8_norm((px[2 + j] >> 8) & 0xff));
      o1[2 * j + 1] = pack2(u8_norm((px[2 + j] >> 16) & 0xff), u8_norm(px[2 + j] >> 24));
    }
    bf16_t* dst = out + (int64_t)b * 784 + 16 * w;
    *(u32x4*)dst = o0;
    *(u32x4*)(dst + 8) = o1;
    if (lab_out && w == 0) lab_out[b] = lab_src[row];
  }
}

// K10 hot path with the epoch shuffle fused in: the dataset row of batch entry b is
// the Feistel image of stream position start + b (perm_positions_k), computed by
// each thread (a few dozen integer ops) instead of by a separate launch + index array.
__global__ __launch_bounds__(256) void prep_images_784_perm_k(const uint8_t* __restrict__ src,
                                                               const int32_t* __restrict__ lab_src, int B,
                                                               int64_t start, int64_t N, uint32_t seed, int h,
                                                               bf16_t* __restrict__ out,
                                                               int32_t* __restrict__ lab_out) {
  const int nvec = B * PREP_V;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += gridDim.x * blockDim.x) {
    const int b = v / PREP_V, w = v - b * PREP_V;
    const int64_t p = start + b;
    const int64_t e = p / N;
    uint64_t x = (uint64_t)(p - e * N);
    const uint32_t ek = mix32((uint32_t)e ^ 0x9e3779b9u) ^ seed;
    uint32_t key[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) key[r] = mix32(ek + 0x85ebca77u * (uint32_t)(r + 1));
    do { x = feistel4(x, key, h); } while (x >= (uint64_t)N);
    const int64_t row = (int64_t)x;
    const u32x4 px = *(const u32x4*)(src + row * 784 + 16 * w);
    u32x4 o0, o1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      o0[2 * j] = pack2(u8_norm(px[j] & 0xff), u8_norm((px[j] >> 8) & 0xff));
      o0[2 * j + 1] = pack2(u8_norm((px[j] >> 16) & 0xff), u8_norm(px[j] >> 24));
      o1[2 * j] = pack2(u8_norm(px[2 + j] & 0xff), u8_norm((px[2 + j] >> 8) & 0xff));
      o1[2 * j + 1] = pack2(u8_norm((px[2 + j] >> 16) & 0xff), u8_norm(px[2 + j] >> 24));
    }
    bf16_t* dst = out + (int64_t)b * 784 + 16 * w;
    *(u32x4*)dst = o0;
    *(u32x4*)(dst + 8) = o1;
    if (w == 0) lab_out[b] = lab_src[row];
  }
}

}  // namespace

hipError_t perm_positions(int64_t* out, int64_t start, int n, int64_t N, uint32_t seed, int h, hipStream_t st,
                          const int32_t* lab_src, int32_t* lab_out) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(perm_positions_k, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, st, out, start, n, N, seed, h,
                     lab_src, lab_out);
  return hipGetLastError();
}

hipError_t prep_images_perm(const uint8_t* src, const int32_t* lab_src, int B, int64_t start, int64_t N,
                            uint32_t seed, int h, bf16_t* out, int32_t* lab_out, hipStream_t st) {
  if ((uintptr_t)src % 16 || (uintptr_t)out % 16 || (int64_t)B * PREP_V >= (1ll << 31)) return hipErrorInvalidValue;
  const int64_t nvec = (int64_t)B * PREP_V;
  hipLaunchKernelGGL(prep_images_784_perm_k, dim3(nblocks(nvec, 256, 8192)), dim3(256), 0, st, src, lab_src, B, start,
                     N, seed, h, out, lab_out);
  return hipGetLastError();
}

hipError_t prep_images(const uint8_t* src, const int64_t* idx, const int32_t* lab_src, int B, int HW, int Csrc,
                       int Cdst, bf16_t* out, int32_t* lab_out, hipStream_t st) {
  if (HW == 784 && Csrc == 1 && Cdst == 1 && (uintptr_t)src % 16 == 0 && (uintptr_t)out % 16 == 0 &&
      (int64_t)B * PREP_V < (1ll << 31)) {
    const int64_t nvec = (int64_t)B * PREP_V;
    hipLaunchKernelGGL(prep_images_784_k, dim3(nblocks(nvec, 256, 8192)), dim3(256), 0, st, src, idx, lab_src, B,
                       out, lab_out);
    return hipGetLastError();
  }
  const int64_t nvec = (int64_t)B * HW * Cdst / 8;
  int nb = nblocks(nvec, TPB, 8192);
  const int need = (B + TPB - 1) / TPB;
  if (nb < need) nb = need;
  hipLaunchKernelGGL(prep_images_k, dim3(nb), dim3(TPB), 0, st, src, idx, lab_src, B, HW, Csrc, Cdst, out, lab_out);
  return hipGetLastError();
}

}  // namespace mnistx
