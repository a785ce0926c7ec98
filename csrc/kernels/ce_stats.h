// Deterministic per-step cross-entropy statistics (loss sum, correct count, NaN
// flag) shared by the softmax-CE kernel (misc.hip) and the fused dense head
// (mlp_head.hip).  Each block reduces its threads in a fixed tree, writes one
// partial to `work`, and the last block to finish (ticket counter at
// work[4 * CE_MAXB]) combines the partials in block order: bitwise identical
// results across runs and between hipGraph replay and eager execution.
#pragma once
#include "common.h"

#include <type_traits>

constexpr int CE_MAXB = 1024;  // max blocks per launch (work holds 4 floats per block + ticket)

// Label smoothing.  The softmax-CE kernels take a compile-time SMOOTH switch; the smoothed
// instantiation has ONE more trailing kernel argument, eps (a `float` argument pack, empty in the
// plain instantiation, whose arguments and code therefore stay what they were).  With
// on = 1 - eps and off = eps / NC (NC = the real class count):
//   loss = log(se) - on * (l_y - mx) - off * sum_{c < NC} (l_c - mx)
//   dl_c = (p_c - on * [c == y] - off) * scale
// The class sum is over the differences, which stay finite for |l_c - mx| <= 1e37.
template <typename... T>
DEV float smooth_eps(T... eps) {
  static_assert(sizeof...(T) <= 1, "one eps at most");
  if constexpr (sizeof...(T) == 0) return 0.f;
  else return (eps + ...);
}

// Two labels per row (mixup / CutMix, mix.hip).  The MIX form of the same kernels is read off the
// pack's types: (eps, const int32_t* labels2, const float* lam [, ...]) instead of (eps); eps is
// always there and may be 0, so mixing and smoothing share one instantiation per kernel.  With
// ya = labels[m], yb = labels2[m], lam = lam[m] and om = 1 - lam:
//   loss = log(se) - on * (lam (l_ya - mx) + om (l_yb - mx)) - off * sum_{c < NC} (l_c - mx)
//   dl_c = (p_c - on * (lam [c == ya] + om [c == yb]) - off) * scale
// A row with lam == 1 drops the yb term by a select (mix_om, mix_logit), never by a product with 0:
// an infinite l_yb leaves such a row finite.  lam + om is exactly 1 for lam in [0.5, 1], so ya == yb
// gives `on` at that class.  The top-1 count stays l_ya >= mx: ya is the dominant label.
template <typename... T>
constexpr bool pack_has_mix = (std::is_same_v<T, const float*> || ...);
template <typename... R>
DEV float mix_eps(float e, const int32_t*, const float*, R...) { return e; }
template <typename... R>
DEV const int32_t* mix_labels2(float, const int32_t* l2, const float*, R...) { return l2; }
template <typename... R>
DEV const float* mix_lam(float, const int32_t*, const float* lm, R...) { return lm; }
// labels2[m] / lam[m]; the fused heads pass min(m, nb - 1), as their X loads do (a row past the batch
// is never stored or counted), so the loads sit under no branch and repeated calls merge into one
template <typename... A>
DEV int mix_row_label(int64_t m, A... a) { return mix_labels2(a...)[m]; }
template <typename... A>
DEV float mix_row_lam(int64_t m, A... a) { return mix_lam(a...)[m]; }
DEV float mix_om(float lam) { return lam < 1.f ? 1.f - lam : 0.f; }
// lam (l_ya - mx) + om (l_yb - mx) from da = l_ya - mx, db = l_yb - mx
DEV float mix_logit(float lam, float da, float db) { return lam < 1.f ? fmaf(lam, da, (1.f - lam) * db) : da; }
// the loss from tl = mix_logit(..), the class sum sd and lse = log(se).  eps = 0 (off == 0) leaves the
// class sum out by a select: a -inf logit in a class no label names makes sd -inf, and 0 * inf is NaN
DEV float mix_ce(float on, float off, float tl, float sd, float lse) {
  const float a = fmaf(-on, tl, lse);
  return off != 0.f ? fmaf(-off, sd, a) : a;
}
// the target of class c: on * (lam [c == ya] + om [c == yb]) + off
DEV float mix_target(int c, int ya, int yb, float lam, float om, float on, float off) {
  return fmaf(on, (c == ya ? lam : 0.f) + (c == yb ? om : 0.f), off);
}

// Every thread of the block must call this (it synchronises the block).
// With work == nullptr each block adds its partial atomically (order-dependent).
// defer: only write the block's partial; finalize_k combines them in block order in
// the step's last launch (no agent-scope fence here: each one writes back the L2,
// 11 us of the LeNet-5 head at B = 65536).
template <int NW>
DEV void ce_block_stats(float loss, float corr, float bad, float* __restrict__ stats, float* __restrict__ work,
                        bool defer = false) {
  __shared__ float red[3][NW];
  __shared__ int last;
  loss = warp_sum(loss);
  corr = warp_sum(corr);
  bad = warp_sum(bad);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = loss;
    red[1][wave] = corr;
    red[2][wave] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    loss = red[0][0];
    corr = red[1][0];
    bad = red[2][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      loss += red[0][w];
      corr += red[1][w];
      bad += red[2][w];
    }
    if (!work) {
      atomicAdd(&stats[0], loss);
      atomicAdd(&stats[1], corr);
      if (bad > 0.f) stats[2] = 1.f;
    } else {
      work[4 * blockIdx.x] = loss;
      work[4 * blockIdx.x + 1] = corr;
      work[4 * blockIdx.x + 2] = bad;
      if (defer) {
        last = 0;
      } else {
        __threadfence();
        unsigned* ticket = (unsigned*)(work + 4 * CE_MAXB);
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
      }
    }
  }
  if (!work) return;
  __syncthreads();
  if (!last) return;
  __threadfence();
  // last block: combine the partials in block order (64 lanes of wave 0, fixed tree)
  if (wave != 0) return;
  const volatile float* wv = work;
  float a = 0.f, b = 0.f, c = 0.f;
  for (int i = lane; i < (int)gridDim.x; i += 64) {
    a += wv[4 * i];
    b += wv[4 * i + 1];
    c += wv[4 * i + 2];
  }
  a = warp_sum(a);
  b = warp_sum(b);
  c = warp_sum(c);
  if (lane == 0) {
    stats[0] += a;
    stats[1] += b;
    if (c > 0.f) stats[2] = 1.f;
    *(unsigned*)(work + 4 * CE_MAXB) = 0u;
  }
}

// Deterministic per-block column sums of fp32 values (the last layer's bias gradient =
// sum over rows of dlogits, kept in fp32 as the reference's tf.float32 graph does:
// mnist_input.py:203-205 / 224-226): v[c] of every thread -> wave (fixed xor tree) ->
// waves in order -> out[c].  Every thread of the block must call this.
template <int NW, int LD>
DEV void block_colsum(const float (&v)[LD], float* __restrict__ out) {
  __shared__ float red[NW][LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < LD; ++c) {
    const float s = warp_sum(v[c]);
    if (lane == 0) red[wave][c] = s;
  }
  __syncthreads();
  if (threadIdx.x < LD) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += red[w][threadIdx.x];
    out[threadIdx.x] = s;
  }
}
