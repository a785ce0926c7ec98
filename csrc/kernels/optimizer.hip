// Fused optimizer + EMA + LR schedule (K9) with its norm passes (clipping, LARS / LAMB), the
// step finalisation (loss EMAs, global_step, NaN flag) and the fp32 -> padded bf16 cast.
// The eight optimizer kernels share one body, fused_opt_body.h, as a textual include.
#include "common.h"
#include "launchers.h"
#include "perm.h"
#include "ticket.h"
#include "tpb.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace mnistx {
namespace {

// ------------------------------------------------------------------ K9 fused optimizer
// Each workgroup owns one contiguous chunk of ONE segment (block -> segment
// table built on the host), so there is no per-element segment search and the
// L2 norm needed for the weight-decay loss is reduced in the workgroup and added
// with a single atomic per workgroup.
constexpr int MAXSEG = 16;
constexpr int FIN_WAVES = 4, FIN_MAXW = 64;
template <bool COH>
DEV void finalize_body(const FinArgs& f, float* wsum);
constexpr int OPT_EPT = 2;                       // elements per thread: one consecutive pair (fused_opt_k)
constexpr int OPT_CHUNK = TPB * OPT_EPT;         // elements per workgroup
struct SegTable {
  OptSeg s[MAXSEG];
  FastDiv fij[MAXSEG], fj[MAXSEG];   // I*J and J of each segment (bf16-copy index math)
  int blk0[MAXSEG + 1];
  int n;
  int l2n;                           // l2[0..l2n): per-tensor sums; l2[l2n + block]: partials
};

// Clipping by global norm: the pieces fused_opt_body.h uses under CLIP (kernels further down).
constexpr int GN_BLOCKS = 512;   // grid of grad_sqnorm_k = partials every optimizer block sums
constexpr int GN_UNROLL = 4;     // full chunks whose loads grad_sqnorm_k issues together
static_assert(GN_BLOCKS <= 1024 && GN_BLOCKS % TPB == 0, "gn_total: GN_BLOCKS / TPB partials per thread");
// sqrt of the sum of the GN_BLOCKS partials gnorm[2 ..], the same bits in every thread of every
// block that calls it: thread t adds partials t, t + TPB, ... in order, then warp_sum, then the
// waves in index order.  gred: TPB / 64 floats of LDS.  Contains a __syncthreads.
DEV float gn_total(const float* gnorm, float* gred) {
  constexpr int R = GN_BLOCKS / TPB;
  float v[R];
#pragma unroll
  for (int u = 0; u < R; ++u) v[u] = gnorm[2 + threadIdx.x + u * TPB];
  float t = 0.f;
#pragma unroll
  for (int u = 0; u < R; ++u) t += v[u];
  t = warp_sum(t);
  if ((threadIdx.x & 63) == 0) gred[threadIdx.x >> 6] = t;
  __syncthreads();
  float ss = 0.f;
#pragma unroll
  for (int w = 0; w < TPB / 64; ++w) ss += gred[w];
  return sqrtf(ss);
}
// s = c / max(gn, c): exactly 1 for gn <= c (gn = 0 included); NaN for a non-finite gn, as
// tf.clip_by_global_norm (fmaxf would return c for a NaN norm and hide it)
DEV float clip_scale(float gn, float c) {
  if (!isfinite(gn)) return __builtin_nanf("");
  return c / (gn <= c ? c : gn);
}
// g * s as a multiply of its own: kept out of the rule's fused multiply-adds, so that s = 1
// leaves every rule bitwise what it is without clipping
DEV float clip_mul(float g, float s) {
#pragma clang fp contract(off)
  return g * s;
}

// Layer-wise trust ratios (OPT_LARS / OPT_LAMB): the pieces fused_opt_body.h and the norm kernels
// share.  tnorm: [3 k] ||p_k||  [3 k + 1] ||g_k|| (LARS) or ||u_k|| (LAMB)  [3 k + 2] r_k, then
// per variable k GN_BLOCKS pairs (sum p^2, sum g^2 or u^2), one per block of var_sqnorm_k.
DEV float* lw_parts(float* tnorm, int nvar, int k) { return tnorm + 3 * nvar + (size_t)k * (2 * GN_BLOCKS); }
// g_eff as the unclipped kernels contract it: the gradient's product rounded, the decay's fused
DEV float lw_geff(float p, float g, float grad_scale, float wd) {
#pragma clang fp contract(off)
  return __builtin_fmaf(wd, p, g * grad_scale);
}
// LAMB's reciprocal bias corrections 1 / (1 - b^t), t = step + 1, as -expm1(t log b) in double
DEV void lamb_corr(int64_t step, const OptParams& op, float& ic1, float& ic2) {
  const double t = (double)(step + 1);
  ic1 = (float)(1.0 / -expm1(t * op.log_b1));
  ic2 = (float)(1.0 / -expm1(t * op.log_b2));
}
// LAMB's new m, v and u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps), contraction pinned:
// the norm pass and the apply pass get the same bits from the same inputs
DEV float lamb_u(float m0, float v0, float g, const OptParams& op, float ic1, float ic2, float& m, float& v) {
#pragma clang fp contract(off)
  m = op.b1 * m0 + op.omb1 * g;
  v = op.b2 * v0 + op.omb2 * (g * g);
  return (m * ic1) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v * ic2) + op.eps);
}
// The two sums of one variable over the var_sqnorm_k blocks that walked one of its chunks
// [c_lo, c_hi) -- every other block stored 0 -- the same bits in every thread of every block
// that calls it: thread t adds blocks b_lo + t, b_lo + t + TPB, ... in order, then warp_sum, then
// the waves in index order.  red: 2 * TPB / 64 floats of LDS.  Contains a __syncthreads.
DEV void lw_var_sums(const float* part, int c_lo, int c_hi, int per, float* red, float& sp, float& su) {
  float a = 0.f, b = 0.f;
  if (c_hi > c_lo) {
    const int b_hi = (c_hi - 1) / per;
    for (int blk = c_lo / per + (int)threadIdx.x; blk <= b_hi; blk += TPB) {
      a += part[2 * blk];
      b += part[2 * blk + 1];
    }
  }
  a = warp_sum(a);
  b = warp_sum(b);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = a;
    red[TPB / 64 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  sp = 0.f;
  su = 0.f;
#pragma unroll
  for (int w = 0; w < TPB / 64; ++w) {
    sp += red[w];
    su += red[TPB / 64 + w];
  }
}
// r_k from the two sums; pn, un: the norms.  A non-finite norm of an adapted variable gives NaN
// (the > 0 tests alone would turn a NaN norm into ratio 1 and hide it)
DEV float lw_ratio(bool lamb, int adapt, float sp, float su, float eta, float eps, float& pn, float& un) {
  pn = sqrtf(sp);
  un = sqrtf(su);
  if (!adapt) return 1.f;
  if (!isfinite(pn) || !isfinite(un)) return __builtin_nanf("");
  if (!(pn > 0.f && un > 0.f)) return 1.f;
  return lamb ? pn / un : eta * pn / (un + eps);
}

// The learning rate at global step t (LrSched, launchers.h), in fp32 as written there; every
// product and sum is an operation of its own.  The staircase is the optimizer body's own line.
// For polynomial and cosine, t >= T returns lr_end itself and t <= W (x = 0) takes lr0 itself, so
// neither end depends on how powf or cosf round.  Block-uniform in the optimizer kernels.
DEV float sched_lr(float lr0, float decay_rate, int64_t decay_steps, const LrSched& sc, int64_t t) {
#pragma clang fp contract(off)
  const int64_t W = sc.warmup, T = sc.total;
  float base = lr0;
  if (sc.kind == LR_STAIRCASE) {
    if (decay_steps > 0) base *= powf(decay_rate, (float)(t / decay_steps));
  } else {
    if (t >= T) return sc.lr_end;   // T > W: the warmup is over
    if (t > W) {
      const float x = (float)(t - W) / (float)(T - W);
      const float shape = sc.kind == LR_POLYNOMIAL ? powf(1.f - x, sc.power) : 0.5f * (1.f + cosf(3.14159265358979f * x));
      base = sc.lr_end + (lr0 - sc.lr_end) * shape;
    }
  }
  if (W > 0 && t < W) return (float)(t + 1) / (float)W * base;
  return base;
}

// sched_lr for a vector of steps: what lr_at_steps() shows is what the optimizer kernels apply
__global__ __launch_bounds__(TPB) void lr_at_steps_k(const int64_t* __restrict__ steps, float* __restrict__ out,
                                                     int64_t n, float lr0, float decay_rate, int64_t decay_steps,
                                                     LrSched sc) {
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
    out[i] = sched_lr(lr0, decay_rate, decay_steps, sc, steps[i]);
}

__global__ __launch_bounds__(TPB) void fused_opt_k(float* __restrict__ params, const float* __restrict__ grads,
                                                   float* __restrict__ mom, float* __restrict__ ema,
                                                   bf16_t* __restrict__ bf, SegTable tab,
                                                   const int64_t* __restrict__ step_p, OptParams op,
                                                   float* __restrict__ l2, FinArgs fin, PermJob pj) {
  constexpr int RULE = OPT_CLASSIC;   // SGD / momentum / Nesterov, chosen at run time by OptParams
  constexpr bool CLIP = false;
  float* const slot2 = nullptr;
  float* const gnorm = nullptr;
  const float clip_norm = 0.f;
  constexpr bool LW_SELF = false;   // OPT_LARS / OPT_LAMB: layerwise_opt_k only
  float* const tnorm = nullptr;
  const float lars_eta = 0.f;
  const int lw_per = 1;
  constexpr bool SCHED = false;     // warmup / polynomial / cosine: the *_sched_k kernels only
  const LrSched sc{};
#include "fused_opt_body.h"
}

// fused_opt_k with the rate from sched_lr (a kernel of its own: fused_opt_k's code and arguments
// stay what they are)
__global__ __launch_bounds__(TPB) void fused_opt_sched_k(float* __restrict__ params, const float* __restrict__ grads,
                                                         float* __restrict__ mom, float* __restrict__ ema,
                                                         bf16_t* __restrict__ bf, SegTable tab,
                                                         const int64_t* __restrict__ step_p, OptParams op,
                                                         float* __restrict__ l2, FinArgs fin, PermJob pj, LrSched sc) {
  constexpr int RULE = OPT_CLASSIC;
  constexpr bool CLIP = false;
  float* const slot2 = nullptr;
  float* const gnorm = nullptr;
  const float clip_norm = 0.f;
  constexpr bool LW_SELF = false;
  float* const tnorm = nullptr;
  const float lars_eta = 0.f;
  const int lw_per = 1;
  constexpr bool SCHED = true;
#include "fused_opt_body.h"
}

// Adam / RMSProp / Adagrad (OptParams): the same body with the rule fixed at compile time and a
// second slot pointer
template <int RULE>
__global__ __launch_bounds__(TPB) void adaptive_opt_k(float* __restrict__ params, const float* __restrict__ grads,
                                                      float* __restrict__ mom, float* __restrict__ slot2,
                                                      float* __restrict__ ema, bf16_t* __restrict__ bf, SegTable tab,
                                                      const int64_t* __restrict__ step_p, OptParams op,
                                                      float* __restrict__ l2, FinArgs fin, PermJob pj) {
  constexpr bool CLIP = false;
  float* const gnorm = nullptr;
  const float clip_norm = 0.f;
  constexpr bool LW_SELF = false;   // OPT_LARS / OPT_LAMB: layerwise_opt_k only
  float* const tnorm = nullptr;
  const float lars_eta = 0.f;
  const int lw_per = 1;
  constexpr bool SCHED = false;
  const LrSched sc{};
#include "fused_opt_body.h"
}

template <int RULE>
__global__ __launch_bounds__(TPB) void adaptive_opt_sched_k(float* __restrict__ params, const float* __restrict__ grads,
                                                            float* __restrict__ mom, float* __restrict__ slot2,
                                                            float* __restrict__ ema, bf16_t* __restrict__ bf,
                                                            SegTable tab, const int64_t* __restrict__ step_p,
                                                            OptParams op, float* __restrict__ l2, FinArgs fin,
                                                            PermJob pj, LrSched sc) {
  constexpr bool CLIP = false;
  float* const gnorm = nullptr;
  const float clip_norm = 0.f;
  constexpr bool LW_SELF = false;
  float* const tnorm = nullptr;
  const float lars_eta = 0.f;
  const int lw_per = 1;
  constexpr bool SCHED = true;
#include "fused_opt_body.h"
}

// Clipping by global norm (tf.clip_by_global_norm of the gradient the rules consume,
// g_eff = grad * grad_scale + wd * p, over ALL segments): grad_sqnorm_k, then clipped_opt_k<RULE>
// on the same stream.  gnorm: [0] global norm  [1] scale s  [2 + b] block b's sum(g_eff^2).
// Every sum runs in a fixed order and nothing is handed over between blocks of one launch: no
// atomics, no ticket (red_tickets cannot be taken under capture, and one ticket address
// serialises a large grid), so replay is bitwise equal to eager at any size.
//
// Block b of the GN_BLOCKS-block grid owns chunks [b * per, (b + 1) * per) of the optimizer's
// own (segment, OPT_CHUNK) decomposition and walks them in order; a block past the last chunk
// stores 0.  Runs of GN_UNROLL full chunks of a segment at an even offset issue all their
// 8-byte loads before the first use; every other chunk goes through the optimizer body's pair /
// scalar-tail paths, one at a time.  Each thread adds its elements in chunk order.
DEV float gn_term(float acc, float p, float g, float grad_scale, float wd) {
  const float ge = g * grad_scale + wd * p;
  return acc + ge * ge;
}

__global__ __launch_bounds__(TPB) void grad_sqnorm_k(const float* __restrict__ params, const float* __restrict__ grads,
                                                     SegTable tab, float grad_scale, int per,
                                                     float* __restrict__ gnorm) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  __shared__ float red[TPB / 64];
  const int nc = tab.blk0[tab.n];
  const int c0 = min(nc, (int)blockIdx.x * per), c1 = min(nc, c0 + per);
  float acc = 0.f;
  int si = 0, c = c0;
  while (c < c1) {
    while (si + 1 < tab.n && c >= tab.blk0[si + 1]) ++si;
    const int64_t off = tab.s[si].off, n = tab.s[si].n;
    const float wd = tab.s[si].wd;
    const int64_t lo = (int64_t)(c - tab.blk0[si]) * OPT_CHUNK;
    const bool even = (off & 1) == 0;
    if (even && c + GN_UNROLL <= c1 && lo + GN_UNROLL * OPT_CHUNK <= n) {
      const int64_t e = off + lo + 2 * (int64_t)threadIdx.x;
      f32x2_t p2[GN_UNROLL], g2[GN_UNROLL];
#pragma unroll
      for (int u = 0; u < GN_UNROLL; ++u) {
        p2[u] = *(const f32x2_t*)(params + e + u * OPT_CHUNK);
        g2[u] = *(const f32x2_t*)(grads + e + u * OPT_CHUNK);
      }
#pragma unroll
      for (int u = 0; u < GN_UNROLL; ++u) {
        acc = gn_term(acc, p2[u][0], g2[u][0], grad_scale, wd);
        acc = gn_term(acc, p2[u][1], g2[u][1], grad_scale, wd);
      }
      c += GN_UNROLL;
      continue;
    }
    // out-of-range elements load element 0 and are never added
    const int64_t li0 = lo + 2 * (int64_t)threadIdx.x;
    float pv[OPT_EPT], gv[OPT_EPT];
    if (even && li0 + 1 < n) {
      const f32x2_t p2 = *(const f32x2_t*)(params + off + li0), g2 = *(const f32x2_t*)(grads + off + li0);
#pragma unroll
      for (int u = 0; u < OPT_EPT; ++u) {
        pv[u] = p2[u];
        gv[u] = g2[u];
      }
    } else {
#pragma unroll
      for (int u = 0; u < OPT_EPT; ++u) {
        const int64_t li = li0 + u;
        const int64_t e = off + (li < n ? li : 0);
        pv[u] = params[e];
        gv[u] = grads[e];
      }
    }
#pragma unroll
    for (int u = 0; u < OPT_EPT; ++u)
      if (li0 + u < n) acc = gn_term(acc, pv[u], gv[u], grad_scale, wd);
    ++c;
  }
  acc = warp_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < TPB / 64; ++w) t += red[w];
    gnorm[2 + blockIdx.x] = t;
  }
}

// grad_global_norm's last step (not on the training path, where every optimizer block does this)
__global__ __launch_bounds__(TPB) void gnorm_finish_k(float* __restrict__ gnorm) {
  __shared__ float gred[TPB / 64];
  const float gn = gn_total(gnorm, gred);
  if (threadIdx.x == 0) gnorm[0] = gn;
}

// the optimizer body compiled with clipping, one instance per rule (slot2: as adaptive_opt_k;
// unused by OPT_CLASSIC)
template <int RULE>
__global__ __launch_bounds__(TPB) void clipped_opt_k(float* __restrict__ params, const float* __restrict__ grads,
                                                     float* __restrict__ mom, float* __restrict__ slot2,
                                                     float* __restrict__ ema, bf16_t* __restrict__ bf, SegTable tab,
                                                     const int64_t* __restrict__ step_p, OptParams op,
                                                     float* __restrict__ l2, FinArgs fin, PermJob pj,
                                                     float* __restrict__ gnorm, float clip_norm) {
  constexpr bool CLIP = true;
  constexpr bool LW_SELF = false;
  float* const tnorm = nullptr;
  const float lars_eta = 0.f;
  const int lw_per = 1;
  constexpr bool SCHED = false;
  const LrSched sc{};
#include "fused_opt_body.h"
}

template <int RULE>
__global__ __launch_bounds__(TPB) void clipped_opt_sched_k(float* __restrict__ params, const float* __restrict__ grads,
                                                           float* __restrict__ mom, float* __restrict__ slot2,
                                                           float* __restrict__ ema, bf16_t* __restrict__ bf,
                                                           SegTable tab, const int64_t* __restrict__ step_p,
                                                           OptParams op, float* __restrict__ l2, FinArgs fin,
                                                           PermJob pj, float* __restrict__ gnorm, float clip_norm,
                                                           LrSched sc) {
  constexpr bool CLIP = true;
  constexpr bool LW_SELF = false;
  float* const tnorm = nullptr;
  const float lars_eta = 0.f;
  const int lw_per = 1;
  constexpr bool SCHED = true;
#include "fused_opt_body.h"
}

// Layer-wise trust ratios (OPT_LARS / OPT_LAMB): var_sqnorm_k<LAMB>, then var_ratio_k or none,
// then layerwise_opt_k<RULE, SELF> on the same stream.  var_sqnorm_k is grad_sqnorm_k per
// variable: the same chunk decomposition over GN_BLOCKS blocks and the same unrolled / pair /
// scalar-tail load paths, but two running sums -- p^2 and g_eff^2 (LARS) or u^2 (LAMB, whose new
// m, v and u are formed in registers from mom and slot2 and never stored) -- that the block
// flushes to the slot of (variable, block) whenever its chunk range leaves a variable.  A block
// stores 0 for every variable it holds no chunk of, so nothing stale survives, and no slot is
// written twice.  Read-only apart from the partials; no atomics, no ticket.
DEV void lw_flush(float a, float b, float* red, float* dst) {
  a = warp_sum(a);
  b = warp_sum(b);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = a;
    red[TPB / 64 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float ta = 0.f, tb = 0.f;
    for (int w = 0; w < TPB / 64; ++w) {
      ta += red[w];
      tb += red[TPB / 64 + w];
    }
    dst[0] = ta;
    dst[1] = tb;
  }
  __syncthreads();   // red is free for the next variable's flush
}

template <bool LAMB>
DEV void lw_term(float& ap, float& au, float p, float g, float m0, float v0, float wd, const OptParams& op, float ic1,
                 float ic2) {
  float x = lw_geff(p, g, op.grad_scale, wd);
  if constexpr (LAMB) {
    float m, v;
    x = lamb_u(m0, v0, x, op, ic1, ic2, m, v);
  }
  ap += p * p;
  au += x * x;
}

template <bool LAMB>
__global__ __launch_bounds__(TPB) void var_sqnorm_k(const float* __restrict__ params, const float* __restrict__ grads,
                                                    const float* __restrict__ mom, const float* __restrict__ slot2,
                                                    SegTable tab, const int64_t* __restrict__ step_p, OptParams op,
                                                    int per, float* __restrict__ tnorm) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  __shared__ float red[2 * (TPB / 64)];
  float ic1 = 1.f, ic2 = 1.f;
  if constexpr (LAMB) {
    __shared__ float lcorr[2];
    if (threadIdx.x == 0) lamb_corr(*step_p, op, lcorr[0], lcorr[1]);
    __syncthreads();
    ic1 = lcorr[0];
    ic2 = lcorr[1];
  }
  const int nc = tab.blk0[tab.n];
  const int c0 = min(nc, (int)blockIdx.x * per), c1 = min(nc, c0 + per);
  float ap = 0.f, au = 0.f;
  int si = 0, c = c0, cur = -1;
  uint32_t done = 0;   // variables this block has flushed (MAXSEG <= 32)
  while (c < c1) {
    while (si + 1 < tab.n && c >= tab.blk0[si + 1]) ++si;
    if (si != cur) {   // the chunk range crossed into another variable
      if (cur >= 0) {
        lw_flush(ap, au, red, lw_parts(tnorm, tab.n, cur) + 2 * blockIdx.x);
        done |= 1u << cur;
        ap = au = 0.f;
      }
      cur = si;
    }
    const int64_t off = tab.s[si].off, n = tab.s[si].n;
    const float wd = tab.s[si].wd;
    const int64_t lo = (int64_t)(c - tab.blk0[si]) * OPT_CHUNK;
    const bool even = (off & 1) == 0;
    if (even && c + GN_UNROLL <= c1 && lo + GN_UNROLL * OPT_CHUNK <= n) {
      const int64_t e = off + lo + 2 * (int64_t)threadIdx.x;
      f32x2_t p2[GN_UNROLL], g2[GN_UNROLL], m2[GN_UNROLL], s2[GN_UNROLL];
#pragma unroll
      for (int u = 0; u < GN_UNROLL; ++u) {
        p2[u] = *(const f32x2_t*)(params + e + u * OPT_CHUNK);
        g2[u] = *(const f32x2_t*)(grads + e + u * OPT_CHUNK);
        if constexpr (LAMB) {
          m2[u] = *(const f32x2_t*)(mom + e + u * OPT_CHUNK);
          s2[u] = *(const f32x2_t*)(slot2 + e + u * OPT_CHUNK);
        } else {
          m2[u] = s2[u] = f32x2_t{0.f, 0.f};
        }
      }
#pragma unroll
      for (int u = 0; u < GN_UNROLL; ++u) {
        lw_term<LAMB>(ap, au, p2[u][0], g2[u][0], m2[u][0], s2[u][0], wd, op, ic1, ic2);
        lw_term<LAMB>(ap, au, p2[u][1], g2[u][1], m2[u][1], s2[u][1], wd, op, ic1, ic2);
      }
      c += GN_UNROLL;
      continue;
    }
    // out-of-range elements load element 0 and are never added
    const int64_t li0 = lo + 2 * (int64_t)threadIdx.x;
    float pv[OPT_EPT], gv[OPT_EPT], mv[OPT_EPT], sv[OPT_EPT];
    if (even && li0 + 1 < n) {
      const f32x2_t p2 = *(const f32x2_t*)(params + off + li0), g2 = *(const f32x2_t*)(grads + off + li0);
      f32x2_t m2 = {0.f, 0.f}, s2 = {0.f, 0.f};
      if constexpr (LAMB) {
        m2 = *(const f32x2_t*)(mom + off + li0);
        s2 = *(const f32x2_t*)(slot2 + off + li0);
      }
#pragma unroll
      for (int u = 0; u < OPT_EPT; ++u) {
        pv[u] = p2[u];
        gv[u] = g2[u];
        mv[u] = m2[u];
        sv[u] = s2[u];
      }
    } else {
#pragma unroll
      for (int u = 0; u < OPT_EPT; ++u) {
        const int64_t li = li0 + u;
        const int64_t e = off + (li < n ? li : 0);
        pv[u] = params[e];
        gv[u] = grads[e];
        mv[u] = sv[u] = 0.f;
        if constexpr (LAMB) {
          mv[u] = mom[e];
          sv[u] = slot2[e];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < OPT_EPT; ++u)
      if (li0 + u < n) lw_term<LAMB>(ap, au, pv[u], gv[u], mv[u], sv[u], wd, op, ic1, ic2);
    ++c;
  }
  if (cur >= 0) {
    lw_flush(ap, au, red, lw_parts(tnorm, tab.n, cur) + 2 * blockIdx.x);
    done |= 1u << cur;
  }
  if ((int)threadIdx.x < tab.n && !((done >> threadIdx.x) & 1u)) {
    float* z = lw_parts(tnorm, tab.n, threadIdx.x) + 2 * blockIdx.x;
    z[0] = 0.f;
    z[1] = 0.f;
  }
}

// norms and ratio of variable blockIdx.x from its partials: the hand-off launch (and var_norms')
__global__ __launch_bounds__(TPB) void var_ratio_k(SegTable tab, int lamb, float lars_eta, float eps, int per,
                                                   float* __restrict__ tnorm) {
  __shared__ float lred[2 * (TPB / 64)];
  const int k = blockIdx.x;
  float sp, su, pn, un;
  lw_var_sums(lw_parts(tnorm, tab.n, k), tab.blk0[k], tab.blk0[k + 1], per, lred, sp, su);
  const float r = lw_ratio(lamb != 0, tab.s[k].adapt, sp, su, lars_eta, eps, pn, un);
  if (threadIdx.x == 0) {
    tnorm[3 * k] = pn;
    tnorm[3 * k + 1] = un;
    tnorm[3 * k + 2] = r;
  }
}

// the optimizer body compiled for the layer-wise rules (RULE = OPT_LARS, OPT_LAMB); SELF: every
// block sums its own variable's partials, else it reads the ratio var_ratio_k wrote
template <int RULE, bool SELF>
__global__ __launch_bounds__(TPB) void layerwise_opt_k(float* __restrict__ params, const float* __restrict__ grads,
                                                       float* __restrict__ mom, float* __restrict__ slot2,
                                                       float* __restrict__ ema, bf16_t* __restrict__ bf, SegTable tab,
                                                       const int64_t* __restrict__ step_p, OptParams op,
                                                       float* __restrict__ l2, FinArgs fin, PermJob pj,
                                                       float* __restrict__ tnorm, float lars_eta, int lw_per) {
  static_assert(RULE == OPT_LARS || RULE == OPT_LAMB, "layerwise_opt_k: the layer-wise rules only");
  constexpr bool CLIP = false;
  constexpr bool LW_SELF = SELF;
  float* const gnorm = nullptr;
  const float clip_norm = 0.f;
  constexpr bool SCHED = false;
  const LrSched sc{};
#include "fused_opt_body.h"
}

template <int RULE, bool SELF>
__global__ __launch_bounds__(TPB) void layerwise_opt_sched_k(float* __restrict__ params, const float* __restrict__ grads,
                                                             float* __restrict__ mom, float* __restrict__ slot2,
                                                             float* __restrict__ ema, bf16_t* __restrict__ bf,
                                                             SegTable tab, const int64_t* __restrict__ step_p,
                                                             OptParams op, float* __restrict__ l2, FinArgs fin,
                                                             PermJob pj, float* __restrict__ tnorm, float lars_eta,
                                                             int lw_per, LrSched sc) {
  static_assert(RULE == OPT_LARS || RULE == OPT_LAMB, "layerwise_opt_sched_k: the layer-wise rules only");
  constexpr bool CLIP = false;
  constexpr bool LW_SELF = SELF;
  float* const gnorm = nullptr;
  const float clip_norm = 0.f;
  constexpr bool SCHED = true;
#include "fused_opt_body.h"
}

// stats: [0] ce_sum acc [1] correct acc [2] nan flag [3] -
//        [4] ce_mean [5] accuracy [6] total_loss [7] steps done (float)
// loss_ema: n_ema x {biased, local_step, avg}  (TF zero-debiased EMA, decay 0.9:
//           mnist_input.py:288-290); order = weight losses..., cross_entropy, total_loss
static_assert(64 * FIN_WAVES == TPB, "finalize_body also runs as the last block of fused_opt_k");
// the body of finalize_k, run by one TPB-thread block: by finalize_k, or by the last block of
// fused_opt_k (FinArgs::ticket set), which then replaces the separate launch
template <bool COH>   // COH: the optimizer's l2 partials of this launch, read coherently
DEV void finalize_body(const FinArgs& f, float* wsum) {
  int64_t* step = f.step;
  float* stats = f.stats;
  float* l2 = f.l2;
  const int* l2r = f.l2r;
  const int l2base = f.l2base, nw = f.nw, n_ema = f.n_ema, batch = f.batch, increment = f.increment;
  const float* wds = f.wds;
  float* loss_ema = f.loss_ema;
  const float* ce_work = f.ce_work;
  const int ce_nblk = f.ce_nblk;
  // wave 0 lane i owns loss entry i (weight losses..., cross_entropy, total_loss), so the
  // EMA read-modify-writes run in parallel instead of as one dependent chain.  The per-
  // weight sum(w^2) partials are summed by all FIN_WAVES waves (weight w by wave w %
  // FIN_WAVES, the same per-weight order as one wave): their load latencies overlap
  // instead of queueing behind each other (LeNet: 5 weights, ~11 -> ~5 us).
  const int t = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // wave 0: the CE partials and every per-lane input of the EMA update, loaded up front;
  // waves 1..FIN_WAVES-1: the per-weight sum(w^2) partials -- the two phases' memory
  // round trips overlap instead of following each other
  float ce_sum = 0.f, corr_sum = 0.f, l2t = 0.f, wdt = 0.f, e0 = 0.f, e1 = 0.f;
  if (wv == 0) {
    ce_sum = stats[0];
    corr_sum = stats[1];
    if (l2 && t < nw) l2t = l2[t];
    if (t < nw) wdt = wds[t];
    if (loss_ema && t < n_ema && t < nw + 2) {
      e0 = loss_ema[3 * t];
      e1 = loss_ema[3 * t + 1];
    }
    if (ce_nblk > 0) {
      // deferred CE partials (ce_block_stats defer): the same lane-strided, fixed-tree sum as
      // the ticket combine's last block, so the loss is bitwise what that path produced;
      // 8 partials per lane in flight per round, summed in the same per-lane order
      float a = 0.f, b = 0.f, c = 0.f;
      int i = t;
      for (; i + 7 * 64 < ce_nblk; i += 8 * 64) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *(const f32x4*)(ce_work + 4 * (i + 64 * u));
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          a += v[u][0];
          b += v[u][1];
          c += v[u][2];
        }
      }
      for (; i < ce_nblk; i += 64) {
        a += ce_work[4 * i];
        b += ce_work[4 * i + 1];
        c += ce_work[4 * i + 2];
      }
      a = warp_sum(a);
      b = warp_sum(b);
      c = warp_sum(c);
      ce_sum += a;
      corr_sum += b;
      if (t == 0 && c > 0.f) stats[2] = 1.f;
    }
  } else if (l2 && l2r) {
    for (int w = wv - 1; w < nw && w < FIN_MAXW; w += FIN_WAVES - 1) {
      const int b0 = l2r[3 * w + 1], b1 = l2r[3 * w + 2];
      // 4 independent chains per lane, combined in a fixed order; 16 loads in flight per
      // round (the reference CNN's local3 has thousands of partials: 4 per round left this
      // wave's round trips most of finalize_k's ~11 us)
      float s4[4] = {0.f, 0.f, 0.f, 0.f};
      int b = b0 + t;
      for (; b + 64 * 15 < b1; b += 64 * 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = COH ? ld_coh(l2 + l2base + b + 64 * u) : l2[l2base + b + 64 * u];
#pragma unroll
        for (int u = 0; u < 16; ++u) s4[u & 3] += v[u];
      }
      for (; b + 192 < b1; b += 256) {
#pragma unroll
        for (int u = 0; u < 4; ++u) s4[u] += COH ? ld_coh(l2 + l2base + b + 64 * u) : l2[l2base + b + 64 * u];
      }
      for (; b < b1; b += 64) s4[0] += COH ? ld_coh(l2 + l2base + b) : l2[l2base + b];
      float sum = (s4[0] + s4[1]) + (s4[2] + s4[3]);
      sum = warp_sum(sum);
      if (t == 0) wsum[w] = sum;
    }
  }
  __syncthreads();
  if (wv != 0) return;
  const float ce = ce_sum / (float)batch;
  const float acc = corr_sum / (float)batch;
  // sum(w^2) of weight t: the fused optimizer's per-block partials l2[l2base + b],
  // b in [l2r[3w+1], l2r[3w+2]), summed by the whole wave in a fixed order
  float l2v = l2t;
  if (l2 && l2r)
    for (int w = 0; w < nw && w < FIN_MAXW; ++w)
      if (t == l2r[3 * w]) l2v += wsum[w];
  const float wl = t < nw ? wdt * 0.5f * l2v : 0.f;
  float total = ce;
  for (int i = 0; i < nw; ++i) total += __shfl(wl, i, 64);   // fixed order (bitwise as before)
  if (loss_ema && t < n_ema && t < nw + 2) {
    const float v = t < nw ? wl : (t == nw ? ce : total);
    float* e = loss_ema + 3 * t;
    const float b = 0.9f * e0 + 0.1f * v, n = e1 + 1.f;
    e[0] = b;
    e[1] = n;
    e[2] = b / (1.f - powf(0.9f, n));
  }
  if (l2 && t < nw) l2[t] = 0.f;
  if (t != 0) return;
  stats[4] = ce;
  stats[5] = acc;
  stats[6] = total;
  stats[7] += 1.f;
  if (!isfinite(total)) stats[2] = 1.f;
  stats[0] = 0.f;
  stats[1] = 0.f;
  if (increment) *step += 1;
}

__global__ __launch_bounds__(64 * FIN_WAVES) void finalize_k(FinArgs f) {
  __shared__ float wsum[FIN_MAXW];
  finalize_body<false>(f, wsum);
}

__global__ void cast_pad_k(const float* __restrict__ src, bf16_t* __restrict__ dst, int G, int I, int J, int Ip,
                           int Jp) {
  const int64_t total = (int64_t)G * Ip * Jp;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int jj = (int)(t % Jp);
    const int64_t r = t / Jp;
    const int ii = (int)(r % Ip);
    const int gg = (int)(r / Ip);
    float v = 0.f;
    if (ii < I && jj < J) v = src[((int64_t)gg * I + ii) * J + jj];
    dst[t] = f2bf(v);
  }
}

}  // namespace

// optimizer blocks (chunks of OPT_CHUNK elements) of a segment of n elements
static int opt_chunks(int64_t n) { return (int)((n + OPT_CHUNK - 1) / OPT_CHUNK); }

int fused_optimizer_blocks(const OptSeg* segs, int nseg) {
  int nb = 0;
  for (int i = 0; i < nseg; ++i) nb += opt_chunks(segs[i].n);
  return nb;
}

static int g_opt_fin_fused = -1;
void set_opt_fin_fused(int on) { g_opt_fin_fused = on; }
int opt_fin_fused_enabled() {
  if (g_opt_fin_fused < 0) {
    const char* e = getenv("MNISTX_OPT_FIN_FUSED");
    g_opt_fin_fused = (e && *e) ? atoi(e) != 0 : 1;
  }
  return g_opt_fin_fused;
}

hipError_t finalize_step(const FinArgs& f, hipStream_t st) {
  if (f.nw > FIN_MAXW) return hipErrorInvalidValue;
  FinArgs a = f;
  a.ticket = nullptr;
  hipLaunchKernelGGL(finalize_k, dim3(1), dim3(64 * FIN_WAVES), 0, st, a);
  return hipGetLastError();
}

// the block -> segment table of the optimizer launches; returns the number of optimizer blocks
// (chunks), or -1 for segments the kernels' 32-bit index math cannot hold
static int build_seg_table(const OptSeg* segs, int nseg, int l2n, SegTable& tab) {
  int nb = 0;
  for (int i = 0; i < nseg; ++i) {
    if (segs[i].n >= (1ll << 31) || (int64_t)segs[i].I * segs[i].J >= (1ll << 31)) return -1;
    tab.s[i] = segs[i];
    tab.fij[i] = FastDiv((uint32_t)(segs[i].I * segs[i].J));
    tab.fj[i] = FastDiv((uint32_t)segs[i].J);
    tab.blk0[i] = nb;
    nb += opt_chunks(segs[i].n);
  }
  tab.blk0[nseg] = nb;
  tab.n = nseg;
  tab.l2n = l2n;
  return nb;
}

int grad_norm_max_blocks() { return GN_BLOCKS; }

static void launch_grad_sqnorm(const float* params, const float* grads, const SegTable& tab, int nb, float grad_scale,
                               float* gnorm, hipStream_t st) {
  const int per = std::max(1, (nb + GN_BLOCKS - 1) / GN_BLOCKS);
  hipLaunchKernelGGL(grad_sqnorm_k, dim3(GN_BLOCKS), dim3(TPB), 0, st, params, grads, tab, grad_scale, per, gnorm);
}

hipError_t grad_global_norm(const float* params, const float* grads, const OptSeg* segs, int nseg, float grad_scale,
                            float* gnorm, hipStream_t st) {
  if (nseg > MAXSEG || nseg < 1 || !gnorm) return hipErrorInvalidValue;
  SegTable tab;
  const int nb = build_seg_table(segs, nseg, 0, tab);
  if (nb < 0) return hipErrorInvalidValue;
  launch_grad_sqnorm(params, grads, tab, nb, grad_scale, gnorm, st);
  hipLaunchKernelGGL(gnorm_finish_k, dim3(1), dim3(TPB), 0, st, gnorm);
  return hipGetLastError();
}

int var_norm_buffer_size(int nseg) { return nseg * (3 + 2 * GN_BLOCKS); }

// The ratio hand-off.  Measured (bench/micro_opt.py --handoff): on LeNet-5 (62 K parameters, 125
// chunks) the apply blocks summing their variable's few partials themselves saves the third
// launch, 10.8 against 14.0 us (lars); on the reference CNN (3.46 M, 6.8 K chunks) every one of
// 6.8 K blocks summing up to 450 pairs costs more than the one-block-per-variable launch, 36.5
// against 34.1 us.  So: self-sum up to LW_SELF_MAX_CHUNKS chunks, the launch above.
constexpr int LW_SELF_MAX_CHUNKS = 1024;
static int g_lw_self_sum = -2;   // -2: not read yet; -1: by size; 0 / 1: forced
void set_layerwise_self_sum(int mode) { g_lw_self_sum = mode < 0 ? -1 : (mode != 0); }
int layerwise_self_sum_mode() {
  if (g_lw_self_sum == -2) {
    const char* e = getenv("MNISTX_LAYERWISE_SELF_SUM");
    g_lw_self_sum = (e && *e) ? (atoi(e) != 0) : -1;
  }
  return g_lw_self_sum;
}

// var_sqnorm_k over the optimizer's chunk table; returns the chunks per block the readers need
static int launch_var_sqnorm(const float* params, const float* grads, const float* mom, const float* slot2,
                             const SegTable& tab, int nb, const int64_t* step, const OptParams& op, float* tnorm,
                             hipStream_t st) {
  const int per = std::max(1, (nb + GN_BLOCKS - 1) / GN_BLOCKS);
  if (op.rule == OPT_LAMB)
    hipLaunchKernelGGL(var_sqnorm_k<true>, dim3(GN_BLOCKS), dim3(TPB), 0, st, params, grads, mom, slot2, tab, step,
                       op, per, tnorm);
  else
    hipLaunchKernelGGL(var_sqnorm_k<false>, dim3(GN_BLOCKS), dim3(TPB), 0, st, params, grads, mom, slot2, tab, step,
                       op, per, tnorm);
  return per;
}

hipError_t var_norms(const float* params, const float* grads, const float* mom, const float* slot2,
                     const OptSeg* segs, int nseg, const int64_t* step, OptParams op, float lars_eta, float* tnorm,
                     hipStream_t st) {
  if (nseg > MAXSEG || nseg < 1 || !tnorm) return hipErrorInvalidValue;
  if (op.rule != OPT_LARS && op.rule != OPT_LAMB) return hipErrorInvalidValue;
  if (op.rule == OPT_LAMB && (!mom || !slot2 || !step)) return hipErrorInvalidValue;
  SegTable tab;
  const int nb = build_seg_table(segs, nseg, 0, tab);
  if (nb < 0) return hipErrorInvalidValue;
  const int per = launch_var_sqnorm(params, grads, mom, slot2, tab, nb, step, op, tnorm, st);
  hipLaunchKernelGGL(var_ratio_k, dim3(nseg), dim3(TPB), 0, st, tab, (int)(op.rule == OPT_LAMB), lars_eta, op.eps, per,
                     tnorm);
  return hipGetLastError();
}

// what showing (lr_at_steps) and applying (fused_optimizer) a schedule both require of it
static bool lr_sched_valid(const LrSched& s) {
  if (s.kind < LR_STAIRCASE || s.kind > LR_COSINE || s.warmup < 0) return false;
  return s.kind == LR_STAIRCASE || s.total > s.warmup;
}

// f(std::integral_constant<int, RULE>{}) for the run-time rule (validated by the caller)
template <class F>
static void with_rule(int rule, F f) {
  switch (rule) {
    case OPT_ADAM: f(std::integral_constant<int, OPT_ADAM>{}); break;
    case OPT_RMSPROP: f(std::integral_constant<int, OPT_RMSPROP>{}); break;
    case OPT_ADAGRAD: f(std::integral_constant<int, OPT_ADAGRAD>{}); break;
    case OPT_LARS: f(std::integral_constant<int, OPT_LARS>{}); break;
    case OPT_LAMB: f(std::integral_constant<int, OPT_LAMB>{}); break;
    default: f(std::integral_constant<int, OPT_CLASSIC>{});
  }
}

hipError_t fused_optimizer(float* params, const float* grads, float* mom, float* ema, bf16_t* bf, const OptSeg* segs,
                           int nseg, const int64_t* step, OptParams op, float* l2, int l2n, hipStream_t st,
                           const FinArgs* fin, const PermJob* perm, float* slot2, float clip_norm,
                           float* gnorm, float lars_eta, float* tnorm, const LrSched* sched) {
  if (nseg > MAXSEG || nseg < 1) return hipErrorInvalidValue;
  // the plain staircase keeps its kernels; anything else goes to the *_sched_k variants
  const bool sch = sched && !lr_sched_is_default(*sched);
  LrSched sc{};
  if (sch) {
    sc = *sched;
    if (!lr_sched_valid(sc)) return hipErrorInvalidValue;
    // applying a schedule asks more than showing it (lr_at_steps): no PS guard, lr_end >= 0, power > 0
    if (op.guard || !(sc.lr_end >= 0.f) || !(sc.power > 0.f)) return hipErrorInvalidValue;
  }
  if (op.rule < OPT_CLASSIC || op.rule > OPT_LAMB) return hipErrorInvalidValue;
  const bool lw = op.rule == OPT_LARS || op.rule == OPT_LAMB;
  if (op.rule != OPT_CLASSIC && (!mom || (op.rule != OPT_ADAGRAD && op.rule != OPT_LARS && !slot2)))
    return hipErrorInvalidValue;
  if (fin && fin->nw > FIN_MAXW) return hipErrorInvalidValue;
  const bool clip = clip_norm > 0.f;
  if (clip && (!gnorm || op.guard)) return hipErrorInvalidValue;   // a PS push is never clipped
  // the layer-wise rules: never a PS push, never clipped; LARS runs the classic momentum text
  if (lw && (!tnorm || op.guard || clip || !(lars_eta > 0.f))) return hipErrorInvalidValue;
  if (op.rule == OPT_LARS && (!op.use_momentum || op.nesterov)) return hipErrorInvalidValue;
  SegTable tab;
  const int nb = build_seg_table(segs, nseg, l2n, tab);
  if (nb < 0) return hipErrorInvalidValue;
  FinArgs fa{};
  int* tickets = nullptr;
  if (fin && !op.guard && nb <= 1024 && opt_fin_fused_enabled()) tickets = red_tickets(st, true);
  if (tickets) {
    fa = *fin;
    fa.ticket = tickets + OPT_TICKET_SLOT;   // after the reduce's (ticket.h)
  }
  PermJob pj{};
  int npb = 0;
  if (perm && perm->n > 0) {
    pj = *perm;
    pj.blk0 = nb;
    npb = (pj.n + TPB - 1) / TPB;
  }
  const dim3 grid(nb + npb);
  // the norm passes of the layer-wise rules and of clipping come first on st
  int per = 0;
  bool self = false;
  if (lw) {
    per = launch_var_sqnorm(params, grads, mom, slot2, tab, nb, step, op, tnorm, st);
    const int mode = layerwise_self_sum_mode();
    self = mode < 0 ? nb <= LW_SELF_MAX_CHUNKS : mode != 0;
    if (!self)
      hipLaunchKernelGGL(var_ratio_k, dim3(nseg), dim3(TPB), 0, st, tab, (int)(op.rule == OPT_LAMB), lars_eta, op.eps,
                         per, tnorm);
  } else if (clip) {
    launch_grad_sqnorm(params, grads, tab, nb, op.grad_scale, gnorm, st);
  }
  // every kernel but the two classic ones (no slot2) takes these arguments, then its family's own
  auto launch = [&](auto kern, auto... extra) {
    hipLaunchKernelGGL(kern, grid, dim3(TPB), 0, st, params, grads, mom, slot2, ema, bf, tab, step, op, l2, fa, pj,
                       extra...);
  };
  with_rule(op.rule, [&](auto rule) {
    constexpr int R = decltype(rule)::value;
    if constexpr (R == OPT_LARS || R == OPT_LAMB) {   // validated above: never clipped
      auto layerwise = [&](auto self_sum) {
        constexpr bool SELF = decltype(self_sum)::value;
        if (sch) launch(layerwise_opt_sched_k<R, SELF>, tnorm, lars_eta, per, sc);
        else launch(layerwise_opt_k<R, SELF>, tnorm, lars_eta, per);
      };
      if (self) layerwise(std::true_type{});
      else layerwise(std::false_type{});
    } else if (clip) {
      if (sch) launch(clipped_opt_sched_k<R>, gnorm, clip_norm, sc);
      else launch(clipped_opt_k<R>, gnorm, clip_norm);
    } else if constexpr (R == OPT_CLASSIC) {
      if (sch)
        hipLaunchKernelGGL(fused_opt_sched_k, grid, dim3(TPB), 0, st, params, grads, mom, ema, bf, tab, step, op, l2, fa,
                           pj, sc);
      else
        hipLaunchKernelGGL(fused_opt_k, grid, dim3(TPB), 0, st, params, grads, mom, ema, bf, tab, step, op, l2, fa, pj);
    } else {
      if (sch) launch(adaptive_opt_sched_k<R>, sc);
      else launch(adaptive_opt_k<R>);
    }
  });
  if (fin && !tickets) return finalize_step(*fin, st);
  return hipGetLastError();
}

hipError_t lr_at_steps(const int64_t* steps, float* out, int64_t n, float lr0, float decay_rate, int64_t decay_steps,
                       LrSched sched, hipStream_t st) {
  if (n < 0 || !lr_sched_valid(sched)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(lr_at_steps_k, dim3(nblocks(n, TPB, 1024)), dim3(TPB), 0, st, steps, out, n, lr0, decay_rate,
                     decay_steps, sched);
  return hipGetLastError();
}

hipError_t cast_f32_bf16_padded(const float* src, bf16_t* dst, int G, int I, int J, int Ip, int Jp, hipStream_t st) {
  const int64_t total = (int64_t)G * Ip * Jp;
  hipLaunchKernelGGL(cast_pad_k, dim3(nblocks(total, TPB, 8192)), dim3(TPB), 0, st, src, dst, G, I, J, Ip, Jp);
  return hipGetLastError();
}

}  // namespace mnistx
