// Stand-alone softmax cross-entropy (K8): loss, top-1 count, NaN flag and dlogits in one pass.
// The label targets and the statistics hand-off are ce_stats.h, shared with the fused heads.
#include "common.h"
#include "ce_stats.h"
#include "launchers.h"
#include "tpb.h"

#include <algorithm>

namespace mnistx {
namespace {

// ------------------------------------------------------------------ K8 softmax cross-entropy
// stats[0] += sum(-log p[label]) ; stats[1] += #(logit[label] == max) ; stats[2] = 1 if non-finite.
// The label target (plain; SMOOTH: eps; two labels: eps, labels2, lam; DISTILL: a CeDistill) is the trailing pack's
// CeTarget (ce_stats.h).
template <bool SMOOTH = false, typename... EPS>
__global__ void softmax_ce_k(const float* __restrict__ logits, int ldl, const int32_t* __restrict__ labels, int B,
                             int NC, float scale, bf16_t* __restrict__ dl, int ldd, float* __restrict__ stats,
                             float* __restrict__ probs, EPS... eps) {
  using TG = CeTarget<EPS...>;
  static_assert(SMOOTH == TG::SMOOTH && !TG::DROP, "the smoothed instantiation takes eps, the mixed one eps, labels2 and lam");
  const TG tg(NC, eps...);
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  float loss = 0.f, corr = 0.f;
  int bad = 0;
  if (row < B) {
    const float* l = logits + (int64_t)row * ldl;
    float mx = -INFINITY;
    for (int c = 0; c < NC; ++c) mx = fmaxf(mx, l[c]);
    float se = 0.f;
    for (int c = 0; c < NC; ++c) se += __expf(l[c] - mx);
    const float inv = 1.f / se;
    const int lab = labels ? labels[row] : -1;
    typename TG::Row tr = tg.row(lab, row);
    if constexpr (TG::DISTILL) {   // the scalars of the row's soft part (ce_stats.h)
      typename TG::Row& sf = tr;
      const float* tp = tg.trow(row);
      const float iT = tg.dist->iT;
      sf.tm = -INFINITY;
      for (int c = 0; c < NC; ++c) sf.tm = fmaxf(sf.tm, tp[c]);
      float st = 0.f, seT = 0.f;
      for (int c = 0; c < NC; ++c) {
        st += __expf((tp[c] - sf.tm) * iT);
        seT += __expf((l[c] - mx) * iT);
      }
      sf.ist = 1.f / st;
      sf.iseT = 1.f / seT;
      const float lst = __logf(st), lseT = __logf(seT);
      sf.soft = 0.f;
      for (int c = 0; c < NC; ++c) {
        const float v = (tp[c] - sf.tm) * iT;
        sf.soft += __expf(v) * sf.ist * ((v - lst) - ((l[c] - mx) * iT - lseT));
      }
    }
    if (labels) {
      const float ll = l[lab];
      if constexpr (TG::NEEDS_DB) tr.db = l[tr.yb] - mx;
      if constexpr (TG::NEEDS_SD)
        for (int c = 0; c < NC; ++c) tr.sd += l[c] - mx;
      loss = tg.loss(tr, ll - mx, __logf(se));
      corr = (ll >= mx) ? 1.f : 0.f;
      if (!isfinite(loss)) bad = 1;
    }
    if (dl) {
      bf16_t* d = dl + (int64_t)row * ldd;
      for (int c = 0; c < ldd; ++c) {
        float g = 0.f;
        if constexpr (TG::DISTILL) {
          if (c < NC) {
            const float* tp = tg.trow(row);
            const float ps = __expf((l[c] - mx) * tg.dist->iT) * tr.iseT - __expf((tp[c] - tr.tm) * tg.dist->iT) * tr.ist;
            g = tg.dgrad(__expf(l[c] - mx) * inv - tg.q(tr, c), ps) * scale;
          }
        } else
        if (c < NC) g = (__expf(l[c] - mx) * inv - tg.q(tr, c)) * scale;
        d[c] = f2bf(g);
      }
    }
    if (probs)
      for (int c = 0; c < NC; ++c) probs[(int64_t)row * NC + c] = __expf(l[c] - mx) * inv;
  }
  if (stats) {
    loss = warp_sum(loss);
    corr = warp_sum(corr);
    bad = warp_sum_i(bad);
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&stats[0], loss);
      atomicAdd(&stats[1], corr);
      if (bad) stats[2] = 1.f;
    }
  }
}

// Row-vectorized variant for padded logit rows of LD = 16 / 32 floats (the
// classifier output is padded to >= 16 columns): one thread per row, f32x4 loads,
// 16-byte bf16 stores.  Statistics: warp + block reduction, then either one
// atomic per block or -- with a workspace -- per-block partials combined by the
// last block to finish (ticket counter) in block order: bitwise deterministic.
template <int LD, bool SMOOTH = false, typename... EPS>
__global__ __launch_bounds__(256) void softmax_ce_rows_k(const float* __restrict__ logits,
                                                         const int32_t* __restrict__ labels, int B, int NC,
                                                         float scale, bf16_t* __restrict__ dl,
                                                         float* __restrict__ stats, float* __restrict__ probs,
                                                         float* __restrict__ work, int defer_stats,
                                                         float* __restrict__ dbias, EPS... eps) {
  using TG = CeTarget<EPS...>;
  static_assert(SMOOTH == TG::SMOOTH && !TG::DROP, "the smoothed instantiation takes eps, the mixed one eps, labels2 and lam");
  const TG tg(NC, eps...);
  float loss = 0.f, corr = 0.f, bad = 0.f;
  float cs[LD];   // fp32 column sums of dlogits (dbias: the last layer's bias gradient partial)
#pragma unroll
  for (int c = 0; c < LD; ++c) cs[c] = 0.f;
  for (int row = blockIdx.x * 256 + threadIdx.x; row < B; row += gridDim.x * 256) {
    float l[LD];
#pragma unroll
    for (int v = 0; v < LD / 4; ++v) {
      const f32x4 t = *(const f32x4*)(logits + (int64_t)row * LD + 4 * v);
      l[4 * v] = t[0];
      l[4 * v + 1] = t[1];
      l[4 * v + 2] = t[2];
      l[4 * v + 3] = t[3];
    }
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < LD; ++c)
      if (c < NC) mx = fmaxf(mx, l[c]);
    float e[LD], se = 0.f;
#pragma unroll
    for (int c = 0; c < LD; ++c) {
      e[c] = c < NC ? __expf(l[c] - mx) : 0.f;
      se += e[c];
    }
    const float inv = 1.f / se;
    const int lab = labels ? labels[row] : -1;
    typename TG::Row tr = tg.row(lab, row);
    // DISTILL: the teacher's row, loaded once (a clamped column: the columns >= NC are never read)
    if constexpr (TG::DISTILL) {
      typename TG::Row& sf = tr;
      const float* tp = tg.trow(row);
      const float iT = tg.dist->iT;
      float tv[LD], tm = -INFINITY;
#pragma unroll
      for (int c = 0; c < LD; ++c) tv[c] = tp[min(c, NC - 1)];
#pragma unroll
      for (int c = 0; c < LD; ++c)
        if (c < NC) tm = fmaxf(tm, tv[c]);
      float ev[LD], eu[LD], st = 0.f, seT = 0.f;
#pragma unroll
      for (int c = 0; c < LD; ++c) {
        tv[c] = (tv[c] - tm) * iT;                           // v_c
        ev[c] = c < NC ? __expf(tv[c]) : 0.f;
        eu[c] = c < NC ? __expf((l[c] - mx) * iT) : 0.f;     // exp(u_c)
        st += ev[c];
        seT += eu[c];
      }
      const float ist = 1.f / st, iseT = 1.f / seT, lst = __logf(st), lseT = __logf(seT);
      sf.soft = 0.f;
#pragma unroll
      for (int c = 0; c < LD; ++c) {
        const float qc = ev[c] * ist;
        sf.ps[c] = eu[c] * iseT - qc;
        if (c < NC) sf.soft += qc * ((tv[c] - lst) - ((l[c] - mx) * iT - lseT));
      }
    }
    if (labels) {
      float ll = 0.f;
#pragma unroll
      for (int c = 0; c < LD; ++c) ll = (c == lab) ? l[c] : ll;
      if constexpr (TG::NEEDS_DB) {
        float lb = 0.f;
#pragma unroll
        for (int c = 0; c < LD; ++c) lb = (c == tr.yb) ? l[c] : lb;
        tr.db = lb - mx;
      }
      if constexpr (TG::NEEDS_SD) {
#pragma unroll
        for (int c = 0; c < LD; ++c)
          if (c < NC) tr.sd += l[c] - mx;
      }
      const float lo = tg.loss(tr, ll - mx, __logf(se));
      loss += lo;
      corr += (ll >= mx) ? 1.f : 0.f;
      if (!isfinite(lo)) bad = 1.f;
    }
    if (dl) {
#pragma unroll
      for (int v = 0; v < LD / 8; ++v) {
        u32x4 o;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const int c0 = 8 * v + 2 * h;
          float g0 = c0 < NC ? (e[c0] * inv - tg.q(tr, c0)) * scale : 0.f;
          float g1 = c0 + 1 < NC ? (e[c0 + 1] * inv - tg.q(tr, c0 + 1)) * scale : 0.f;
          if constexpr (TG::DISTILL) {
            g0 = c0 < NC ? tg.dgrad(e[c0] * inv - tg.q(tr, c0), tr.ps[c0]) * scale : 0.f;
            g1 = c0 + 1 < NC ? tg.dgrad(e[c0 + 1] * inv - tg.q(tr, c0 + 1), tr.ps[c0 + 1]) * scale : 0.f;
          }
          o[h] = pack2(g0, g1);
          cs[c0] += g0;
          cs[c0 + 1] += g1;
        }
        *(u32x4*)(dl + (int64_t)row * LD + 8 * v) = o;
      }
    }
    if (probs)
#pragma unroll
      for (int c = 0; c < LD; ++c)
        if (c < NC) probs[(int64_t)row * NC + c] = e[c] * inv;
  }
  if (dl && dbias) block_colsum<4, LD>(cs, dbias + (int64_t)blockIdx.x * LD);
  if (stats) ce_block_stats<4>(loss, corr, bad, stats, work, defer_stats != 0);
}

}  // namespace

int softmax_ce_dbias_blocks(int B, int ldl) {
  return (ldl == 16 || ldl == 32) && B > 0 ? (int)std::min<int64_t>(CE_MAXB, ((int64_t)B + 255) / 256) : 0;
}

hipError_t softmax_ce(const float* logits, int ldl, const int32_t* labels, int B, int NC, float scale,
                      bf16_t* dlogits, int ldd, float* stats, float* probs, float* work, hipStream_t st,
                      int* defer_blocks, float* dbias, float label_smoothing, const int32_t* labels2,
                      const float* lam, const CeDistill* distill) {
  const int nb = (int)std::min<int64_t>(CE_MAXB, ((int64_t)B + 255) / 256);
  const bool mix = labels2 != nullptr;   // the mixed instantiations: eps (0 allowed), labels2, lam
  if (mix != (lam != nullptr) || (mix && !labels)) return hipErrorInvalidValue;
  const bool smooth = label_smoothing != 0.f;   // the smoothed instantiations, eps as their last argument
  if (smooth && !labels) return hipErrorInvalidValue;
  // the distilled instantiations: a CeDistill alone in the pack
  if (distill && (mix || smooth || !labels || !distill->t || NC < 1 || distill->ldt < NC)) return hipErrorInvalidValue;
  if (defer_blocks) *defer_blocks = 0;
  const bool rows_ok = (ldl == 16 || ldl == 32) && NC <= ldl && (!dlogits || ldd == ldl) &&
                       ((uintptr_t)logits % 16 == 0) && (!dlogits || (uintptr_t)dlogits % 16 == 0);
  if (rows_ok && B > 0) {
    const int defer = (defer_blocks && work && stats) ? 1 : 0;
    if (defer) *defer_blocks = nb;
    if (distill && ldl == 16)
      hipLaunchKernelGGL((softmax_ce_rows_k<16, false, CeDistill>), dim3(nb), dim3(256), 0, st, logits, labels, B, NC,
                         scale, dlogits, stats, probs, work, defer, dbias, *distill);
    else if (distill)
      hipLaunchKernelGGL((softmax_ce_rows_k<32, false, CeDistill>), dim3(nb), dim3(256), 0, st, logits, labels, B, NC,
                         scale, dlogits, stats, probs, work, defer, dbias, *distill);
    else if (mix && ldl == 16)
      hipLaunchKernelGGL((softmax_ce_rows_k<16, true, float, const int32_t*, const float*>), dim3(nb), dim3(256), 0, st,
                         logits, labels, B, NC, scale, dlogits, stats, probs, work, defer, dbias, label_smoothing,
                         labels2, lam);
    else if (mix)
      hipLaunchKernelGGL((softmax_ce_rows_k<32, true, float, const int32_t*, const float*>), dim3(nb), dim3(256), 0, st,
                         logits, labels, B, NC, scale, dlogits, stats, probs, work, defer, dbias, label_smoothing,
                         labels2, lam);
    else if (smooth && ldl == 16)
      hipLaunchKernelGGL((softmax_ce_rows_k<16, true, float>), dim3(nb), dim3(256), 0, st, logits, labels, B, NC, scale,
                         dlogits, stats, probs, work, defer, dbias, label_smoothing);
    else if (smooth)
      hipLaunchKernelGGL((softmax_ce_rows_k<32, true, float>), dim3(nb), dim3(256), 0, st, logits, labels, B, NC, scale,
                         dlogits, stats, probs, work, defer, dbias, label_smoothing);
    else if (ldl == 16)
      hipLaunchKernelGGL(softmax_ce_rows_k<16>, dim3(nb), dim3(256), 0, st, logits, labels, B, NC, scale, dlogits,
                         stats, probs, work, defer, dbias);
    else
      hipLaunchKernelGGL(softmax_ce_rows_k<32>, dim3(nb), dim3(256), 0, st, logits, labels, B, NC, scale, dlogits,
                         stats, probs, work, defer, dbias);
    return hipGetLastError();
  }
  if (dbias) return hipErrorInvalidValue;   // the row kernel's block partials only
  if (distill)
    hipLaunchKernelGGL((softmax_ce_k<false, CeDistill>), dim3((B + TPB - 1) / TPB), dim3(TPB), 0, st, logits, ldl, labels,
                       B, NC, scale, dlogits, ldd, stats, probs, *distill);
  else if (mix)
    hipLaunchKernelGGL((softmax_ce_k<true, float, const int32_t*, const float*>), dim3((B + TPB - 1) / TPB), dim3(TPB), 0,
                       st, logits, ldl, labels, B, NC, scale, dlogits, ldd, stats, probs, label_smoothing, labels2, lam);
  else if (smooth)
    hipLaunchKernelGGL((softmax_ce_k<true, float>), dim3((B + TPB - 1) / TPB), dim3(TPB), 0, st, logits, ldl, labels, B,
                       NC, scale, dlogits, ldd, stats, probs, label_smoothing);
  else
    hipLaunchKernelGGL(softmax_ce_k<>, dim3((B + TPB - 1) / TPB), dim3(TPB), 0, st, logits, ldl, labels, B, NC, scale,
                       dlogits, ldd, stats, probs);
  return hipGetLastError();
}

}  // namespace mnistx
