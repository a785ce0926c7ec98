// Deterministic per-step cross-entropy statistics (loss sum, correct count, NaN
// flag) shared by the softmax-CE kernel (softmax_ce.hip) and the fused dense head
// (mlp_head.hip).  Each block reduces its threads in a fixed tree, writes one
// partial to `work`, and the last block to finish (ticket counter at
// work[4 * CE_MAXB]) combines the partials in block order: bitwise identical
// results across runs and between hipGraph replay and eager execution.
#pragma once
#include "common.h"
#include "launchers.h"

#include <type_traits>

using mnistx::CE_MAXB;   // max blocks per launch (work holds 4 floats per block + ticket)

// The label target of the softmax-CE kernels, one view of their trailing argument pack.  The pack is
// [eps] [labels2, lam] [HeadDrop], or a CeDistill alone; what it holds is read off its types, so the
// plain instantiation has no trailing argument and keeps the arguments and the code it always had.
//   SMOOTH (eps): label smoothing.  With on = 1 - eps and off = eps / NC (NC = the real class count):
//     loss = log(se) - on * (l_y - mx) - off * sum_{c < NC} (l_c - mx)
//     dl_c = (p_c - on * [c == y] - off) * scale
//   The class sum is over the differences, which stay finite for |l_c - mx| <= 1e37.
//   MIX (eps, which may be 0, then labels2 and lam): two labels per row (mixup / CutMix, mix.hip).  With
//   ya = labels[m], yb = labels2[m], lam = lam[m] and om = 1 - lam:
//     loss = log(se) - on * (lam (l_ya - mx) + om (l_yb - mx)) - off * sum_{c < NC} (l_c - mx)
//     dl_c = (p_c - on * (lam [c == ya] + om [c == yb]) - off) * scale
//   A row with lam == 1 drops the yb term by a select, never by a product with 0: an infinite l_yb leaves
//   such a row finite.  eps = 0 (off == 0) leaves the class sum out by a select too: a -inf logit in a
//   class no label names makes it -inf, and 0 * inf is NaN.  lam + om is exactly 1 for lam in [0.5, 1],
//   so ya == yb gives `on` at that class.  The top-1 count stays l_ya >= mx: ya is the dominant label.
//   DROP (a HeadDrop closes the pack; mlp_head_k alone): dropout on the hidden layers (dropout_rng.h).
//   DISTILL (a CeDistill, launchers.h, alone in the pack): the dense soft target of a frozen teacher at a
//   temperature (Hinton-style knowledge distillation).  With t_c the teacher's logits of the row, a = alpha,
//   iT = 1 / T and d_c = l_c - mx:
//     u_c = d_c * iT               seT = sum exp(u_c)   pT_c = exp(u_c) / seT
//     v_c = (t_c - max_c t_c) * iT st  = sum exp(v_c)   q_c  = exp(v_c) / st
//     soft = sum_c q_c * ((v_c - log st) - (u_c - log seT))          KL(q || pT), formed per class
//     loss = (1 - a) * hard + a * T^2 * soft,   hard = log(se) - d_y (the plain row loss)
//     dl_c = ((1 - a) * (p_c - [c == y]) + a * T * (pT_c - q_c)) * scale
//   The KL is summed per class, never as a difference of two sums: equal student and teacher rows give
//   soft == 0 and a zero soft gradient without cancellation.  q_c == 0 (underflow) contributes 0 while
//   the other factor is finite; a non-finite teacher or student logit makes the row's loss non-finite
//   (the NaN flag).  The kernel loads the teacher's row once (trow) and fills in the Row: soft, and
//   ps[i] = pT_c - q_c of the classes the thread holds, in the kernel's own class layout; dgrad() joins
//   the two gradients.
// A kernel builds one CeTarget from (NC, eps...) and one Row per batch row (the second label and the
// weight are loaded there, once), fills in what the row's loss reads beside da = l_ya - mx and lse =
// log(se) -- db = l_yb - mx where the Row has it, the class sum sd likewise -- and asks for the row's
// loss and for the target q of a class.  The plain Row is the label alone: a plain kernel declares
// nothing it does not use (a dead declaration is enough to change its register allocation).
struct CeRow { int ya; };
struct CeRowSmooth { int ya; float sd; };
struct CeRowMix { int ya, yb; float lam, om, db, sd; };
// DISTILL: soft = KL(q || pT) and ps[i] = pT_c - q_c of the (at most 32) classes a thread holds; the members
// a kernel does not touch cost nothing (every index is a constant after unrolling).  The generic
// kernels (a run-time class count, no per-class registers) keep the row's scalars instead -- tm = max_c
// t_c, ist = 1 / st, iseT = 1 / seT -- and form v_c and u_c again where they need them, as they form
// l_c - mx again.
struct CeRowDistill { int ya; float soft, tm, ist, iseT; float ps[32]; };

template <typename... P>
struct CeTarget {
  static constexpr bool SMOOTH = (std::is_same_v<P, float> || ...);
  static constexpr bool MIX = (std::is_same_v<P, const float*> || ...);
  static constexpr bool DROP = (std::is_same_v<P, mnistx::HeadDrop> || ...);
  static constexpr bool DISTILL = (std::is_same_v<P, mnistx::CeDistill> || ...);
  static_assert(sizeof...(P) == (SMOOTH ? 1 : 0) + (MIX ? 2 : 0) + (DROP ? 1 : 0) + (DISTILL ? 1 : 0) &&
                    (SMOOTH || !MIX) && (!DISTILL || sizeof...(P) == 1),
                "the pack is [eps] [labels2, lam] [HeadDrop], or a CeDistill alone; labels2 and lam come with eps");
  static constexpr bool NEEDS_DB = MIX, NEEDS_SD = SMOOTH;   // the Row has db / sd for the kernel to fill in
  using Row = std::conditional_t<MIX, CeRowMix,
                                 std::conditional_t<SMOOTH, CeRowSmooth, std::conditional_t<DISTILL, CeRowDistill, CeRow>>>;

  float on = 1.f, off = 0.f;
  const int32_t* labels2 = nullptr;
  const float* lam = nullptr;
  const mnistx::HeadDrop* drop = nullptr;
  const mnistx::CeDistill* dist = nullptr;

  DEV CeTarget(int nc, const P&... p) { (take(nc, p), ...); }

  // The target of row m with first label ya.  The fused heads pass min(m, nb - 1), as their X loads do
  // (a row past the batch is never stored or counted), so the two loads sit under no branch.
  DEV Row row(int ya, int64_t m) const {
    if constexpr (MIX) {
      const float lm = lam[m];
      return Row{ya, labels2[m], lm, lm < 1.f ? 1.f - lm : 0.f, 0.f, 0.f};
    } else if constexpr (SMOOTH) {
      return Row{ya, 0.f};
    } else if constexpr (DISTILL) {
      Row r;
      r.ya = ya;
      return r;
    } else {
      return Row{ya};
    }
  }
  DEV float loss(const Row& r, float da, float lse) const {
    if constexpr (MIX) {
      const float tl = r.lam < 1.f ? fmaf(r.lam, da, (1.f - r.lam) * r.db) : da;
      const float a = fmaf(-on, tl, lse);
      return off != 0.f ? fmaf(-off, r.sd, a) : a;
    } else if constexpr (SMOOTH) {
      return fmaf(-off, r.sd, fmaf(-on, da, lse));
    } else if constexpr (DISTILL) {   // (1 - a) * hard + a * T^2 * soft
      return fmaf(dist->alpha * dist->T * dist->T, r.soft, (1.f - dist->alpha) * -(da - lse));
    } else {
      return -(da - lse);
    }
  }
  DEV float q(const Row& r, int c) const {
    if constexpr (MIX) return fmaf(on, (c == r.ya ? r.lam : 0.f) + (c == r.yb ? r.om : 0.f), off);
    else if constexpr (SMOOTH) return c == r.ya ? on + off : off;
    else return c == r.ya ? 1.f : 0.f;
  }
  // DISTILL (q() is the one-hot there): the teacher's logits of row m (the fused heads pass min(m, nb - 1),
  // as for row()),
  DEV const float* trow(int64_t m) const { return dist->t + m * dist->ldt; }
  // and a class's gradient from ph = p_c - [c == y] and ps = pT_c - q_c
  DEV float dgrad(float ph, float ps) const { return fmaf(dist->alpha * dist->T, ps, (1.f - dist->alpha) * ph); }

 private:
  DEV void take(int nc, float eps) {
    off = eps / (float)nc;
    on = 1.f - eps;
  }
  DEV void take(int, const int32_t* l2) { labels2 = l2; }
  DEV void take(int, const float* lm) { lam = lm; }
  DEV void take(int, const mnistx::HeadDrop& d) { drop = &d; }
  DEV void take(int, const mnistx::CeDistill& d) { dist = &d; }
};

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
