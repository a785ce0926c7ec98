// The body of fused_opt_k, adaptive_opt_k<RULE>, clipped_opt_k<RULE> and layerwise_opt_k<RULE, SELF>
// (optimizer.hip), included inside each kernel so that each compiles it as its own code (a function
// template in its place changes all 24 instances: contraction, the guard's load), with perm.h and
// ticket.h included before it and the kernel's parameters in scope:
//   params, grads, mom, slot2, ema, bf, tab, step_p, op, l2, fin, pj, gnorm, clip_norm, tnorm,
//   lars_eta, lw_per, sc, and `constexpr int RULE`, `constexpr bool CLIP`, `constexpr bool LW_SELF`,
//   `constexpr bool SCHED`.
// SCHED (the *_sched_k kernels only): the rate comes from sched_lr -- warmup, polynomial or cosine
// decay (LrSched sc) -- in place of the staircase line; everything after `lr` is the same text.
// Without SCHED the staircase line is compiled alone, as before.
// RULE = OPT_LARS / OPT_LAMB (layerwise_opt_k only): the variable's trust ratio r_k scales the
// update.  tnorm holds var_sqnorm_k's per-(variable, block) partials; with LW_SELF every block
// sums its own variable's partials in the same fixed order (lw_var_sums), so all blocks of a
// variable hold the bitwise-same r_k and its first block records norms and ratio; without, the
// block reads the r_k that var_ratio_k wrote.  LARS then runs the classic momentum text on
// r_k * g_eff (a multiply of its own: r_k = 1 is bit for bit momentum); LAMB recomputes m, v, u
// through lamb_u, the helper the norm pass measured u with.
// CLIP (clipped_opt_k only): clip by global norm.  gnorm[2 ..] holds grad_sqnorm_k's per-block
// partials of sum(g_eff^2); every block sums them itself in the same fixed order (gn_total), so
// all blocks hold the bitwise-same norm and scale s = clip_norm / max(norm, clip_norm) with no
// hand-off between blocks, and the rule sees g_eff * s.  Without CLIP none of it is compiled.
// RULE = OPT_CLASSIC is SGD / momentum / Nesterov, chosen at run time by OptParams; the adaptive
// rules (Adam, RMSProp, Adagrad) are compile-time, so the classic kernel's code does not change
// with them.  slot2: the second slot buffer (Adam v, RMSProp ms), read and written like mom.
// Everything outside the rule -- the perm job's blocks, the PS guard, EMA, bf16 / W^T copies,
// l2 partials, the finalize ticket -- is the same text for every rule.
  constexpr bool ADAPT = RULE != OPT_CLASSIC;
  constexpr bool TWO = RULE == OPT_ADAM || RULE == OPT_RMSPROP || RULE == OPT_LAMB;   // rules with a second slot
  constexpr bool LW = RULE == OPT_LARS || RULE == OPT_LAMB;
  const int use_m = ADAPT ? 1 : op.use_momentum;                   // the first slot is read and written
  __shared__ float red[TPB / 64];
  __shared__ float wsum[FIN_MAXW];
  __shared__ int last;
  const int nopt = pj.n > 0 ? pj.blk0 : (int)gridDim.x;   // optimizer blocks; the rest: the perm job
  if ((int)blockIdx.x >= nopt) {
    perm_one(((int)blockIdx.x - nopt) * TPB + threadIdx.x, pj.out, pj.start, pj.n, pj.N, pj.seed, pj.h, pj.lab_src,
             pj.lab_out);
    return;
  }
  if (op.guard && *op.guard != op.guard_want) {   // a stale / torn PS push: never applied
    if (blockIdx.x == 0 && threadIdx.x == 0) *op.guard_err = op.guard_id;
    return;
  }
  int si = 0;
  while (si + 1 < tab.n && (int)blockIdx.x >= tab.blk0[si + 1]) ++si;
  const OptSeg sg = tab.s[si];
  const int64_t step = *step_p;
  float lr = op.lr0;
  if constexpr (SCHED) {
    lr = sched_lr(op.lr0, op.decay_rate, op.decay_steps, sc, step);   // block-uniform
  } else {
    if (op.decay_steps > 0) lr *= powf(op.decay_rate, (float)(step / op.decay_steps));  // staircase
  }
  float ema_d = 0.f;
  if (op.ema_max >= 0.f) ema_d = fminf(op.ema_max, (1.f + (float)step) / (10.f + (float)step));
  const int64_t lo = (int64_t)(blockIdx.x - tab.blk0[si]) * OPT_CHUNK;
  const int64_t ij = (int64_t)sg.I * sg.J;
  float sq = 0.f;
  // each thread owns a PAIR of consecutive elements (8-byte loads / stores of params, grads,
  // momentum and EMA; one 4-byte bf16 store when the pair stays in one row of the padded
  // copy), all loads issued before any use; the pair falls back to two scalar accesses in a
  // segment at an odd offset.  Out-of-range elements load element 0 and are never stored.
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const int64_t li0 = lo + 2 * (int64_t)threadIdx.x;
  const bool vec = (sg.off & 1) == 0 && li0 + 1 < sg.n;
  float pv[OPT_EPT], gv[OPT_EPT], mv[OPT_EPT], sv[OPT_EPT], ev[OPT_EPT];
  if (vec) {
    const int64_t e = sg.off + li0;
    const f32x2_t p2 = *(const f32x2_t*)(params + e), g2 = *(const f32x2_t*)(grads + e);
    const f32x2_t m2 = use_m ? *(const f32x2_t*)(mom + e) : f32x2_t{0.f, 0.f};
    f32x2_t s2 = {0.f, 0.f};
    if constexpr (TWO) s2 = *(const f32x2_t*)(slot2 + e);
    const f32x2_t e2 = op.ema_max >= 0.f ? *(const f32x2_t*)(ema + e) : f32x2_t{0.f, 0.f};
#pragma unroll
    for (int u = 0; u < OPT_EPT; ++u) {
      pv[u] = p2[u];
      gv[u] = g2[u];
      mv[u] = m2[u];
      sv[u] = s2[u];
      ev[u] = e2[u];
    }
  } else {
#pragma unroll
    for (int u = 0; u < OPT_EPT; ++u) {
      const int64_t li = li0 + u;
      const int64_t e = sg.off + (li < sg.n ? li : 0);
      pv[u] = params[e];
      gv[u] = grads[e];
      mv[u] = use_m ? mom[e] : 0.f;
      sv[u] = 0.f;
      if constexpr (TWO) sv[u] = slot2[e];
      ev[u] = op.ema_max >= 0.f ? ema[e] : 0.f;
    }
  }
  // Adam's bias corrections, once per block (thread 0, behind the loads already in flight):
  // sqrt(1 - b2^t) / (1 - b1^t) with t = step + 1, as -expm1(t log b) in double -- fp32
  // 1 - powf(0.999, t) is off by 6e-5 at t = 1
  float clip_s = 1.f;
  if constexpr (CLIP) {   // behind the loads already in flight
    __shared__ float gred[TPB / 64];
    const float gn = gn_total(gnorm, gred);
    clip_s = clip_scale(gn, clip_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      gnorm[0] = gn;
      gnorm[1] = clip_s;
    }
  }
  float lw_r = 1.f, lw_ic1 = 1.f, lw_ic2 = 1.f;
  if constexpr (LW) {   // behind the loads already in flight
    if constexpr (LW_SELF) {
      __shared__ float lred[2 * (TPB / 64)];
      const bool first = (int)blockIdx.x == tab.blk0[si];
      if (sg.adapt || first) {   // block-uniform
        float sp, su, pn, un;
        lw_var_sums(lw_parts(tnorm, tab.n, si), tab.blk0[si], tab.blk0[si + 1], lw_per, lred, sp, su);
        lw_r = lw_ratio(RULE == OPT_LAMB, sg.adapt, sp, su, lars_eta, op.eps, pn, un);
        if (first && threadIdx.x == 0) {
          tnorm[3 * si] = pn;
          tnorm[3 * si + 1] = un;
          tnorm[3 * si + 2] = lw_r;
        }
      }
    } else {
      lw_r = tnorm[3 * si + 2];
    }
    if constexpr (RULE == OPT_LAMB) {
      __shared__ float lcorr[2];
      if (threadIdx.x == 0) lamb_corr(step, op, lcorr[0], lcorr[1]);
      __syncthreads();
      lw_ic1 = lcorr[0];
      lw_ic2 = lcorr[1];
    }
  }
  float lr_t = lr;
  if constexpr (RULE == OPT_ADAM) {
    __shared__ float corr;
    if (threadIdx.x == 0) {
      const double t = (double)(step + 1);
      corr = (float)(sqrt(-expm1(t * op.log_b2)) / -expm1(t * op.log_b1));
    }
    __syncthreads();
    lr_t = lr * corr;
  }
  float po[OPT_EPT], mo[OPT_EPT], so[OPT_EPT], eo[OPT_EPT];
#pragma unroll
  for (int u = 0; u < OPT_EPT; ++u) {
    float p = pv[u];
    if (li0 + u < sg.n) sq += p * p;
    float g;
    if constexpr (LW) {
      // g_eff exactly as the norm pass formed it (lw_geff), and as the unclipped kernels contract it
      g = lw_geff(p, gv[u], op.grad_scale, sg.wd);
      if constexpr (RULE == OPT_LARS) g = clip_mul(g, lw_r);
    } else if constexpr (CLIP) {
      // the sum as the unclipped kernels contract it (the gradient's product rounded, the decay's
      // fused), spelled out: left to itself the compiler pairs the two products here and adds
      // them unfused.  Then the scale: s = 1 changes no bit (tests/test_clip_norm_gpu.py).
      g = clip_mul(__builtin_fmaf(sg.wd, p, gv[u] * op.grad_scale), clip_s);
    } else {
      g = gv[u] * op.grad_scale + sg.wd * p;
    }
    so[u] = 0.f;
    if constexpr (RULE == OPT_ADAM) {
      // eps outside the root: m = v = 0 (a gradient that was always zero) gives 0 * 1/eps = 0
      const float m = op.b1 * mv[u] + op.omb1 * g;
      const float v = op.b2 * sv[u] + op.omb2 * (g * g);
      mo[u] = m;
      so[u] = v;
      p -= lr_t * m * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(v) + op.eps);
    } else if constexpr (RULE == OPT_RMSPROP) {
      const float ms = op.b2 * sv[u] + op.omb2 * (g * g);
      const float m = op.momentum * mv[u] + lr * g * __builtin_amdgcn_rsqf(ms + op.eps);
      mo[u] = m;
      so[u] = ms;
      p -= m;
    } else if constexpr (RULE == OPT_ADAGRAD) {
      const float acc = mv[u] + g * g;
      mo[u] = acc;
      p -= lr * g * __builtin_amdgcn_rsqf(acc);
    } else if constexpr (RULE == OPT_LAMB) {
      float m, v;
      const float uu = lamb_u(mv[u], sv[u], g, op, lw_ic1, lw_ic2, m, v);
      mo[u] = m;
      so[u] = v;
      p -= lr * clip_mul(uu, lw_r);
    } else {
      float upd = g;
      mo[u] = 0.f;
      if (op.use_momentum) {
        const float v = mv[u] * op.momentum + g;
        mo[u] = v;
        upd = op.nesterov ? g + op.momentum * v : v;
      }
      p -= lr * upd;
    }
    po[u] = p;
    eo[u] = op.ema_max >= 0.f ? ev[u] - (1.f - ema_d) * (ev[u] - p) : 0.f;
  }
  if (vec) {
    const int64_t e = sg.off + li0;
    *(f32x2_t*)(params + e) = f32x2_t{po[0], po[1]};
    if (use_m) *(f32x2_t*)(mom + e) = f32x2_t{mo[0], mo[1]};
    if constexpr (TWO) *(f32x2_t*)(slot2 + e) = f32x2_t{so[0], so[1]};
    if (op.ema_max >= 0.f) *(f32x2_t*)(ema + e) = f32x2_t{eo[0], eo[1]};
  } else {
#pragma unroll
    for (int u = 0; u < OPT_EPT; ++u) {
      if (li0 + u >= sg.n) continue;
      const int64_t e = sg.off + li0 + u;
      params[e] = po[u];
      if (use_m) mom[e] = mo[u];
      if constexpr (TWO) slot2[e] = so[u];
      if (op.ema_max >= 0.f) ema[e] = eo[u];
    }
  }
  if (sg.bf_off >= 0) {
    // 32-bit magic-number divisions (segments < 2^31 elements): the 64-bit divides here
    // were most of this kernel's time on the 3.2M-element local3 weights
    int64_t bi[OPT_EPT];
    int jj0 = 0, ii0 = 0;
#pragma unroll
    for (int u = 0; u < OPT_EPT; ++u) {
      const int l32 = (int)(li0 + u);
      const int gg = tab.fij[si].div(l32);
      const int rem = l32 - gg * (int)ij;
      const int ii = tab.fj[si].div(rem), jj = rem - ii * sg.J;
      bi[u] = sg.bf_off + ((int64_t)gg * sg.Ip + ii) * sg.Jp + jj;
      if (u == 0) {
        jj0 = jj;
        ii0 = ii;
      }
    }
    const bf16_t b0 = f2bf(po[0]), b1 = f2bf(po[1]);
    if (vec && bi[1] == bi[0] + 1 && (bi[0] & 1) == 0) {
      *(uint32_t*)(bf + bi[0]) = (uint32_t)b0 | ((uint32_t)b1 << 16);
    } else {
      if (li0 < sg.n) bf[bi[0]] = b0;
      if (li0 + 1 < sg.n) bf[bi[1]] = b1;
    }
    if (sg.bft_off >= 0) {   // W^T copy (fused dense head): scattered 2-byte stores
      if (li0 < sg.n) bf[sg.bft_off + (int64_t)jj0 * sg.It + ii0] = b0;
      if (li0 + 1 < sg.n) {
        const int l32 = (int)(li0 + 1);
        const int gg = tab.fij[si].div(l32);
        const int rem = l32 - gg * (int)ij;
        const int ii = tab.fj[si].div(rem), jj = rem - ii * sg.J;
        bf[sg.bft_off + (int64_t)jj * sg.It + ii] = b1;
      }
    }
  }
  if (l2 && sg.track_l2) {
    // per-block partial, summed in block order by finalize_k: one float atomic per
    // block on ONE address serialised ~6.8K blocks (96 us of the reference CNN's
    // update) and made the weight-decay loss order-dependent
    sq = warp_sum(sq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = 0.f;
      for (int w = 0; w < TPB / 64; ++w) t += red[w];
      if (fin.ticket) st_coh(l2 + tab.l2n + blockIdx.x, t);
      else l2[tab.l2n + blockIdx.x] = t;
    }
  }
  if (!fin.ticket) return;
  // the step's finalize in this launch: the last block to take a ticket (thread 0, after its
  // coherent partial store) runs it, reading the partials coherently; every block has read
  // *step_p by now
  if (threadIdx.x == 0) last = take_ticket(fin.ticket) == nopt - 1;
  __syncthreads();
  if (!last) return;
  if (threadIdx.x == 0) *fin.ticket = 0;
  finalize_body<true>(fin, wsum);
