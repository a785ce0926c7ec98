// The softmax cross-entropy of both fused heads (mlp_head.hip: mlp_head_k and ce_tail_k), included
// inside each kernel, as fused_opt_body.h is: a device function is simplified on its own before it
// is inlined, and the plain instantiations then came out of the compiler as other code (operands
// commuted, the dlogits no longer paired into v_pk_fma_f32: mlp_head_k<true> 4291 -> 4302
// instructions), where this text gives them the code they had.  In scope:
//   GRADS, tg (the kernel's CeTarget, ce_stats.h), lg[8] (the logits of batch row m: register i of lane
//   half h holds class (i&3) + 8(i>>2) + 4h), lab (its label; -1 past the batch), m, nb, nc, h, valid, scale,
//   dl, loss / corr / bad (the thread's CE statistics), cs[8] (fp32 dlogits column sums, dbias).
// A DISTILL target also reads the teacher's row here (tg.trow) and keeps its soft part in the Row.
// The text ends INSIDE its `if constexpr (GRADS) {` block, which the kernel goes on with (its
// data-gradient chain) and closes: dlp[4], the row's packed bf16 dlogits and the B operand of the fc5
// data gradient, is declared in there, because declared outside -- dead in the eval forms -- it was
// enough to reorder their registers.
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if ((i & 3) + 8 * (i >> 2) + 4 * h < nc) mx = fmaxf(mx, lg[i]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float e[8], se = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      e[i] = ((i & 3) + 8 * (i >> 2) + 4 * h < nc) ? __expf(lg[i] - mx) : 0.f;
      se += e[i];
    }
    se += __shfl_xor(se, 32, 64);
    if (!valid) lab = -1;
    float ll = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) ll = ((i & 3) + 8 * (i >> 2) + 4 * h == lab) ? lg[i] : ll;
    ll += __shfl_xor(ll, 32, 64);
    typename TG::Row row = tg.row(lab, min(m, nb - 1));
    if constexpr (TG::NEEDS_DB) {   // l_yb, found and joined as ll is
      float lb = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) lb = ((i & 3) + 8 * (i >> 2) + 4 * h == row.yb) ? lg[i] : lb;
      lb += __shfl_xor(lb, 32, 64);
      row.db = lb - mx;
    }
    if constexpr (TG::NEEDS_SD) {   // the masked class sum of l_c - mx, joined likewise
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if ((i & 3) + 8 * (i >> 2) + 4 * h < nc) row.sd += lg[i] - mx;
      row.sd += __shfl_xor(row.sd, 32, 64);
    }
    // DISTILL: the teacher's row, loaded once and under no branch (a clamped column: the columns >= nc
    // are never read), in the class layout of lg[]; the row sums st and seT joined as se is.
    if constexpr (TG::DISTILL) {
      const float* tp = tg.trow(min(m, nb - 1));
      const float iT = tg.dist->iT;
      float tv[8], tm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 8; ++i) tv[i] = tp[min((i & 3) + 8 * (i >> 2) + 4 * h, nc - 1)];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if ((i & 3) + 8 * (i >> 2) + 4 * h < nc) tm = fmaxf(tm, tv[i]);
      tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
      float ev[8], eu[8], st = 0.f, seT = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const bool in = (i & 3) + 8 * (i >> 2) + 4 * h < nc;
        tv[i] = (tv[i] - tm) * iT;                       // v_c
        ev[i] = in ? __expf(tv[i]) : 0.f;
        eu[i] = in ? __expf((lg[i] - mx) * iT) : 0.f;    // exp(u_c)
        st += ev[i];
        seT += eu[i];
      }
      st += __shfl_xor(st, 32, 64);
      seT += __shfl_xor(seT, 32, 64);
      const float ist = 1.f / st, iseT = 1.f / seT, lst = __logf(st), lseT = __logf(seT);
      float soft = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float qc = ev[i] * ist;
        row.ps[i] = eu[i] * iseT - qc;
        if ((i & 3) + 8 * (i >> 2) + 4 * h < nc) soft += qc * ((tv[i] - lst) - ((lg[i] - mx) * iT - lseT));
      }
      row.soft = soft + __shfl_xor(soft, 32, 64);
    }
    if (valid && h == 0) {
      const float lo = tg.loss(row, ll - mx, __logf(se));
      loss += lo;
      corr += (ll >= mx) ? 1.f : 0.f;
      bad = isfinite(lo) ? bad : 1.f;
    }
    if constexpr (GRADS) {   // closed by the including kernel, after its data-gradient chain
      uint32_t dlp[4];
      const float inv = 1.f / se;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        float g2[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int i = 2 * w + k, cls = (i & 3) + 8 * (i >> 2) + 4 * h;
          if constexpr (TG::DISTILL) g2[k] = cls < nc ? tg.dgrad(e[i] * inv - tg.q(row, cls), row.ps[i]) * scale : 0.f;
          else
          g2[k] = cls < nc ? (e[i] * inv - tg.q(row, cls)) * scale : 0.f;
          cs[i] += valid ? g2[k] : 0.f;
        }
        dlp[w] = pack2(g2[0], g2[1]);
      }
      if (valid)
#pragma unroll
        for (int q = 0; q < 2; ++q) *(u32x2*)(dl + (int64_t)m * LD3 + 8 * q + 4 * h) = u32x2{dlp[2 * q], dlp[2 * q + 1]};
