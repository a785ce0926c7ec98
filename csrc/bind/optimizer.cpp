// _kernels bindings: split-K reduce, the fused optimizer and its norms, the step's finalize.
#include "bind/common.h"

namespace {

mnistx::RedSpec red_spec(Tensor slab, int64_t splits, int64_t M, int64_t N, int64_t G, int64_t Ipad, int64_t I,
                         int64_t J, int64_t bias_row, Tensor wdst, const Tensor* bdst, double scale) {
  check(slab, at::kFloat, splits * M * N, "slab");
  TORCH_CHECK(I <= Ipad && J <= N && G * Ipad <= M, "reduce geometry");
  TORCH_CHECK(aligned(slab, 16), "slab must be 16-byte aligned");
  check(wdst, at::kFloat, G * I * J, "wdst");
  float* b = nullptr;
  if (bdst != nullptr && bdst->defined() && bdst->numel() > 0) {
    TORCH_CHECK(bias_row >= 0 && bias_row < M, "bias_row");
    check(*bdst, at::kFloat, J, "bdst");
    b = P<float>(*bdst);
  }
  return mnistx::RedSpec{P<float>(slab), P<float>(wdst), b, (int)splits, (int)M, (int)N, (int)G, (int)Ipad, (int)I,
                         (int)J, (int)bias_row, (float)scale};
}

void splitk_reduce(Tensor slab, int64_t splits, int64_t M, int64_t N, int64_t G, int64_t Ipad, int64_t I, int64_t J,
                   int64_t bias_row, Tensor wdst, optional<Tensor> bdst, double scale) {
  const Tensor* bp = has(bdst) ? &*bdst : nullptr;
  const mnistx::RedSpec r = red_spec(slab, splits, M, N, G, Ipad, I, J, bias_row, wdst, bp, scale);
  hip_ok(mnistx::splitk_reduce_multi(&r, 1, cur_stream()), "splitk_reduce");
}

// Several split-K slabs reduced by one launch per pass.  geo: int64 [n, 8] on CPU =
// (splits, M, N, G, Ipad, I, J, bias_row) per tensor; bdsts[i] empty = no bias.
void splitk_reduce_multi(std::vector<Tensor> slabs, std::vector<Tensor> wdsts, std::vector<Tensor> bdsts, Tensor geo,
                         std::vector<double> scales) {
  const int64_t n = (int64_t)slabs.size();
  TORCH_CHECK((int64_t)wdsts.size() == n && (int64_t)bdsts.size() == n && (int64_t)scales.size() == n,
              "splitk_reduce_multi: list lengths differ");
  TORCH_CHECK(geo.device().is_cpu() && geo.scalar_type() == at::kLong && geo.dim() == 2 && geo.size(0) == n &&
                  geo.size(1) == 8 && geo.is_contiguous(),
              "splitk_reduce_multi: geo must be a contiguous CPU int64 [n, 8] tensor");
  const int64_t* g = geo.data_ptr<int64_t>();
  std::vector<mnistx::RedSpec> specs;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t* r = g + 8 * i;
    specs.push_back(red_spec(slabs[i], r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], wdsts[i], &bdsts[i],
                             scales[i]));
  }
  hip_ok(mnistx::splitk_reduce_multi(specs.data(), (int)n, cur_stream()), "splitk_reduce_multi");
}

mnistx::FinArgs prep_fin(Tensor step, Tensor stats, optional<Tensor> l2, optional<Tensor> wds, int64_t nw,
                         optional<Tensor> loss_ema, int64_t n_ema, int64_t batch, bool increment,
                         optional<Tensor> l2_ranges, optional<Tensor> ce_work, int64_t ce_nblk) {
  check(step, at::kLong, 1, "step");
  check(stats, at::kFloat, 8, "stats");
  TORCH_CHECK(nw <= 64, "finalize: at most 64 weight-decay entries");
  mnistx::FinArgs f{};
  f.step = P<int64_t>(step);
  f.stats = P<float>(stats);
  if (nw > 0) {
    TORCH_CHECK(l2.has_value() && wds.has_value(), "l2/wds needed when nw > 0");
    check(*l2, at::kFloat, nw, "l2");
    check(*wds, at::kFloat, nw, "wds");
    f.l2 = P<float>(*l2);
    f.wds = P<const float>(*wds);
  }
  f.nw = (int)nw;
  if (has(loss_ema)) {
    check(*loss_ema, at::kFloat, 3 * n_ema, "loss_ema");
    f.loss_ema = P<float>(*loss_ema);
    f.n_ema = (int)n_ema;
  }
  if (nw > 0 && has(l2_ranges)) {
    check(*l2_ranges, at::kInt, 3 * nw, "l2_ranges");
    f.l2r = P<const int>(*l2_ranges);
    // partials follow the nw per-weight slots (binding fused_optimizer: l2n = max track index)
  }
  f.l2base = (int)nw;
  if (ce_nblk > 0) {
    TORCH_CHECK(has(ce_work) && ce_nblk <= 1024, "ce_work needed for ce_nblk > 0");
    check(*ce_work, at::kFloat, mnistx::CE_WORK_FLOATS, "ce_work");
    f.ce_work = P<const float>(*ce_work);
    f.ce_nblk = (int)ce_nblk;
  }
  f.batch = (int)batch;
  f.increment = increment ? 1 : 0;
  return f;
}

void finalize_step(Tensor step, Tensor stats, optional<Tensor> l2, optional<Tensor> wds, int64_t nw,
                   optional<Tensor> loss_ema, int64_t n_ema, int64_t batch, bool increment,
                   optional<Tensor> l2_ranges, optional<Tensor> ce_work, int64_t ce_nblk) {
  const auto f = prep_fin(step, stats, l2, wds, nw, loss_ema, n_ema, batch, increment, l2_ranges, ce_work, ce_nblk);
  hip_ok(mnistx::finalize_step(f, cur_stream()), "finalize_step");
}

// segs: int64 tensor [nseg, 14] on CPU:
//   off, n, G, I, J, Ip, Jp, bf_off, wd_bits(float32 as int), track_l2, bft_off, Jt, It, 0
// bf: the buffer of the bf16 copies, whose ranges are checked (nullptr: a caller that never
// writes them); max_l2: the largest track_l2 index
std::vector<mnistx::OptSeg> read_segs(const Tensor& segs, int64_t total, const Tensor* bf, int& max_l2) {
  TORCH_CHECK(!segs.is_cuda() && segs.scalar_type() == at::kLong && segs.dim() == 2 && segs.size(1) == 14,
              "segs: CPU int64 [n,14]");
  const int nseg = (int)segs.size(0);
  std::vector<mnistx::OptSeg> sv(nseg);
  auto a = segs.accessor<int64_t, 2>();
  int64_t expect_off = 0;
  max_l2 = 0;
  for (int i = 0; i < nseg; ++i) {
    auto& s = sv[i];
    s.off = a[i][0];
    s.n = a[i][1];
    s.G = (int)a[i][2];
    s.I = (int)a[i][3];
    s.J = (int)a[i][4];
    s.Ip = (int)a[i][5];
    s.Jp = (int)a[i][6];
    s.bf_off = a[i][7];
    int32_t wb = (int32_t)a[i][8];
    std::memcpy(&s.wd, &wb, 4);
    s.track_l2 = (int)a[i][9];
    s.bft_off = a[i][10];
    s.Jt = (int)a[i][11];
    s.It = (int)a[i][12];
    s.adapt = a[i][13] != 0 ? 1 : 0;   // lars / lamb: the variable takes its own trust ratio
    TORCH_CHECK(s.off == expect_off, "segments must tile the flat buffer in order");
    TORCH_CHECK(s.n == (int64_t)s.G * s.I * s.J, "segment size mismatch");
    TORCH_CHECK(s.Ip >= s.I && s.Jp >= s.J, "padding");
    if (bf && s.bf_off >= 0)
      TORCH_CHECK(s.bf_off + (int64_t)s.G * s.Ip * s.Jp <= bf->numel(), "bf16 copy out of range");
    if (bf && s.bft_off >= 0) {
      TORCH_CHECK(s.bf_off >= 0 && s.G == 1 && s.Jt >= s.J && s.It >= s.I, "transposed copy geometry");
      TORCH_CHECK(s.bft_off + (int64_t)s.Jt * s.It <= bf->numel(), "transposed bf16 copy out of range");
    }
    if (s.track_l2 > max_l2) max_l2 = s.track_l2;
    expect_off += s.n;
  }
  TORCH_CHECK(expect_off == total, "segments do not cover the parameters");
  return sv;
}

// The learning-rate schedule's keywords (fused_optimizer, lr_at_steps), validated; `who`: the caller's name
static mnistx::LrSched read_lr_sched(const char* who, const std::string& lr_schedule, int64_t warmup_steps,
                                     int64_t lr_total_steps, double lr_end, double lr_power) {
  std::string name = lr_schedule;
  for (auto& c : name) c = (char)std::tolower((unsigned char)c);
  mnistx::LrSched sc{};
  if (name == "staircase") sc.kind = mnistx::LR_STAIRCASE;
  else if (name == "polynomial") sc.kind = mnistx::LR_POLYNOMIAL;
  else if (name == "cosine") sc.kind = mnistx::LR_COSINE;
  else TORCH_CHECK(false, who, ": unknown lr_schedule '", lr_schedule, "' (staircase|polynomial|cosine)");
  TORCH_CHECK(warmup_steps >= 0, who, ": warmup_steps must be >= 0, got ", warmup_steps);
  TORCH_CHECK(sc.kind == mnistx::LR_STAIRCASE || lr_total_steps > warmup_steps, who,
              ": lr_total_steps must be > warmup_steps (", warmup_steps, "), got ", lr_total_steps);
  TORCH_CHECK(std::isfinite(lr_end) && lr_end >= 0 && std::isfinite((float)lr_end), who,
              ": lr_end must be finite and >= 0, got ", lr_end);
  TORCH_CHECK(std::isfinite(lr_power) && lr_power > 0 && (float)lr_power > 0.f && std::isfinite((float)lr_power), who,
              ": lr_power must be finite and > 0, got ", lr_power);
  sc.warmup = warmup_steps;
  sc.total = lr_total_steps;
  sc.lr_end = (float)lr_end;
  sc.power = (float)lr_power;
  return sc;
}

// out[i] = the learning rate the optimizer launch applies at global step steps[i]: the device's
// own sched_lr, for tests and for plotting a schedule
void lr_at_steps(Tensor steps, Tensor out, double lr0, double decay_rate, int64_t decay_steps,
                 const std::string& lr_schedule, int64_t warmup_steps, int64_t lr_total_steps, double lr_end,
                 double lr_power) {
  const int64_t n = steps.numel();
  check(steps, at::kLong, n, "steps");
  check(out, at::kFloat, n, "out");
  TORCH_CHECK(out.device() == steps.device(), "out: on the steps' device");
  const mnistx::LrSched sc = read_lr_sched("lr_at_steps", lr_schedule, warmup_steps, lr_total_steps, lr_end, lr_power);
  hip_ok(mnistx::lr_at_steps(P<const int64_t>(steps), P<float>(out), n, (float)lr0, (float)decay_rate, decay_steps, sc,
                             cur_stream()),
         "lr_at_steps");
}

// the Adam / LAMB moment coefficients of a launch (fused_optimizer, var_norms)
void moment_coeffs(mnistx::OptParams& op, double beta1, double beta2) {
  op.b1 = (float)beta1;
  op.omb1 = (float)(1.0 - beta1);
  op.b2 = (float)beta2;
  op.omb2 = (float)(1.0 - beta2);
  op.log_b1 = beta1 > 0 ? std::log(beta1) : -1e300;   // beta = 0: b^t = 0, the correction is 1
  op.log_b2 = beta2 > 0 ? std::log(beta2) : -1e300;
}

void fused_optimizer(Tensor params, Tensor grads, Tensor mom, Tensor ema, Tensor bf, Tensor segs, Tensor step,
                     double lr0, double decay_rate, int64_t decay_steps, double momentum, bool nesterov,
                     bool use_momentum, double grad_scale, double ema_max, optional<Tensor> l2,
                     optional<Tensor> guard, int64_t guard_want, optional<Tensor> guard_err, int64_t guard_id,
                     optional<py::tuple> fin, optional<py::tuple> perm, const std::string& rule,
                     optional<Tensor> slot2, double beta1, double beta2, optional<double> epsilon,
                     double rmsprop_decay, optional<double> clip_norm, optional<Tensor> gnorm, double lars_eta,
                     optional<Tensor> tnorm, const std::string& lr_schedule, int64_t warmup_steps,
                     int64_t lr_total_steps, double lr_end, double lr_power) {
  const int64_t total = params.numel();
  check(params, at::kFloat, total, "params");
  check(grads, at::kFloat, total, "grads");
  // the schedule: the plain staircase (no warmup) is the launch as it always was
  const mnistx::LrSched sched =
      read_lr_sched("fused_optimizer", lr_schedule, warmup_steps, lr_total_steps, lr_end, lr_power);
  const bool scheduled = !mnistx::lr_sched_is_default(sched);
  TORCH_CHECK(!(scheduled && has(guard)), "fused_optimizer: lr_schedule '", lr_schedule, "' / warmup_steps ",
              warmup_steps, " cannot be combined with a push guard (parameter-server mode)");
  // rule: the classic names leave the choice to use_momentum / nesterov, as before
  int rule_id = mnistx::OPT_CLASSIC;
  if (rule == "adam") rule_id = mnistx::OPT_ADAM;
  else if (rule == "rmsprop") rule_id = mnistx::OPT_RMSPROP;
  else if (rule == "adagrad") rule_id = mnistx::OPT_ADAGRAD;
  else if (rule == "lars") rule_id = mnistx::OPT_LARS;
  else if (rule == "lamb") rule_id = mnistx::OPT_LAMB;
  else TORCH_CHECK(rule == "sgd" || rule == "momentum" || rule == "nesterov",
                   "fused_optimizer: unknown rule '", rule, "' (sgd|momentum|nesterov|adam|rmsprop|adagrad|lars|lamb)");
  const bool layerwise = rule_id == mnistx::OPT_LARS || rule_id == mnistx::OPT_LAMB;
  if (rule_id == mnistx::OPT_LARS) {   // momentum with a trust ratio: the momentum slot, never Nesterov
    use_momentum = true;
    nesterov = false;
  }
  const bool adaptive = rule_id != mnistx::OPT_CLASSIC;
  const bool two_slots = rule_id == mnistx::OPT_ADAM || rule_id == mnistx::OPT_RMSPROP || rule_id == mnistx::OPT_LAMB;
  if (use_momentum || adaptive) check(mom, at::kFloat, total, "mom");
  if (two_slots) {
    TORCH_CHECK(has(slot2), "fused_optimizer: rule '", rule, "' needs slot2");
    check(*slot2, at::kFloat, total, "slot2");
    TORCH_CHECK(slot2->data_ptr() != mom.data_ptr(), "slot2 aliases mom");
  }
  if (rule_id == mnistx::OPT_ADAM || rule_id == mnistx::OPT_LAMB)
    TORCH_CHECK(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1, rule, ": beta1, beta2 in [0, 1)");
  if (rule_id == mnistx::OPT_RMSPROP) TORCH_CHECK(rmsprop_decay >= 0 && rmsprop_decay <= 1, "rmsprop: decay in [0, 1]");
  if (ema_max >= 0) check(ema, at::kFloat, total, "ema");
  check(step, at::kLong, 1, "step");
  int max_l2 = 0;
  const std::vector<mnistx::OptSeg> sv = read_segs(segs, total, &bf, max_l2);
  const int nseg = (int)sv.size();
  check(bf, at::kBFloat16, 0, "bf");
  float* l2p = nullptr;
  const int l2n = max_l2;
  if (has(l2)) {
    // [max_l2 per-tensor sums | one partial per optimizer block]
    check(*l2, at::kFloat, (int64_t)max_l2 + mnistx::fused_optimizer_blocks(sv.data(), nseg), "l2");
    l2p = P<float>(*l2);
  }
  mnistx::OptParams op{};
  op.lr0 = (float)lr0;
  op.decay_rate = (float)decay_rate;
  op.decay_steps = decay_steps;
  op.momentum = (float)momentum;
  op.nesterov = nesterov ? 1 : 0;
  op.use_momentum = use_momentum ? 1 : 0;
  op.grad_scale = (float)grad_scale;
  op.ema_max = (float)ema_max;
  op.rule = rule_id;
  if (rule_id == mnistx::OPT_ADAM || rule_id == mnistx::OPT_LAMB) {
    moment_coeffs(op, beta1, beta2);
    op.eps = (float)epsilon.value_or(rule_id == mnistx::OPT_LAMB ? 1e-6 : 1e-8);
  } else if (rule_id == mnistx::OPT_RMSPROP) {
    op.b2 = (float)rmsprop_decay;
    op.omb2 = (float)(1.0 - rmsprop_decay);
    op.eps = (float)epsilon.value_or(1e-10);
  } else if (rule_id == mnistx::OPT_LARS) {
    op.eps = (float)epsilon.value_or(0.0);
  }
  if (has(guard)) {   // PS push guard: int64 stamp on the device
    check(*guard, at::kLong, 1, "guard");
    TORCH_CHECK(has(guard_err), "guard needs guard_err");
    check(*guard_err, at::kInt, 1, "guard_err");
    TORCH_CHECK(guard->device() == params.device() && guard_err->device() == params.device(),
                "guard / guard_err: on the parameters' device");
    op.guard = P<const int64_t>(*guard);
    op.guard_want = guard_want;
    op.guard_err = P<int>(*guard_err);
    op.guard_id = (int)guard_id;
  }
  // clipping by global norm: gnorm = [norm, scale, grad_norm_max_blocks() partials]
  float clip = 0.f;
  float* gnp = nullptr;
  if (clip_norm.has_value()) {
    TORCH_CHECK(std::isfinite(*clip_norm) && *clip_norm > 0 && (float)*clip_norm > 0.f &&
                    std::isfinite((float)*clip_norm), "fused_optimizer: clip_norm must be finite and > 0");
    TORCH_CHECK(has(gnorm), "fused_optimizer: clip_norm needs gnorm");
    TORCH_CHECK(!has(guard), "fused_optimizer: clip_norm cannot be combined with a push guard (parameter-server mode)");
    check(*gnorm, at::kFloat, 2 + mnistx::grad_norm_max_blocks(), "gnorm");
    TORCH_CHECK(gnorm->device() == params.device(), "gnorm: on the parameters' device");
    clip = (float)*clip_norm;
    gnp = P<float>(*gnorm);
  }
  // layer-wise trust ratios: tnorm = [nvar x (pnorm, unorm, ratio) | the reduction's partials]
  float* tnp = nullptr;
  if (layerwise) {
    TORCH_CHECK(std::isfinite(lars_eta) && lars_eta > 0 && (float)lars_eta > 0.f && std::isfinite((float)lars_eta),
                "fused_optimizer: lars_eta must be finite and > 0");
    TORCH_CHECK(!clip_norm.has_value(), "fused_optimizer: rule '", rule, "' cannot be combined with clip_norm");
    TORCH_CHECK(!has(guard), "fused_optimizer: rule '", rule,
                "' cannot be combined with a push guard (parameter-server mode)");
    TORCH_CHECK(has(tnorm), "fused_optimizer: rule '", rule, "' needs tnorm");
    check(*tnorm, at::kFloat, mnistx::var_norm_buffer_size(nseg), "tnorm");
    TORCH_CHECK(tnorm->device() == params.device(), "tnorm: on the parameters' device");
    tnp = P<float>(*tnorm);
  }
  // fin: finalize_step's arguments after `step` (the same step tensor), run in this launch
  mnistx::FinArgs fa{};
  const bool has_fin = fin.has_value() && !fin->is_none();
  if (has_fin) {
    const py::tuple& t = *fin;
    TORCH_CHECK(t.size() == 11, "fin: (stats, l2, wds, nw, loss_ema, n_ema, batch, increment, l2_ranges, ce_work, ce_nblk)");
    auto ot = [&](int i) { return t[i].is_none() ? optional<Tensor>() : optional<Tensor>(t[i].cast<Tensor>()); };
    fa = prep_fin(step, t[0].cast<Tensor>(), ot(1), ot(2), t[3].cast<int64_t>(), ot(4), t[5].cast<int64_t>(),
                  t[6].cast<int64_t>(), t[7].cast<bool>(), ot(8), ot(9), t[10].cast<int64_t>());
  }
  // perm: (out, lab_src, lab_out, start, N, seed, h) -- perm_positions of the next batch, run by
  // extra blocks of this launch
  mnistx::PermJob pj{};
  const bool has_perm = perm.has_value() && !perm->is_none();
  if (has_perm) {
    const py::tuple& t = *perm;
    TORCH_CHECK(t.size() == 7, "perm: (out, lab_src, lab_out, start, N, seed, h)");
    Tensor out = t[0].cast<Tensor>(), ls = t[1].cast<Tensor>(), lo = t[2].cast<Tensor>();
    const int64_t start = t[3].cast<int64_t>(), N = t[4].cast<int64_t>(), seed = t[5].cast<int64_t>(),
                  h = t[6].cast<int64_t>();
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kLong && out.is_contiguous() &&
                    out.device() == params.device(), "perm: out");
    perm_domain("perm", N, h);
    TORCH_CHECK(out.numel() < (1ll << 31), "perm: too many rows");
    check(ls, at::kInt, N, "perm lab_src");
    check(lo, at::kInt, out.numel(), "perm lab_out");
    pj.out = out.data_ptr<int64_t>();
    pj.lab_src = P<const int32_t>(ls);
    pj.lab_out = P<int32_t>(lo);
    pj.start = start;
    pj.N = N;
    pj.seed = (uint32_t)seed;
    pj.h = (int)h;
    pj.n = (int)out.numel();
  }
  hip_ok(mnistx::fused_optimizer(P<float>(params), P<const float>(grads),
                                 (use_momentum || adaptive) ? P<float>(mom) : nullptr,
                                 ema_max >= 0 ? P<float>(ema) : nullptr, BFm(bf), sv.data(), nseg,
                                 P<const int64_t>(step), op, l2p, l2n, cur_stream(), has_fin ? &fa : nullptr,
                                 has_perm ? &pj : nullptr, two_slots ? P<float>(*slot2) : nullptr, clip, gnp,
                                 (float)lars_eta, tnp, scheduled ? &sched : nullptr),
         "fused_optimizer");
}

// The per-variable norms and trust ratios alone, as the lars / lamb update computes them:
// tnorm[3 k .. 3 k + 2] = ||p_k||, ||g_k|| (lars) or ||u_k|| (lamb), r_k afterwards.  Not on the
// training path.
void var_norms(Tensor params, Tensor grads, Tensor segs, double grad_scale, Tensor tnorm, const std::string& rule,
               optional<Tensor> mom, optional<Tensor> slot2, optional<Tensor> step, double beta1, double beta2,
               optional<double> epsilon, double lars_eta) {
  const int64_t total = params.numel();
  check(params, at::kFloat, total, "params");
  check(grads, at::kFloat, total, "grads");
  TORCH_CHECK(rule == "lars" || rule == "lamb", "var_norms: rule lars|lamb");
  const bool lamb = rule == "lamb";
  TORCH_CHECK(std::isfinite(lars_eta) && (float)lars_eta > 0.f && std::isfinite((float)lars_eta),
              "var_norms: lars_eta must be finite and > 0");
  int max_l2 = 0;
  const std::vector<mnistx::OptSeg> sv = read_segs(segs, total, nullptr, max_l2);
  check(tnorm, at::kFloat, mnistx::var_norm_buffer_size((int)sv.size()), "tnorm");
  TORCH_CHECK(grads.device() == params.device() && tnorm.device() == params.device(),
              "grads / tnorm: on the parameters' device");
  mnistx::OptParams op{};
  op.grad_scale = (float)grad_scale;
  op.rule = lamb ? mnistx::OPT_LAMB : mnistx::OPT_LARS;
  op.eps = (float)epsilon.value_or(lamb ? 1e-6 : 0.0);
  const float *mp = nullptr, *sp = nullptr;
  const int64_t* stp = nullptr;
  if (lamb) {
    TORCH_CHECK(has(mom) && has(slot2) && has(step), "var_norms: lamb needs mom, slot2 and step");
    check(*mom, at::kFloat, total, "mom");
    check(*slot2, at::kFloat, total, "slot2");
    check(*step, at::kLong, 1, "step");
    TORCH_CHECK(mom->device() == params.device() && slot2->device() == params.device() &&
                    step->device() == params.device(), "mom / slot2 / step: on the parameters' device");
    TORCH_CHECK(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1, "lamb: beta1, beta2 in [0, 1)");
    moment_coeffs(op, beta1, beta2);
    mp = P<const float>(*mom);
    sp = P<const float>(*slot2);
    stp = P<const int64_t>(*step);
  }
  hip_ok(mnistx::var_norms(P<const float>(params), P<const float>(grads), mp, sp, sv.data(), (int)sv.size(), stp, op,
                           (float)lars_eta, P<float>(tnorm), cur_stream()),
         "var_norms");
}

// The global norm of g_eff = grad * grad_scale + wd * p alone, as the clipped update computes it:
// gnorm[0] afterwards (gnorm[2..]: the per-block partials).  Not on the training path.
void grad_global_norm(Tensor params, Tensor grads, Tensor segs, double grad_scale, Tensor gnorm) {
  const int64_t total = params.numel();
  check(params, at::kFloat, total, "params");
  check(grads, at::kFloat, total, "grads");
  check(gnorm, at::kFloat, 2 + mnistx::grad_norm_max_blocks(), "gnorm");
  TORCH_CHECK(grads.device() == params.device() && gnorm.device() == params.device(),
              "grads / gnorm: on the parameters' device");
  int max_l2 = 0;
  const std::vector<mnistx::OptSeg> sv = read_segs(segs, total, nullptr, max_l2);
  hip_ok(mnistx::grad_global_norm(P<const float>(params), P<const float>(grads), sv.data(), (int)sv.size(),
                                  (float)grad_scale, P<float>(gnorm), cur_stream()),
         "grad_global_norm");
}

}  // namespace

void bind_optimizer(py::module_& m) {
  m.def("splitk_reduce", &splitk_reduce);
  m.def("splitk_reduce_multi", &splitk_reduce_multi);
  m.def("set_reduce_fused", [](int64_t on) { mnistx::set_reduce_fused((int)on); },
        "A/B switch of the one-launch split-K reduce (MNISTX_REDUCE_FUSED)");
  m.def("reduce_fused_enabled", []() { return mnistx::reduce_fused_enabled() != 0; });
  m.def("finalize_step", &finalize_step, py::arg("step"), py::arg("stats"), py::arg("l2"), py::arg("wds"),
        py::arg("nw"), py::arg("loss_ema"), py::arg("n_ema"), py::arg("batch"), py::arg("increment"),
        py::arg("l2_ranges") = py::none(), py::arg("ce_work") = py::none(), py::arg("ce_nblk") = 0);
  m.def("set_opt_fin_fused", [](int64_t on) { mnistx::set_opt_fin_fused((int)on); },
        "A/B switch of the optimizer launch running the step's finalize (MNISTX_OPT_FIN_FUSED)");
  m.def("opt_fin_fused_enabled", []() { return mnistx::opt_fin_fused_enabled() != 0; });
  m.def("lr_at_steps", &lr_at_steps, py::arg("steps"), py::arg("out"), py::arg("lr0"), py::arg("decay_rate"),
        py::arg("decay_steps"), py::kw_only(), py::arg("lr_schedule") = "staircase", py::arg("warmup_steps") = 0,
        py::arg("lr_total_steps") = 0, py::arg("lr_end") = 0.0, py::arg("lr_power") = 1.0,
        "out[i] = the learning rate the optimizer launch applies at global step steps[i] (the device's own function)");
  m.def("fused_optimizer", &fused_optimizer, py::arg("params"), py::arg("grads"), py::arg("mom"), py::arg("ema"),
        py::arg("bf"), py::arg("segs"), py::arg("step"), py::arg("lr0"), py::arg("decay_rate"),
        py::arg("decay_steps"), py::arg("momentum"), py::arg("nesterov"), py::arg("use_momentum"),
        py::arg("grad_scale"), py::arg("ema_max"), py::arg("l2") = py::none(), py::arg("guard") = py::none(),
        py::arg("guard_want") = 0, py::arg("guard_err") = py::none(), py::arg("guard_id") = 0,
        py::arg("fin") = py::none(), py::arg("perm") = py::none(), py::kw_only(), py::arg("rule") = "sgd",
        py::arg("slot2") = py::none(), py::arg("beta1") = 0.9, py::arg("beta2") = 0.999,
        py::arg("epsilon") = py::none(), py::arg("rmsprop_decay") = 0.9, py::arg("clip_norm") = py::none(),
        py::arg("gnorm") = py::none(), py::arg("lars_eta") = 0.001, py::arg("tnorm") = py::none(),
        py::arg("lr_schedule") = "staircase", py::arg("warmup_steps") = 0, py::arg("lr_total_steps") = 0,
        py::arg("lr_end") = 0.0, py::arg("lr_power") = 1.0);
  m.def("fused_optimizer_blocks", [](Tensor segs) {
    TORCH_CHECK(!segs.is_cuda() && segs.scalar_type() == at::kLong && segs.dim() == 2, "segs: CPU int64 [n,14]");
    auto a = segs.accessor<int64_t, 2>();
    std::vector<mnistx::OptSeg> sv(segs.size(0));
    for (int64_t i = 0; i < segs.size(0); ++i) sv[i].n = a[i][1];
    return (int64_t)mnistx::fused_optimizer_blocks(sv.data(), (int)sv.size());
  });
  m.def("var_norms", &var_norms, py::arg("params"), py::arg("grads"), py::arg("segs"), py::arg("grad_scale"),
        py::arg("tnorm"), py::kw_only(), py::arg("rule") = "lars", py::arg("mom") = py::none(),
        py::arg("slot2") = py::none(), py::arg("step") = py::none(), py::arg("beta1") = 0.9, py::arg("beta2") = 0.999,
        py::arg("epsilon") = py::none(), py::arg("lars_eta") = 0.001,
        "tnorm[3k..3k+2] = ||p_k||, ||g_k|| (lars) or ||u_k|| (lamb), trust ratio r_k; fixed-order sums");
  m.def("var_norm_buffer_size", [](int64_t nvar) { return (int64_t)mnistx::var_norm_buffer_size((int)nvar); });
  m.def("set_layerwise_self_sum", [](int64_t mode) { mnistx::set_layerwise_self_sum((int)mode); },
        "A/B switch of the lars / lamb ratio hand-off: 1 = every apply block sums its variable's partials, "
        "0 = a one-block-per-variable launch does, -1 (default) = by size (MNISTX_LAYERWISE_SELF_SUM)");
  m.def("layerwise_self_sum_mode", []() { return (int64_t)mnistx::layerwise_self_sum_mode(); });
  m.def("grad_global_norm", &grad_global_norm, py::arg("params"), py::arg("grads"), py::arg("segs"),
        py::arg("grad_scale"), py::arg("gnorm"),
        "gnorm[0] = sqrt(sum over all segments of (grad * grad_scale + wd * p)^2), fixed-order sums");
  m.def("grad_norm_max_blocks", []() { return (int64_t)mnistx::grad_norm_max_blocks(); });
}
