// _kernels bindings: softmax cross-entropy, the fused dense heads, dropout.
#include "bind/common.h"

namespace {

// label_smoothing of the softmax-CE bindings: finite, 0 <= eps < 1
float smoothing_arg(double eps, const char* op) {
  TORCH_CHECK_VALUE(std::isfinite(eps) && eps >= 0.0 && eps < 1.0, op, ": label_smoothing must be finite with 0 <= "
              "label_smoothing < 1, got ", eps);
  return (float)eps;
}

// labels2 / lam of the softmax-CE bindings (mixup / CutMix): both or neither (ValueError), int32 [nb]
// and fp32 [nb] on the labels' device
struct MixArgs {
  const int32_t* labels2 = nullptr;
  const float* lam = nullptr;
};
MixArgs mix_args(const optional<Tensor>& labels2, const optional<Tensor>& lam, int64_t nb, const Tensor* labels,
                 const char* op) {
  const bool h2 = has(labels2), hl = has(lam);
  TORCH_CHECK_VALUE(h2 == hl, op, ": labels2 and lam come together, got ", h2 ? "labels2" : "lam", " alone");
  MixArgs a;
  if (!h2) return a;
  TORCH_CHECK_VALUE(labels != nullptr, op, ": labels2 and lam need labels");
  check(*labels2, at::kInt, nb, "labels2");
  check(*lam, at::kFloat, nb, "lam");
  TORCH_CHECK(labels2->device() == labels->device() && lam->device() == labels->device(), op,
              ": labels2 and lam must be on the labels' device");
  a.labels2 = P<const int32_t>(*labels2);
  a.lam = P<const float>(*lam);
  return a;
}

// teacher_logits / teacher_ld / distill_alpha / distill_temperature of the softmax-CE bindings (knowledge
// distillation, ce_stats.h DISTILL).  All of it is checked before anything is launched (ValueError):
// alpha finite in [0, 1]; T finite and > 0 with T * T finite in fp32; the teacher fp32, contiguous, on
// `like`'s device, teacher_ld >= nc and at least nb * teacher_ld elements; never together with a
// non-zero label_smoothing, labels2 / lam or dropout.  on == false (no teacher, or alpha == 0): the launch
// without the keywords.
struct DistillArgs {
  bool on = false;
  mnistx::CeDistill d{};
};
DistillArgs distill_args(const optional<Tensor>& teacher, int64_t ld, double alpha, double T, int64_t nb, int64_t nc,
                         const Tensor& like, float eps, bool mixed, bool dropped, const char* op) {
  TORCH_CHECK_VALUE(std::isfinite(alpha) && alpha >= 0.0 && alpha <= 1.0, op,
                    ": distill_alpha must be finite with 0 <= distill_alpha <= 1, got ", alpha);
  const float Tf = (float)T;
  TORCH_CHECK_VALUE(std::isfinite(T) && T > 0.0 && Tf > 0.f && std::isfinite(Tf * Tf) && std::isfinite(1.f / Tf), op,
                    ": distill_temperature must be finite and > 0 with its square finite in fp32, got ", T);
  DistillArgs a;
  if (!has(teacher)) return a;
  TORCH_CHECK_VALUE(eps == 0.f, op, ": teacher_logits cannot be combined with label_smoothing (", eps, ")");
  TORCH_CHECK_VALUE(!mixed, op, ": teacher_logits cannot be combined with labels2 / lam");
  TORCH_CHECK_VALUE(!dropped, op, ": teacher_logits cannot be combined with dropout");
  TORCH_CHECK_VALUE(teacher->is_cuda() && teacher->device() == like.device(), op,
                    ": teacher_logits must be a GPU tensor on the logits' device, got ", teacher->device());
  TORCH_CHECK_VALUE(teacher->scalar_type() == at::kFloat, op, ": teacher_logits must be float32, got ",
                    teacher->scalar_type());
  TORCH_CHECK_VALUE(teacher->is_contiguous(), op, ": teacher_logits must be contiguous");
  TORCH_CHECK_VALUE(ld >= nc && ld < ((int64_t)1 << 31), op, ": teacher_ld must be >= n_classes (", nc, "), got ", ld);
  TORCH_CHECK_VALUE(nb >= 0 && teacher->numel() >= nb * ld, op, ": teacher_logits needs ", nb * ld, " elements (",
                    nb, " rows of teacher_ld ", ld, "), has ", teacher->numel());
  if (alpha == 0.0) return a;   // the plain launch
  a.on = true;
  a.d = mnistx::CeDistill{P<const float>(*teacher), (int)ld, (float)alpha, Tf, 1.f / Tf};
  return a;
}

int64_t softmax_ce(Tensor logits, int64_t ldl, optional<Tensor> labels, int64_t B, int64_t NC, double scale,
                   optional<Tensor> dlogits, int64_t ldd, optional<Tensor> stats, optional<Tensor> probs,
                   optional<Tensor> work, bool defer_stats, optional<Tensor> dbias, double label_smoothing,
                   optional<Tensor> labels2, optional<Tensor> lam, optional<Tensor> teacher_logits, int64_t teacher_ld,
                   double distill_alpha, double distill_temperature) {
  const float eps = smoothing_arg(label_smoothing, "softmax_ce");
  const MixArgs mx = mix_args(labels2, lam, B, has(labels) ? &*labels : nullptr, "softmax_ce");
  const DistillArgs ds = distill_args(teacher_logits, teacher_ld, distill_alpha, distill_temperature, B, NC, logits, eps,
                                      mx.labels2 != nullptr, false, "softmax_ce");
  TORCH_CHECK_VALUE(!ds.on || has(labels), "softmax_ce: teacher_logits needs labels");
  TORCH_CHECK(ldl >= NC, "ldl < NC");
  check(logits, at::kFloat, B * ldl, "logits");   // whole padded rows (vector loads)
  const int32_t* lab = nullptr;
  if (has(labels)) {
    check(*labels, at::kInt, B, "labels");
    lab = P<const int32_t>(*labels);
  }
  TORCH_CHECK(eps == 0.f || lab != nullptr, "softmax_ce: label_smoothing needs labels");
  mnistx::bf16_t* dl = nullptr;
  if (has(dlogits)) {
    TORCH_CHECK(lab != nullptr, "dlogits needs labels");
    TORCH_CHECK(ldd >= NC, "ldd < NC");
    check(*dlogits, at::kBFloat16, B * ldd, "dlogits");
    TORCH_CHECK(ldd == ldl || ldd >= NC, "ldd");
    dl = BFm(*dlogits);
  }
  float* st = nullptr;
  if (has(stats)) {
    check(*stats, at::kFloat, 8, "stats");
    st = P<float>(*stats);
  }
  float* pr = nullptr;
  if (has(probs)) {
    check(*probs, at::kFloat, B * NC, "probs");
    pr = P<float>(*probs);
  }
  float* wk = nullptr;
  if (has(work)) {
    check(*work, at::kFloat, mnistx::CE_WORK_FLOATS, "work");
    wk = P<float>(*work);
  }
  float* db = nullptr;
  if (has(dbias)) {
    TORCH_CHECK(dl != nullptr, "dbias needs dlogits");
    const int nblk = mnistx::softmax_ce_dbias_blocks((int)B, (int)ldl);
    TORCH_CHECK(nblk > 0, "dbias: only the row kernel (ldl 16 / 32) writes bias partials");
    check(*dbias, at::kFloat, (int64_t)nblk * ldl, "dbias");
    db = P<float>(*dbias);
  }
  int deferred = 0;
  hip_ok(mnistx::softmax_ce(P<const float>(logits), (int)ldl, lab, (int)B, (int)NC, (float)scale, dl, (int)ldd, st, pr,
                            wk, cur_stream(), defer_stats ? &deferred : nullptr, db, eps, mx.labels2, mx.lam,
                            ds.on ? &ds.d : nullptr),
         "softmax_ce");
  return deferred;   // blocks whose CE partials the caller's finalize_step must combine
}

bool mlp_head_supported(int64_t d0, int64_t ld1, int64_t ld2, int64_t ld3, int64_t n1, int64_t n2, int64_t nc,
                        int64_t B) {
  return mnistx::mlp_head_supported((int)d0, (int)ld1, (int)ld2, (int)ld3, (int)n1, (int)n2, (int)nc, (int)B);
}

// Fused LeNet-5 dense head.  x [>=nb, 400] bf16; w3t [128,416], w4t [96,128], w5t [16,96]
// zero-padded transposed bf16 weights (FlatParams.bf16t_view); outputs h3 [nb,120], h4 [nb,88] bf16, logits [nb,16] fp32;
// with dl: dl [nb,16], dh4 [nb,88], dh3 [nb,120], dx [nb,400] bf16.
bool ce_tail_supported(int64_t d0, int64_t nc, int64_t B) { return mnistx::ce_tail_supported((int)d0, (int)nc, (int)B); }

// the reference CNN's softmax_linear + softmax CE (+ data gradient masked by x > 0): mlp_head.hip ce_tail_k
void ce_tail(Tensor x, Tensor w5t, Tensor b5, int64_t nc, Tensor labels, int64_t nb, double scale, Tensor logits,
             optional<Tensor> dl, optional<Tensor> dx, Tensor stats, optional<Tensor> work, bool defer_stats,
             optional<Tensor> dbias, double label_smoothing, optional<Tensor> labels2, optional<Tensor> lam,
             optional<Tensor> teacher_logits, int64_t teacher_ld, double distill_alpha, double distill_temperature) {
  const float eps = smoothing_arg(label_smoothing, "ce_tail");
  const MixArgs mx = mix_args(labels2, lam, nb, &labels, "ce_tail");
  const DistillArgs ds = distill_args(teacher_logits, teacher_ld, distill_alpha, distill_temperature, nb, nc, x, eps,
                                      mx.labels2 != nullptr, false, "ce_tail");
  TORCH_CHECK_VALUE(!ds.on || has(dl), "ce_tail: teacher_logits is a training quantity and needs dl");
  TORCH_CHECK(mnistx::ce_tail_supported(192, (int)nc, (int)std::max<int64_t>(nb, 1)), "ce_tail: unsupported geometry");
  check(x, at::kBFloat16, nb * 192, "x");
  check(w5t, at::kBFloat16, 16 * 192, "w5t");
  check(b5, at::kFloat, nc, "b5");
  check(labels, at::kInt, nb, "labels");
  check(logits, at::kFloat, nb * 16, "logits");
  check(stats, at::kFloat, 8, "stats");
  for (const Tensor* t : {&x, &w5t, &logits})
    TORCH_CHECK(aligned(*t, 16), "ce_tail: operands must be 16-byte aligned");
  const bool has_work = has(work);
  if (has_work) check(*work, at::kFloat, mnistx::CE_WORK_FLOATS, "work");
  mnistx::bf16_t *pdl = nullptr, *pdx = nullptr;
  if (has(dl)) {
    TORCH_CHECK(has(dx), "ce_tail: dl needs dx");
    check(*dl, at::kBFloat16, nb * 16, "dl");
    check(*dx, at::kBFloat16, nb * 192, "dx");
    for (const Tensor* t : {&*dl, &*dx})
      TORCH_CHECK(aligned(*t, 16), "ce_tail: gradients must be 16-byte aligned");
    pdl = BFm(*dl);
    pdx = BFm(*dx);
  }
  float* db = nullptr;
  if (has(dbias)) {
    TORCH_CHECK(pdl != nullptr, "ce_tail: dbias needs dl");
    check(*dbias, at::kFloat, (int64_t)mnistx::ce_tail_blocks((int)nb) * 16, "dbias");
    db = P<float>(*dbias);
  }
  TORCH_CHECK(eps == 0.f || pdl != nullptr, "ce_tail: label_smoothing is a training quantity and needs dl");
  TORCH_CHECK(mx.labels2 == nullptr || pdl != nullptr, "ce_tail: labels2 / lam are training quantities and need dl");
  const mnistx::TailArgs a{BF(x), BF(w5t), P<const float>(b5), (int)nc, P<const int32_t>(labels), (int)nb, (float)scale,
                           P<float>(logits), pdl, pdx, P<float>(stats), has_work ? P<float>(*work) : nullptr,
                           defer_stats ? 1 : 0, db};
  hip_ok(mnistx::ce_tail(a, cur_stream(), eps, mx.labels2, mx.lam, ds.on ? &ds.d : nullptr), "ce_tail");
}

// The dropout arguments of a binding, validated (ValueError): the drop rate p (finite, 0 <= p < 1) as
// the 16-bit keep threshold thr = clamp(floor((1 - p) * 65536 + 0.5), 1, 65535) and inv_keep =
// float(65536 / thr); the seed (0 <= seed < 2^63: a Python int beyond int64 fails the conversion
// first); the layer id, which shares a counter word with the draw group (dropout_rng.h).
struct DropArgs {
  uint32_t thr;
  float inv_keep;
};
DropArgs dropout_rate(double p, const char* op) {
  TORCH_CHECK_VALUE(std::isfinite(p) && p >= 0.0 && p < 1.0, op, ": dropout must be finite with 0 <= dropout < 1, got ",
                    p);
  const double t = std::min(std::max(std::floor((1.0 - p) * 65536.0 + 0.5), 1.0), 65535.0);
  return DropArgs{(uint32_t)t, (float)(65536.0 / t)};
}
const int64_t* dropout_key(const Tensor& step, int64_t seed, int64_t layer, const char* op) {
  TORCH_CHECK_VALUE(seed >= 0, op, ": dropout seed must be >= 0 and below 2^63, got ", seed);
  TORCH_CHECK_VALUE(layer >= 0 && layer < mnistx::DROP_MAX_LAYER, op, ": dropout layer id must be in [0, 65536), got ",
                    layer);
  check(step, at::kLong, 1, "step");
  return P<const int64_t>(step);
}

void mlp_head(Tensor x, Tensor w3t, Tensor b3, int64_t n1, Tensor w4t, Tensor b4, int64_t n2, Tensor w5t, Tensor b5,
              int64_t nc, Tensor labels, int64_t nb, double scale, Tensor h3, Tensor h4, Tensor logits,
              optional<Tensor> dl, optional<Tensor> dh4, optional<Tensor> dh3, optional<Tensor> dx, Tensor stats,
              optional<Tensor> work, bool defer_stats, optional<Tensor> dbias, double label_smoothing, double dropout,
              optional<Tensor> drop_step, int64_t drop_seed, int64_t drop_layer3, int64_t drop_layer4,
              optional<Tensor> labels2, optional<Tensor> lam, optional<Tensor> teacher_logits, int64_t teacher_ld,
              double distill_alpha, double distill_temperature) {
  const float eps = smoothing_arg(label_smoothing, "mlp_head");
  const MixArgs mx = mix_args(labels2, lam, nb, &labels, "mlp_head");
  const DropArgs da = dropout_rate(dropout, "mlp_head");
  const DistillArgs ds = distill_args(teacher_logits, teacher_ld, distill_alpha, distill_temperature, nb, nc, x, eps,
                                      mx.labels2 != nullptr, dropout != 0.0, "mlp_head");
  TORCH_CHECK_VALUE(!ds.on || has(dl), "mlp_head: teacher_logits is a training quantity and needs dl");
  mnistx::HeadDrop hd{};
  if (dropout != 0.0) {   // 0 launches what is launched without the key
    TORCH_CHECK_VALUE(has(drop_step), "mlp_head: dropout needs drop_step");
    hd.step = dropout_key(*drop_step, drop_seed, drop_layer3, "mlp_head");
    dropout_key(*drop_step, drop_seed, drop_layer4, "mlp_head");
    hd.seed = (uint64_t)drop_seed;
    hd.layer3 = (int)drop_layer3;
    hd.layer4 = (int)drop_layer4;
    hd.thr = da.thr;
    hd.inv_keep = da.inv_keep;
  }
  TORCH_CHECK(mnistx::mlp_head_supported(400, 120, 88, 16, (int)n1, (int)n2, (int)nc, (int)std::max<int64_t>(nb, 1)),
              "mlp_head: unsupported geometry");
  check(x, at::kBFloat16, nb * 400, "x");
  check(w3t, at::kBFloat16, 128 * 416, "w3t");
  check(w4t, at::kBFloat16, 96 * 128, "w4t");
  check(w5t, at::kBFloat16, 16 * 96, "w5t");
  check(b3, at::kFloat, n1, "b3");
  check(b4, at::kFloat, n2, "b4");
  check(b5, at::kFloat, nc, "b5");
  check(labels, at::kInt, nb, "labels");
  check(h3, at::kBFloat16, nb * 120, "h3");
  check(h4, at::kBFloat16, nb * 88, "h4");
  check(logits, at::kFloat, nb * 16, "logits");
  check(stats, at::kFloat, 8, "stats");
  const bool has_work = has(work);   // none: order-dependent atomics
  if (has_work) check(*work, at::kFloat, mnistx::CE_WORK_FLOATS, "work");
  for (const Tensor* t : {&x, &w3t, &w4t, &w5t, &h3, &h4, &logits})
    TORCH_CHECK(aligned(*t, 16), "mlp_head: operands must be 16-byte aligned");
  mnistx::bf16_t *pdl = nullptr, *pdh4 = nullptr, *pdh3 = nullptr, *pdx = nullptr;
  if (has(dl)) {
    TORCH_CHECK(dh4.has_value() && dh3.has_value() && dx.has_value(), "mlp_head: dl needs dh4, dh3, dx");
    check(*dl, at::kBFloat16, nb * 16, "dl");
    check(*dh4, at::kBFloat16, nb * 88, "dh4");
    check(*dh3, at::kBFloat16, nb * 120, "dh3");
    check(*dx, at::kBFloat16, nb * 400, "dx");
    for (const Tensor* t : {&*dl, &*dh4, &*dh3, &*dx})
      TORCH_CHECK(aligned(*t, 8), "mlp_head: gradients must be 8-byte aligned");
    pdl = BFm(*dl);
    pdh4 = BFm(*dh4);
    pdh3 = BFm(*dh3);
    pdx = BFm(*dx);
  }
  float* db = nullptr;
  if (has(dbias)) {
    TORCH_CHECK(pdl != nullptr, "mlp_head: dbias needs dl");
    check(*dbias, at::kFloat, (int64_t)mnistx::mlp_head_blocks((int)nb) * 16, "dbias");
    db = P<float>(*dbias);
  }
  TORCH_CHECK(eps == 0.f || pdl != nullptr, "mlp_head: label_smoothing is a training quantity and needs dl");
  TORCH_CHECK(hd.step == nullptr || pdl != nullptr, "mlp_head: dropout is a training quantity and needs dl");
  TORCH_CHECK(mx.labels2 == nullptr || pdl != nullptr, "mlp_head: labels2 / lam are training quantities and need dl");
  const mnistx::HeadArgs a{BF(x), BF(w3t), P<const float>(b3), (int)n1, BF(w4t), P<const float>(b4), (int)n2, BF(w5t),
                           P<const float>(b5), (int)nc, P<const int32_t>(labels), (int)nb, (float)scale, BFm(h3),
                           BFm(h4), P<float>(logits), pdl, pdh4, pdh3, pdx, P<float>(stats),
                           has_work ? P<float>(*work) : nullptr, (defer_stats && has_work) ? 1 : 0, db};
  hip_ok(mnistx::mlp_head(a, cur_stream(), eps, hd.step ? &hd : nullptr, mx.labels2, mx.lam, ds.on ? &ds.d : nullptr),
         "mlp_head");
}

// stand-alone dropout (dropout.hip), in place on x [nb, ld] bf16 with n real columns
void dropout_apply(bool bwd, Tensor x, int64_t nb, int64_t n, int64_t ld, Tensor step, int64_t seed, int64_t layer,
                   double p) {
  const char* op = bwd ? "dropout_bwd" : "dropout_fwd";
  const DropArgs da = dropout_rate(p, op);
  const int64_t* st = dropout_key(step, seed, layer, op);
  TORCH_CHECK_VALUE(nb >= 0 && nb < ((int64_t)1 << 31), op, ": nb must be in [0, 2^31), got ", nb);
  TORCH_CHECK_VALUE(n >= 0 && n <= mnistx::DROP_MAX_N, op, ": n must be in [0, 524288], got ", n);
  TORCH_CHECK_VALUE(ld >= n && ld % 8 == 0, op, ": ld must be a multiple of 8 and >= n, got ", ld);
  check(x, at::kBFloat16, nb * ld, bwd ? "dy" : "x");   // whole padded rows (16-byte chunks)
  TORCH_CHECK(aligned(x, 16), op, ": the buffer must be 16-byte aligned");
  TORCH_CHECK(step.device() == x.device(), op, ": step and the buffer must be on one device");
  if (p == 0.0) return;   // rate 0 keeps everything: nothing is launched
  hip_ok((bwd ? mnistx::dropout_bwd : mnistx::dropout_fwd)(BFm(x), nb, (int)n, (int)ld, st, (uint64_t)seed, (int)layer,
                                                          da.thr, da.inv_keep, cur_stream()),
         op);
}
void dropout_fwd(Tensor x, int64_t nb, int64_t n, int64_t ld, Tensor step, int64_t seed, int64_t layer, double p) {
  dropout_apply(false, x, nb, n, ld, step, seed, layer, p);
}
void dropout_bwd(Tensor dy, int64_t nb, int64_t n, int64_t ld, Tensor step, int64_t seed, int64_t layer, double p) {
  dropout_apply(true, dy, nb, n, ld, step, seed, layer, p);
}
// the keep bits of (seed, step, layer) as uint8 [nb, n]
void dropout_mask(Tensor out, int64_t nb, int64_t n, Tensor step, int64_t seed, int64_t layer, double p) {
  const DropArgs da = dropout_rate(p, "dropout_mask");
  const int64_t* st = dropout_key(step, seed, layer, "dropout_mask");
  TORCH_CHECK_VALUE(nb >= 0 && nb < ((int64_t)1 << 31), "dropout_mask: nb must be in [0, 2^31), got ", nb);
  TORCH_CHECK_VALUE(n >= 0 && n <= mnistx::DROP_MAX_N, "dropout_mask: n must be in [0, 524288], got ", n);
  check(out, at::kByte, nb * n, "out");
  TORCH_CHECK(step.device() == out.device(), "dropout_mask: step and out must be on one device");
  hip_ok(mnistx::dropout_mask(P<uint8_t>(out), nb, (int)n, st, (uint64_t)seed, (int)layer, da.thr, cur_stream()),
         "dropout_mask");
}

// the fp32 path's softmax-CE, beside the label-smoothing and distillation checks it shares with the bf16 one
void f32_softmax_ce(Tensor logits, int64_t ldl, optional<Tensor> labels, int64_t B, int64_t NC, double scale,
                    optional<Tensor> dlogits, int64_t ldd, optional<Tensor> stats, optional<Tensor> probs,
                    optional<Tensor> work, double label_smoothing, optional<Tensor> teacher_logits, int64_t teacher_ld,
                    double distill_alpha, double distill_temperature) {
  const float eps = smoothing_arg(label_smoothing, "f32_softmax_ce");
  const DistillArgs ds = distill_args(teacher_logits, teacher_ld, distill_alpha, distill_temperature, B, NC, logits, eps,
                                      false, false, "f32_softmax_ce");
  TORCH_CHECK_VALUE(!ds.on || has(labels), "f32_softmax_ce: teacher_logits needs labels");
  TORCH_CHECK(ldl >= NC, "ldl < NC");
  check(logits, at::kFloat, span(B, ldl, NC), "logits");
  const int32_t* lab = nullptr;
  if (has(labels)) {
    check(*labels, at::kInt, B, "labels");
    lab = P<const int32_t>(*labels);
  }
  float* dl = nullptr;
  if (has(dlogits)) {
    TORCH_CHECK(lab != nullptr && ldd >= NC, "dlogits needs labels and ldd >= NC");
    check(*dlogits, at::kFloat, B * ldd, "dlogits");
    dl = P<float>(*dlogits);
  }
  float* st = nullptr;
  if (has(stats)) {
    check(*stats, at::kFloat, 8, "stats");
    st = P<float>(*stats);
  }
  float* pr = nullptr;
  if (has(probs)) {
    check(*probs, at::kFloat, B * NC, "probs");
    pr = P<float>(*probs);
  }
  float* wk = nullptr;
  if (has(work)) {
    check(*work, at::kFloat, mnistx::CE_WORK_FLOATS, "work");
    wk = P<float>(*work);
  }
  TORCH_CHECK(eps == 0.f || lab != nullptr, "f32_softmax_ce: label_smoothing needs labels");
  hip_ok(mnistx::f32_softmax_ce(P<const float>(logits), (int)ldl, lab, (int)B, (int)NC, (float)scale, dl, (int)ldd,
                                st, pr, wk, cur_stream(), eps, ds.on ? &ds.d : nullptr),
         "f32_softmax_ce");
}

}  // namespace

void bind_loss(py::module_& m) {
  m.def("softmax_ce", &softmax_ce, py::arg("logits"), py::arg("ldl"), py::arg("labels"), py::arg("B"), py::arg("NC"),
        py::arg("scale"), py::arg("dlogits"), py::arg("ldd"), py::arg("stats"), py::arg("probs"),
        py::arg("work") = py::none(), py::arg("defer_stats") = false, py::arg("dbias") = py::none(),
        py::arg("label_smoothing") = 0.0, py::arg("labels2") = py::none(), py::arg("lam") = py::none(), py::arg("teacher_logits") = py::none(), py::arg("teacher_ld") = 0,
        py::arg("distill_alpha") = 0.0, py::arg("distill_temperature") = 1.0);
  m.def("softmax_ce_dbias_blocks",
        [](int64_t B, int64_t ldl) { return (int64_t)mnistx::softmax_ce_dbias_blocks((int)B, (int)ldl); });
  m.def("mlp_head_supported", &mlp_head_supported);
  m.def("mlp_head_blocks", [](int64_t nb) { return (int64_t)mnistx::mlp_head_blocks((int)nb); });
  m.def("ce_tail_supported", &ce_tail_supported);
  m.def("ce_tail_blocks", [](int64_t nb) { return (int64_t)mnistx::ce_tail_blocks((int)nb); });
  m.def("ce_tail", &ce_tail, py::arg("x"), py::arg("w5t"), py::arg("b5"), py::arg("nc"), py::arg("labels"),
        py::arg("nb"), py::arg("scale"), py::arg("logits"), py::arg("dl") = py::none(), py::arg("dx") = py::none(),
        py::arg("stats"), py::arg("work") = py::none(), py::arg("defer_stats") = false, py::arg("dbias") = py::none(),
        py::arg("label_smoothing") = 0.0, py::arg("labels2") = py::none(), py::arg("lam") = py::none(), py::arg("teacher_logits") = py::none(), py::arg("teacher_ld") = 0,
        py::arg("distill_alpha") = 0.0, py::arg("distill_temperature") = 1.0);
  m.def("mlp_head", &mlp_head, py::arg("x"), py::arg("w3t"), py::arg("b3"), py::arg("n1"), py::arg("w4t"),
        py::arg("b4"), py::arg("n2"), py::arg("w5t"), py::arg("b5"), py::arg("nc"), py::arg("labels"), py::arg("nb"),
        py::arg("scale"), py::arg("h3"), py::arg("h4"), py::arg("logits"), py::arg("dl") = py::none(),
        py::arg("dh4") = py::none(), py::arg("dh3") = py::none(), py::arg("dx") = py::none(), py::arg("stats"),
        py::arg("work"), py::arg("defer_stats") = false, py::arg("dbias") = py::none(),
        py::arg("label_smoothing") = 0.0, py::arg("dropout") = 0.0, py::arg("drop_step") = py::none(),
        py::arg("drop_seed") = 0, py::arg("drop_layer3") = 0, py::arg("drop_layer4") = 0,
        py::arg("labels2") = py::none(), py::arg("lam") = py::none(), py::arg("teacher_logits") = py::none(), py::arg("teacher_ld") = 0,
        py::arg("distill_alpha") = 0.0, py::arg("distill_temperature") = 1.0);
  m.def("dropout_fwd", &dropout_fwd, py::arg("x"), py::arg("nb"), py::arg("n"), py::arg("ld"), py::arg("step"),
        py::arg("seed"), py::arg("layer"), py::arg("p"));
  m.def("dropout_bwd", &dropout_bwd, py::arg("dy"), py::arg("nb"), py::arg("n"), py::arg("ld"), py::arg("step"),
        py::arg("seed"), py::arg("layer"), py::arg("p"));
  m.def("dropout_mask", &dropout_mask, py::arg("out"), py::arg("nb"), py::arg("n"), py::arg("step"), py::arg("seed"),
        py::arg("layer"), py::arg("p"));
  m.def("f32_softmax_ce", &f32_softmax_ce, py::arg("logits"), py::arg("ldl"), py::arg("labels"), py::arg("B"),
        py::arg("NC"), py::arg("scale"), py::arg("dlogits"), py::arg("ldd"), py::arg("stats"), py::arg("probs"),
        py::arg("work") = py::none(), py::arg("label_smoothing") = 0.0, py::arg("teacher_logits") = py::none(), py::arg("teacher_ld") = 0,
        py::arg("distill_alpha") = 0.0, py::arg("distill_temperature") = 1.0);
}
