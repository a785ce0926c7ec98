// _kernels bindings: fused conv + pool, the LeNet band kernels, the reference conv1 weight gradient.
#include "bind/common.h"

namespace {

struct CPGeo {
  int cfg, OH, OW, PH, PW, KM;
};

CPGeo cp_geo(int64_t cin, int64_t cout, int64_t ks, int64_t pad, int64_t h, int64_t w) {
  CPGeo g{};
  g.cfg = mnistx::convpool_config((int)cin, (int)cout, (int)ks, (int)pad, (int)h, (int)w);
  TORCH_CHECK(g.cfg >= 0, "convpool: unsupported geometry cin=", cin, " cout=", cout, " k=", ks, " pad=", pad,
              " ", h, "x", w);
  g.OH = (int)(h + 2 * pad - ks + 1);
  g.OW = (int)(w + 2 * pad - ks + 1);
  g.PH = g.OH / 2;
  g.PW = g.OW / 2;
  g.KM = mnistx::convpool_wgrad_rows(g.cfg);
  return g;
}

int64_t convpool_supported(int64_t cin, int64_t cout, int64_t ks, int64_t pad, int64_t h, int64_t w) {
  return mnistx::convpool_config((int)cin, (int)cout, (int)ks, (int)pad, (int)h, (int)w);
}

int64_t convpool_rows(int64_t cin, int64_t cout, int64_t ks, int64_t pad, int64_t h, int64_t w) {
  return cp_geo(cin, cout, ks, pad, h, w).KM;
}

// (G, Ipad, I, bias_row) arguments of splitk_reduce for this geometry's wgrad slab
std::vector<int64_t> convpool_reduce_args(int64_t cin, int64_t cout, int64_t ks, int64_t pad, int64_t h, int64_t w,
                                          int64_t cin_real) {
  auto g = cp_geo(cin, cout, ks, pad, h, w);
  int o[4];
  TORCH_CHECK(mnistx::convpool_reduce_layout(g.cfg, o) == 0, "convpool_reduce_args");
  return {o[0], o[1], o[2] < 0 ? cin_real : (int64_t)o[2], o[3]};
}

// Input of a fused conv: bf16 x, or the uint8 dataset + per-sample index (Cin == 1 geometries)
mnistx::XSrc cp_src(const Tensor& x, const optional<Tensor>& u8, const optional<Tensor>& idx, int cfg, int64_t B,
                    int64_t hwc) {
  mnistx::XSrc src{nullptr, nullptr, nullptr, 0};
  if (has(u8)) {
    TORCH_CHECK(mnistx::convpool_u8_input(cfg), "convpool: uint8 input only for first layers (Cin 1, or 3 at 28x28)");
    TORCH_CHECK(has(idx), "convpool: uint8 input needs idx");
    check(*u8, at::kByte, hwc, "u8");
    TORCH_CHECK(u8->numel() % hwc == 0 && u8->numel() < (int64_t)INT32_MAX,
                "u8: [n, H*W*C] images, < 2 GB (the kernels address it through one buffer resource)");
    TORCH_CHECK(aligned(*u8, 4), "u8 must be 4-byte aligned");
    check(*idx, at::kLong, B, "idx");
    src.u8 = P<const uint8_t>(*u8);
    src.idx = P<const int64_t>(*idx);
    src.n = (int)(u8->numel() / hwc);       // the kernel clamps every index into [0, n)
  } else if (has(idx)) {
    // x is the resident bf16 dataset [n, H*W*C] (normalised once), gathered through idx
    TORCH_CHECK(mnistx::convpool_u8_input(cfg), "convpool: dataset input only for first layers (Cin 1, or 3 at 28x28)");
    check(x, at::kBFloat16, hwc, "x (dataset)");
    TORCH_CHECK(x.numel() % hwc == 0 && x.numel() * 2 < (int64_t)INT32_MAX,
                "x (dataset): [n, H*W*C] bf16 images, < 2 GB (one buffer resource)");
    TORCH_CHECK(aligned(x, 8), "x (dataset) must be 8-byte aligned");
    check(*idx, at::kLong, B, "idx");
    src.x = BF(x);
    src.idx = P<const int64_t>(*idx);
    src.n = (int)(x.numel() / hwc);
  } else {
    check(x, at::kBFloat16, B * hwc, "x");
    src.x = BF(x);
  }
  return src;
}

void convpool_fwd(Tensor x, Tensor w, Tensor bias, int64_t bias_n, Tensor pooled, Tensor arg, int64_t B, int64_t cin,
                  int64_t cout, int64_t ks, int64_t pad, int64_t h, int64_t wd, optional<Tensor> u8,
                  optional<Tensor> idx, optional<Tensor> lrn_out, double lrn_bias, double lrn_alpha,
                  double lrn_beta, int64_t lrn_r) {
  auto g = cp_geo(cin, cout, ks, pad, h, wd);
  const auto src = cp_src(x, u8, idx, g.cfg, B, h * wd * cin);
  check(w, at::kBFloat16, ks * ks * cin * cout, "w");
  check(bias, at::kFloat, bias_n, "bias");
  check(pooled, at::kBFloat16, B * g.PH * g.PW * cout, "pooled");
  check(arg, at::kByte, B * g.PH * g.PW * mnistx::convpool_arg_bytes(g.cfg), "arg");
  if (has(lrn_out)) {
    // the following LRN (radius 4) written by the same launch (refc1n_fwd_k): reference conv1 only
    TORCH_CHECK(lrn_r == 4 && ((g.cfg == 2 && mnistx::refc1_fwd_lrn_ok()) ||
                               (g.cfg == 3 && mnistx::refc1_fwd3_ok() && !src.u8)),
                "convpool_fwd: lrn_out only for the reference conv1 (1 or 3 -> 32, SAME; 3 channels: bf16 input) "
                "with norm1 radius 4");
    check(*lrn_out, at::kBFloat16, B * g.PH * g.PW * cout, "lrn_out");
    hip_ok(mnistx::refc1_band_fwd(src, BF(w), P<const float>(bias), (int)bias_n, (int)B, BFm(pooled), P<uint8_t>(arg),
                                  cur_stream(), BFm(*lrn_out), (float)lrn_bias, (float)lrn_alpha, (float)lrn_beta,
                                  g.cfg == 3 ? 3 : 1),
           "convpool_fwd (+ norm1)");
    return;
  }
  hip_ok(mnistx::convpool_fwd(g.cfg, src, BF(w), P<const float>(bias), (int)bias_n, (int)B, BFm(pooled),
                              P<uint8_t>(arg), cur_stream()),
         "convpool_fwd");
}

void convpool_wgrad(Tensor x, Tensor dP, Tensor arg, Tensor slab, int64_t grid, int64_t B, int64_t cin, int64_t cout,
                    int64_t ks, int64_t pad, int64_t h, int64_t wd, optional<Tensor> u8, optional<Tensor> idx,
                    optional<Tensor> lrn_p, double lrn_bias, double lrn_alpha, double lrn_beta, int64_t lrn_r) {
  auto g = cp_geo(cin, cout, ks, pad, h, wd);
  TORCH_CHECK(grid >= 1 && grid <= 65535, "grid");
  const int64_t np = B * g.PH * g.PW * cout;
  const auto src = cp_src(x, u8, idx, g.cfg, B, h * wd * cin);
  check(dP, at::kBFloat16, np, "dP");
  check(arg, at::kByte, B * g.PH * g.PW * mnistx::convpool_arg_bytes(g.cfg), "arg");
  check(slab, at::kFloat, grid * g.KM * cout, "slab");
  const mnistx::bf16_t* lp = nullptr;
  if (has(lrn_p)) {
    TORCH_CHECK(lrn_r == 4 && cout == 32 && (g.cfg == 2 || g.cfg == 3), "LRN fold: reference conv1 (Cout 32), radius 4");
    check(*lrn_p, at::kBFloat16, np, "lrn_p");
    lp = BF(*lrn_p);
  }
  hip_ok(mnistx::convpool_wgrad(g.cfg, src, BF(dP), P<const uint8_t>(arg), (int)B, P<float>(slab), (int)grid,
                                cur_stream(), lp, (float)lrn_bias, (float)lrn_alpha, (float)lrn_beta),
         "convpool_wgrad");
}

bool convpool_u8_input(int64_t cin, int64_t cout, int64_t ks, int64_t pad, int64_t h, int64_t w) {
  return mnistx::convpool_u8_input(cp_geo(cin, cout, ks, pad, h, w).cfg) != 0;
}

int64_t convpool_wgrad_grid(int64_t cin, int64_t cout, int64_t ks, int64_t pad, int64_t h, int64_t w) {
  const int n = mnistx::convpool_wgrad_grid(cp_geo(cin, cout, ks, pad, h, w).cfg);
  TORCH_CHECK(n > 0, "convpool_wgrad_grid: occupancy query failed");
  return n;
}

int64_t convpool_arg_bytes(int64_t cin, int64_t cout, int64_t ks, int64_t pad, int64_t h, int64_t w) {
  return mnistx::convpool_arg_bytes(cp_geo(cin, cout, ks, pad, h, w).cfg);
}

bool convpool_has_dgrad(int64_t cin, int64_t cout, int64_t ks, int64_t pad, int64_t h, int64_t w) {
  return mnistx::convpool_has_dgrad(cp_geo(cin, cout, ks, pad, h, w).cfg) != 0;
}

void convpool_dgrad(Tensor dP, Tensor arg, Tensor w, Tensor dx, int64_t B, int64_t cin, int64_t cout, int64_t ks,
                    int64_t pad, int64_t h, int64_t wd, int64_t grid_cap) {
  auto g = cp_geo(cin, cout, ks, pad, h, wd);
  TORCH_CHECK(mnistx::convpool_has_dgrad(g.cfg), "convpool_dgrad: no fused dgrad for this geometry");
  const int64_t np = B * g.PH * g.PW * cout;
  check(dP, at::kBFloat16, np, "dP");
  check(arg, at::kByte, B * g.PH * g.PW * mnistx::convpool_arg_bytes(g.cfg), "arg");
  check(w, at::kBFloat16, ks * ks * cin * cout, "w");
  check(dx, at::kBFloat16, B * h * wd * cin, "dx");
  hip_ok(mnistx::convpool_dgrad(g.cfg, BF(dP), P<const uint8_t>(arg), BF(w), (int)B, BFm(dx), (int)grid_cap,
                                cur_stream()),
         "convpool_dgrad");
}

// The input of the LeNet band kernels: x uint8 or bf16 images [n, 784], gathered through idx or
// the batch itself (idx None); bf16 rows aligned to bf_align bytes
mnistx::XSrc lenet_src(const Tensor& x, const optional<Tensor>& idx, int64_t B, int bf_align) {
  mnistx::XSrc src{nullptr, nullptr, nullptr, 0};
  if (x.scalar_type() == at::kByte) {   // uint8 images, normalised x/255 - 0.5 in the kernel
    check(x, at::kByte, 784, "x");
    TORCH_CHECK(x.numel() % 784 == 0 && x.numel() < (int64_t)INT32_MAX, "x: [n, 784] uint8 images, < 2 GB");
    TORCH_CHECK(aligned(x, 4), "x must be 4-byte aligned");
    src.u8 = P<const uint8_t>(x);
  } else {
    check(x, at::kBFloat16, 784, "x");
    TORCH_CHECK(x.numel() % 784 == 0 && x.numel() * 2 < (int64_t)INT32_MAX, "x: [n, 784] bf16 images, < 2 GB");
    TORCH_CHECK(aligned(x, bf_align), "x must be ", bf_align, "-byte aligned");
    src.x = BF(x);
  }
  src.n = (int)(x.numel() / 784);
  if (has(idx)) {
    check(*idx, at::kLong, B, "idx");
    src.idx = P<const int64_t>(*idx);
  } else {
    TORCH_CHECK(src.n >= B, "x: needs B images without idx");
  }
  return src;
}

// LeNet-5 conv1+pool1+conv2+pool2 forward on banded MFMA tiles (lenet_band.hip).
// x: bf16 images [n, 784] gathered through idx, or the batch itself [B, 784] (idx None).
void lenet_band_fwd(Tensor x, Tensor w1, Tensor b1, int64_t b1n, Tensor w2, Tensor b2, int64_t B, Tensor p2,
                    Tensor arg2, optional<Tensor> p1, optional<Tensor> arg1, optional<Tensor> idx,
                    optional<Tensor> prof) {
  const mnistx::XSrc src = lenet_src(x, idx, B, 16);
  check(w1, at::kBFloat16, 5 * 5 * 8, "w1");
  check(b1, at::kFloat, b1n, "b1");
  TORCH_CHECK(b1n >= 0 && b1n <= 8, "b1n");
  check(w2, at::kBFloat16, 5 * 5 * 8 * 16, "w2");
  check(b2, at::kFloat, 16, "b2");
  TORCH_CHECK(aligned(w1, 16) && aligned(w2, 16), "w1 / w2 must be 16-byte aligned");
  check(p2, at::kBFloat16, B * 400, "p2");
  check(arg2, at::kByte, B * 400, "arg2");
  mnistx::bf16_t* pp1 = nullptr;
  uint8_t* pa1 = nullptr;
  if (has(p1)) {   // with arg1: the convpool layouts; without: combined records
    check(*p1, at::kBFloat16, B * 14 * 14 * 8, "p1");
    TORCH_CHECK(aligned(*p1, 16), "p1 must be 16-byte aligned");
    pp1 = BFm(*p1);
    if (has(arg1)) {
      check(*arg1, at::kByte, B * 14 * 14 * 4, "arg1");
      pa1 = P<uint8_t>(*arg1);
    }
  }
  unsigned long long* pr = nullptr;
  if (has(prof)) {   // experiments: int64[4] clock sums
    check(*prof, at::kLong, 4, "prof");
    pr = P<unsigned long long>(*prof);
  }
  hip_ok(mnistx::lenet_band_fwd(src, BF(w1), P<const float>(b1), (int)b1n, BF(w2), P<const float>(b2), (int)B, pp1,
                                pa1, BFm(p2), P<uint8_t>(arg2), cur_stream(), pr),
         "lenet_band_fwd");
}

// LeNet-5 conv-stack backward as one kernel (lenet_bwd.hip): conv2 dgrad + both weight
// gradients; x as for lenet_band_fwd (the forward's input), p1c (the combined pool1 records:
// lenet_band_fwd with p1 and no arg1) / arg2 from it, dp2 = dL/d pool2 [B, 400].
// slab1 [grid, 32, 8], slab2 [grid, 208, 16] (split-K partials).
void lenet_bwd(Tensor x, Tensor p1, Tensor dp2, Tensor arg2, Tensor w2, int64_t B, Tensor slab1, Tensor slab2,
               int64_t grid, optional<Tensor> idx, optional<Tensor> prof) {
  const mnistx::XSrc src = lenet_src(x, idx, B, 8);
  TORCH_CHECK(B >= 1 && B * 196 * 16 < (int64_t)INT32_MAX, "B");
  check(p1, at::kBFloat16, B * 196 * 8, "p1");
  check(dp2, at::kBFloat16, B * 400, "dp2");
  check(arg2, at::kByte, B * 400, "arg2");
  check(w2, at::kBFloat16, 5 * 5 * 8 * 16, "w2");
  for (const Tensor* t : {&p1, &dp2, &w2})
    TORCH_CHECK(aligned(*t, 16), "p1 / dp2 / w2 must be 16-byte aligned");
  TORCH_CHECK(aligned(arg2, 8), "arg2 alignment");
  const int res = mnistx::lenet_bwd_blocks((int)B);
  TORCH_CHECK(res > 0, "lenet_bwd: occupancy query failed");
  TORCH_CHECK(grid >= 1 && grid <= res, "lenet_bwd: grid must be in [1, ", res, "] (one block per CU, <= tiles)");
  check(slab1, at::kFloat, grid * 32 * 8, "slab1");
  check(slab2, at::kFloat, grid * 208 * 16, "slab2");
  unsigned long long* pr = nullptr;
  if (has(prof)) {
    const char* pw = getenv("MNISTX_BWD_PROF_WAVES");
    check(*prof, at::kLong, (pw && pw[0] == '1') ? 8 + 16 * 8 : 8, "prof");
    pr = P<unsigned long long>(*prof);
  }
  hip_ok(mnistx::lenet_bwd(src, BF(p1), BF(dp2), P<const uint8_t>(arg2), BF(w2), (int)B, P<float>(slab1),
                           P<float>(slab2), (int)grid, cur_stream(), pr),
         "lenet_bwd");
}

// Reference-CNN conv1 weight gradient with the norm1 backward folded in (refc1_wgrad.hip).
// x / u8 / idx as for convpool_wgrad (cfg RefC1g); dn = dL/d norm1, p1 = pool1, arg = pool1 codes.
void refc1_wgrad(Tensor x, Tensor dn, Tensor p1, Tensor arg, Tensor slab, int64_t grid, int64_t B, double lrn_bias,
                 double lrn_alpha, double lrn_beta, optional<Tensor> u8, optional<Tensor> idx, int64_t cin) {
  TORCH_CHECK(cin == 1 || cin == 3, "refc1_wgrad: 1 or 3 input channels");
  const int cfg = mnistx::convpool_config((int)cin, 32, 5, 2, 28, 28);
  TORCH_CHECK(cfg >= 0, "refc1_wgrad: no RefC1 geometry");
  TORCH_CHECK(B >= 1 && B * 784 * cin * 2 < (int64_t)INT32_MAX, "B: the batch (and its index) must stay < 2 GB");
  TORCH_CHECK(cin == 1 || !has(u8), "refc1_wgrad: 3 channels read bf16 (the batch, or the dataset through idx) only");
  const auto src = cp_src(x, u8, idx, cfg, B, 784 * cin);
  if (src.x) TORCH_CHECK(aligned(src.x, 8), "x must be 8-byte aligned");
  const int64_t np = B * 196 * 32;
  check(dn, at::kBFloat16, np, "dn");
  check(p1, at::kBFloat16, np, "p1");
  check(arg, at::kByte, np, "arg");
  for (const Tensor* t : {&dn, &p1})
    TORCH_CHECK(aligned(*t, 16), "dn / p1 must be 16-byte aligned");
  TORCH_CHECK(aligned(arg, 8), "arg must be 8-byte aligned");
  TORCH_CHECK(lrn_beta == 0.75, "refc1_wgrad: LRN beta 0.75 only");
  const int res = mnistx::refc1_wgrad_blocks((int)B);
  TORCH_CHECK(res > 0, "refc1_wgrad: occupancy query failed");
  TORCH_CHECK(grid >= 1 && grid <= res, "refc1_wgrad: grid must be in [1, ", res, "] (one block per CU, <= tiles)");
  check(slab, at::kFloat, grid * (cin == 1 ? 48 : 80) * 32, "slab");
  hip_ok(mnistx::refc1_wgrad(src, BF(dn), BF(p1), P<const uint8_t>(arg), (int)B, (float)lrn_bias, (float)lrn_alpha,
                             (float)lrn_beta, P<float>(slab), (int)grid, cur_stream(), (int)cin),
         "refc1_wgrad");
}

}  // namespace

void bind_fused_conv(py::module_& m) {
  m.def("convpool_supported", &convpool_supported);
  m.def("convpool_rows", &convpool_rows);
  m.def("convpool_reduce_args", &convpool_reduce_args);
  m.def("convpool_fwd", &convpool_fwd, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("bias_n"),
        py::arg("pooled"), py::arg("arg"), py::arg("B"), py::arg("cin"), py::arg("cout"), py::arg("ks"),
        py::arg("pad"), py::arg("h"), py::arg("w_"), py::arg("u8") = py::none(), py::arg("idx") = py::none(),
        py::arg("lrn_out") = py::none(), py::arg("lrn_bias") = 0.0, py::arg("lrn_alpha") = 0.0,
        py::arg("lrn_beta") = 0.0, py::arg("lrn_r") = 0);
  // u8: the forward reads a uint8 dataset (3 channels: the fold needs bf16 input)
  m.def("convpool_fwd_lrn_ok", [](int64_t cin, int64_t cout, int64_t ks, int64_t pad, int64_t h, int64_t w, bool u8) {
    const int cfg = cp_geo(cin, cout, ks, pad, h, w).cfg;
    return (cfg == 2 && mnistx::refc1_fwd_lrn_ok()) || (cfg == 3 && !u8 && mnistx::refc1_fwd3_ok());
  }, py::arg("cin"), py::arg("cout"), py::arg("ks"), py::arg("pad"), py::arg("h"), py::arg("w"), py::arg("u8") = false);
  m.def("convpool_wgrad", &convpool_wgrad, py::arg("x"), py::arg("dP"), py::arg("arg"), py::arg("slab"),
        py::arg("grid"), py::arg("B"), py::arg("cin"), py::arg("cout"), py::arg("ks"), py::arg("pad"), py::arg("h"),
        py::arg("w_"), py::arg("u8") = py::none(), py::arg("idx") = py::none(), py::arg("lrn_p") = py::none(),
        py::arg("lrn_bias") = 0.0, py::arg("lrn_alpha") = 0.0, py::arg("lrn_beta") = 0.0, py::arg("lrn_r") = 0);
  m.def("convpool_u8_input", &convpool_u8_input);
  m.def("convpool_wgrad_grid", &convpool_wgrad_grid);
  m.def("convpool_arg_bytes", &convpool_arg_bytes);
  m.def("convpool_has_dgrad", &convpool_has_dgrad);
  m.def("convpool_dgrad", &convpool_dgrad, py::arg("dP"), py::arg("arg"), py::arg("w"), py::arg("dx"), py::arg("B"),
        py::arg("cin"), py::arg("cout"), py::arg("ks"), py::arg("pad"), py::arg("h"), py::arg("w_"),
        py::arg("grid_cap") = 0);
  m.def("lenet_band_fwd", &lenet_band_fwd, py::arg("x"), py::arg("w1"), py::arg("b1"), py::arg("b1n"),
        py::arg("w2"), py::arg("b2"), py::arg("B"), py::arg("p2"), py::arg("arg2"), py::arg("p1") = py::none(),
        py::arg("arg1") = py::none(), py::arg("idx") = py::none(), py::arg("prof") = py::none());
  m.def("lenet_bwd", &lenet_bwd, py::arg("x"), py::arg("p1"), py::arg("dp2"), py::arg("arg2"),
        py::arg("w2"), py::arg("B"), py::arg("slab1"), py::arg("slab2"), py::arg("grid"), py::arg("idx") = py::none(),
        py::arg("prof") = py::none());
  m.def("lenet_bwd_blocks", [](int64_t B) {
    const int n = mnistx::lenet_bwd_blocks((int)B);
    TORCH_CHECK(n > 0, "lenet_bwd_blocks: occupancy query failed");
    return (int64_t)n;
  });
  m.def("refc1_wgrad", &refc1_wgrad, py::arg("x"), py::arg("dn"), py::arg("p1"), py::arg("arg"), py::arg("slab"),
        py::arg("grid"), py::arg("B"), py::arg("lrn_bias"), py::arg("lrn_alpha"), py::arg("lrn_beta"),
        py::arg("u8") = py::none(), py::arg("idx") = py::none(), py::arg("cin") = 1);
  m.def("refc1_set_skip", [](int64_t s) { mnistx::refc1_set_skip((int)s); });
  m.def("refc1_set_fwd_variant", [](int64_t v) { mnistx::refc1_set_fwd_variant((int)v); });
  m.def("refc1_wgrad_blocks", [](int64_t B) {
    const int n = mnistx::refc1_wgrad_blocks((int)B);
    TORCH_CHECK(n > 0, "refc1_wgrad_blocks: occupancy query failed");
    return (int64_t)n;
  });
}
