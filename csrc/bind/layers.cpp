// _kernels bindings: dense / conv GEMMs, pooling, LRN, and the GEMM / halo switches.
#include "bind/common.h"

namespace {

mnistx::GemmEpi make_epi(const Tensor& out, int64_t M, int64_t N, int64_t ldc, const optional<Tensor>& bias,
                         int64_t bias_n, bool relu, const optional<Tensor>& mask, int64_t ldm) {
  TORCH_CHECK(ldc >= N, "ldc < N");
  mnistx::GemmEpi ep{};
  if (out.scalar_type() == at::kBFloat16) {
    check(out, at::kBFloat16, span(M, ldc, N), "out");
    ep.mode = mnistx::EPI_BF16;
  } else {
    check(out, at::kFloat, span(M, ldc, N), "out");
    ep.mode = mnistx::EPI_F32;
  }
  ep.out = out.data_ptr();
  ep.ldc = (int)ldc;
  ep.bias = nullptr;
  ep.bias_n = 0;
  if (has(bias)) {
    check(*bias, at::kFloat, bias_n, "bias");
    ep.bias = P<const float>(*bias);
    ep.bias_n = (int)bias_n;
  }
  ep.relu = relu ? 1 : 0;
  ep.mask = nullptr;
  ep.ldm = 0;
  if (has(mask)) {
    TORCH_CHECK(ldm >= N, "ldm < N");
    check(*mask, at::kBFloat16, span(M, ldm, N), "mask");
    ep.mask = BF(*mask);
    ep.ldm = (int)ldm;
  }
  ep.slab_stride = 0;
  return ep;
}

mnistx::GemmEpi make_slab(const Tensor& slab, int64_t splits, int64_t M, int64_t N) {
  check(slab, at::kFloat, splits * M * N, "slab");
  mnistx::GemmEpi ep{};
  ep.out = slab.data_ptr();
  ep.ldc = (int)N;
  ep.mode = mnistx::EPI_SLAB;
  ep.slab_stride = M * N;
  return ep;
}

// Effective split count the launcher will use (kchunk rounded to BK=32).
// split-K count the weight-gradient launch really uses: chunks round up to its
// K step (gemm.hip BK_WG = 32)
int64_t eff_splits(int64_t K, int64_t splits) {
  if (splits < 1) splits = 1;
  int64_t kchunk = (K + splits - 1) / splits;
  kchunk = ((kchunk + 31) / 32) * 32;
  if (kchunk < 32) kchunk = 32;
  return (K + kchunk - 1) / kchunk;
}

void dense_fwd(Tensor x, Tensor w, Tensor out, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldw,
               int64_t ldc, optional<Tensor> bias, int64_t bias_n, bool relu, optional<Tensor> mask, int64_t ldm,
               int64_t tile) {
  check(x, at::kBFloat16, span(M, ldx, K), "x");
  check(w, at::kBFloat16, span(K, ldw, N), "w");
  TORCH_CHECK(ldx >= K && ldw >= N, "bad leading dims");
  auto ep = make_epi(out, M, N, ldc, bias, bias_n, relu, mask, ldm);
  hip_ok(mnistx::dense_fwd(BF(x), BF(w), (int)M, (int)N, (int)K, (int)ldx, (int)ldw, ep, cur_stream(), (int)tile),
         "dense_fwd");
}

void dense_dgrad(Tensor dy, Tensor w, Tensor out, int64_t M, int64_t N, int64_t K, int64_t lddy, int64_t ldw,
                 int64_t ldc, optional<Tensor> mask, int64_t ldm, int64_t tile) {
  // out[M, N=Din] = dy[M, K=Dout] . W[Din, Dout]^T
  check(dy, at::kBFloat16, span(M, lddy, K), "dy");
  check(w, at::kBFloat16, span(N, ldw, K), "w");
  TORCH_CHECK(lddy >= K && ldw >= K, "bad leading dims");
  auto ep = make_epi(out, M, N, ldc, c10::nullopt, 0, false, mask, ldm);
  hip_ok(mnistx::dense_dgrad(BF(dy), BF(w), (int)M, (int)N, (int)K, (int)lddy, (int)ldw, ep, cur_stream(),
                             (int)tile),
         "dense_dgrad");
}

int64_t dense_wgrad(Tensor x, Tensor dy, Tensor slab, int64_t Din, int64_t Dout, int64_t B, int64_t ldx, int64_t lddy,
                    bool with_bias, int64_t splits, int64_t tile) {
  check(x, at::kBFloat16, span(B, ldx, Din), "x");
  check(dy, at::kBFloat16, span(B, lddy, Dout), "dy");
  TORCH_CHECK(ldx >= Din && lddy >= Dout, "bad leading dims");
  const int64_t M = Din + (with_bias ? 1 : 0);
  const int64_t S = eff_splits(B, splits);
  auto ep = make_slab(slab, S, M, Dout);
  int used = (int)S;
  hip_ok(mnistx::dense_wgrad(BF(x), BF(dy), (int)Din, (int)Dout, (int)B, (int)ldx, (int)lddy, with_bias ? 1 : 0,
                             (int)S, ep, cur_stream(), (int)tile, &used),
         "dense_wgrad");
  return used;   // the reduce sums exactly the partials written
}

// Split count the conv weight gradient prefers (slab sizing): the halo kernel's
// persistent grid when it covers the geometry, else -1 (use the GEMM rule).
int64_t conv_wgrad_pref_splits(int64_t Nb, int64_t H, int64_t W, int64_t C, int64_t OH, int64_t OW, int64_t KH,
                               int64_t KW, int64_t ph, int64_t pw, int64_t Cout, bool with_bias) {
  if (mnistx::conv_halo_enabled() &&
      mnistx::conv5_halo_wgrad_ok((int)H, (int)W, (int)C, (int)OH, (int)OW, (int)KH, (int)KW, (int)ph, (int)pw,
                                  (int)Cout, with_bias ? 1 : 0))
    return mnistx::conv5_halo_wgrad_grid((int)Nb);
  return -1;
}

// Grouped dense weight gradients (with bias rows) in one launch; returns the
// effective split counts.  Every problem must take the vector loader path
// (leading dims and widths multiples of 8): the executor checks dense_wgrad_group_ok.
std::vector<int64_t> dense_wgrad_group(std::vector<Tensor> x, std::vector<Tensor> dy, std::vector<Tensor> slab,
                                       std::vector<int64_t> Din, std::vector<int64_t> Dout, int64_t B,
                                       std::vector<int64_t> splits) {
  const size_t n = x.size();
  TORCH_CHECK(n >= 1 && n <= 4 && dy.size() == n && slab.size() == n && Din.size() == n && Dout.size() == n &&
                  splits.size() == n,
              "dense_wgrad_group: 1-4 problems, matching lists");
  const mnistx::bf16_t* xp[4];
  const mnistx::bf16_t* dp[4];
  int din[4], dout[4], ldx[4], lddy[4], sp[4];
  mnistx::GemmEpi ep[4];
  for (size_t p = 0; p < n; ++p) {
    TORCH_CHECK(x[p].dim() == 2 && dy[p].dim() == 2, "dense_wgrad_group: 2-D operands");
    const int64_t lx = x[p].size(1), ly = dy[p].size(1);
    TORCH_CHECK(Din[p] % 8 == 0 && Dout[p] % 8 == 0 && lx % 8 == 0 && ly % 8 == 0 && lx >= Din[p] && ly >= Dout[p],
                "dense_wgrad_group: widths must be multiples of 8");
    check(x[p], at::kBFloat16, span(B, lx, Din[p]), "x");
    check(dy[p], at::kBFloat16, span(B, ly, Dout[p]), "dy");
    const int64_t S = eff_splits(B, splits[p]);
    ep[p] = make_slab(slab[p], S, Din[p] + 1, Dout[p]);
    xp[p] = BF(x[p]);
    dp[p] = BF(dy[p]);
    din[p] = (int)Din[p];
    dout[p] = (int)Dout[p];
    ldx[p] = (int)lx;
    lddy[p] = (int)ly;
    sp[p] = (int)S;
  }
  hip_ok(mnistx::dense_wgrad_group((int)n, xp, dp, din, dout, (int)B, ldx, lddy, sp, ep, cur_stream()),
         "dense_wgrad_group");
  return std::vector<int64_t>(sp, sp + n);
}

mnistx::LrnParams lrn_params(int64_t lrn_r, double b, double a, double be) {
  TORCH_CHECK(lrn_r == 0 || lrn_r == 4, "LRN fold: depth_radius 4 only");
  return mnistx::LrnParams{(float)b, (float)a, (float)be, lrn_r == 4 ? 1 : 0};
}

void conv_fwd(Tensor x, Tensor w, Tensor out, int64_t Nb, int64_t H, int64_t W, int64_t C, int64_t OH, int64_t OW,
              int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t Cout, optional<Tensor> bias, int64_t bias_n,
              bool relu, int64_t lrn_r, double lrn_bias, double lrn_alpha, double lrn_beta) {
  check(x, at::kBFloat16, Nb * H * W * C, "x");
  check(w, at::kBFloat16, KH * KW * C * Cout, "w");
  TORCH_CHECK(Cout % 8 == 0, "Cout must be padded to a multiple of 8");
  auto ep = make_epi(out, Nb * OH * OW, Cout, Cout, bias, bias_n, relu, c10::nullopt, 0);
  hip_ok(mnistx::conv_fwd(BF(x), BF(w), (int)Nb, (int)H, (int)W, (int)C, (int)OH, (int)OW, (int)KH, (int)KW, (int)ph,
                          (int)pw, (int)Cout, ep, cur_stream(), lrn_params(lrn_r, lrn_bias, lrn_alpha, lrn_beta)),
         "conv_fwd");
}

void conv_dgrad(Tensor dy, Tensor w, Tensor out, int64_t Nb, int64_t OH, int64_t OW, int64_t Cout, int64_t H,
                int64_t W, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t Cin, optional<Tensor> mask) {
  check(dy, at::kBFloat16, Nb * OH * OW * Cout, "dy");
  check(w, at::kBFloat16, KH * KW * Cin * Cout, "w");
  TORCH_CHECK(Cout % 8 == 0 && Cin % 8 == 0, "channels must be padded to multiples of 8");
  auto ep = make_epi(out, Nb * H * W, Cin, Cin, c10::nullopt, 0, false, mask, Cin);
  hip_ok(mnistx::conv_dgrad(BF(dy), BF(w), (int)Nb, (int)OH, (int)OW, (int)Cout, (int)H, (int)W, (int)KH, (int)KW,
                            (int)ph, (int)pw, (int)Cin, ep, cur_stream()),
         "conv_dgrad");
}

int64_t conv_wgrad(Tensor x, Tensor dy, Tensor slab, int64_t Nb, int64_t H, int64_t W, int64_t C, int64_t OH,
                   int64_t OW, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t Cout, bool with_bias,
                   int64_t splits, int64_t lrn_r, double lrn_bias, double lrn_alpha, double lrn_beta) {
  check(x, at::kBFloat16, Nb * H * W * C, "x");
  check(dy, at::kBFloat16, Nb * OH * OW * Cout, "dy");
  TORCH_CHECK(Cout % 8 == 0, "Cout must be padded to a multiple of 8");
  const int64_t M = KH * KW * C + (with_bias ? 1 : 0);
  const bool halo = mnistx::conv_halo_enabled() &&
                    mnistx::conv5_halo_wgrad_ok((int)H, (int)W, (int)C, (int)OH, (int)OW, (int)KH, (int)KW, (int)ph,
                                                (int)pw, (int)Cout, with_bias ? 1 : 0);
  // halo weight gradient: one partial per persistent block (at most `splits`)
  const int64_t S = halo ? std::max<int64_t>(1, std::min<int64_t>(splits, mnistx::conv5_halo_wgrad_grid((int)Nb)))
                         : eff_splits(Nb * OH * OW, splits);
  auto ep = make_slab(slab, S, M, Cout);
  hip_ok(mnistx::conv_wgrad(BF(x), BF(dy), (int)Nb, (int)H, (int)W, (int)C, (int)OH, (int)OW, (int)KH, (int)KW,
                            (int)ph, (int)pw, (int)Cout, with_bias ? 1 : 0, (int)S, ep, cur_stream(),
                            lrn_params(lrn_r, lrn_bias, lrn_alpha, lrn_beta)),
         "conv_wgrad");
  return S;
}

void maxpool_fwd(Tensor x, Tensor y, Tensor arg, int64_t Nb, int64_t H, int64_t W, int64_t C, int64_t OH,
                 int64_t OW) {
  TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
  TORCH_CHECK(OH == (H + 1) / 2 && OW == (W + 1) / 2, "2x2/2 SAME pooling shape");
  check(x, at::kBFloat16, Nb * H * W * C, "x");
  check(y, at::kBFloat16, Nb * OH * OW * C, "y");
  check(arg, at::kByte, Nb * OH * OW * C, "arg");
  hip_ok(mnistx::maxpool_fwd(BF(x), (int)Nb, (int)H, (int)W, (int)C, (int)OH, (int)OW, BFm(y), P<uint8_t>(arg),
                             cur_stream()),
         "maxpool_fwd");
}

void maxpool_bwd(Tensor dy, Tensor arg, Tensor y, bool relu_mask, Tensor dx, int64_t Nb, int64_t H, int64_t W,
                 int64_t C, int64_t OH, int64_t OW) {
  TORCH_CHECK(C % 8 == 0, "C must be a multiple of 8");
  TORCH_CHECK(OH == (H + 1) / 2 && OW == (W + 1) / 2, "2x2/2 SAME pooling shape");
  check(dy, at::kBFloat16, Nb * OH * OW * C, "dy");
  check(arg, at::kByte, Nb * OH * OW * C, "arg");
  check(y, at::kBFloat16, Nb * OH * OW * C, "y");
  check(dx, at::kBFloat16, Nb * H * W * C, "dx");
  hip_ok(mnistx::maxpool_bwd(BF(dy), P<const uint8_t>(arg), BF(y), relu_mask ? 1 : 0, (int)Nb, (int)H, (int)W,
                             (int)C, (int)OH, (int)OW, BFm(dx), cur_stream()),
         "maxpool_bwd");
}

void lrn_fwd(Tensor x, Tensor y, int64_t P_, int64_t C, int64_t r, double bias, double alpha, double beta) {
  check(x, at::kBFloat16, P_ * C, "x");
  check(y, at::kBFloat16, P_ * C, "y");
  hip_ok(mnistx::lrn_fwd(BF(x), (int)P_, (int)C, (int)r, (float)bias, (float)alpha, (float)beta, BFm(y),
                         cur_stream()),
         "lrn_fwd");
}

void lrn_bwd(Tensor x, Tensor dy, Tensor dx, int64_t P_, int64_t C, int64_t r, double bias, double alpha,
             double beta, bool relu_mask) {
  check(x, at::kBFloat16, P_ * C, "x");
  check(dy, at::kBFloat16, P_ * C, "dy");
  check(dx, at::kBFloat16, P_ * C, "dx");
  hip_ok(mnistx::lrn_bwd(BF(x), BF(dy), (int)P_, (int)C, (int)r, (float)bias, (float)alpha, (float)beta,
                         relu_mask ? 1 : 0, BFm(dx), cur_stream()),
         "lrn_bwd");
}

bool lrn_pool_supported(int64_t H, int64_t W, int64_t C, int64_t r) {
  return mnistx::lrn_pool_supported((int)H, (int)W, (int)C, (int)r);
}

void lrn_pool_fwd(Tensor x, Tensor y, Tensor arg, int64_t Nb, int64_t H, int64_t W, int64_t C, int64_t r,
                  double bias, double alpha, double beta, bool nonneg) {
  TORCH_CHECK(mnistx::lrn_pool_supported((int)H, (int)W, (int)C, (int)r), "lrn_pool: unsupported geometry");
  check(x, at::kBFloat16, Nb * H * W * C, "x");
  check(y, at::kBFloat16, Nb * (H / 2) * (W / 2) * C, "y");
  check(arg, at::kByte, Nb * (H / 2) * (W / 2) * C, "arg");
  hip_ok(mnistx::lrn_pool_fwd(BF(x), (int)Nb, (int)H, (int)W, (int)C, (int)r, (float)bias, (float)alpha,
                              (float)beta, BFm(y), P<uint8_t>(arg), cur_stream(), nonneg ? 1 : 0),
         "lrn_pool_fwd");
}

void lrn_pool_bwd(Tensor x, Tensor dP, Tensor arg, Tensor dx, int64_t Nb, int64_t H, int64_t W, int64_t C,
                  int64_t r, double bias, double alpha, double beta, bool relu_mask) {
  TORCH_CHECK(mnistx::lrn_pool_supported((int)H, (int)W, (int)C, (int)r), "lrn_pool: unsupported geometry");
  check(x, at::kBFloat16, Nb * H * W * C, "x");
  check(dP, at::kBFloat16, Nb * (H / 2) * (W / 2) * C, "dP");
  check(arg, at::kByte, Nb * (H / 2) * (W / 2) * C, "arg");
  check(dx, at::kBFloat16, Nb * H * W * C, "dx");
  hip_ok(mnistx::lrn_pool_bwd(BF(x), BF(dP), P<const uint8_t>(arg), (int)Nb, (int)H, (int)W, (int)C, (int)r,
                              (float)bias, (float)alpha, (float)beta, relu_mask ? 1 : 0, BFm(dx), cur_stream()),
         "lrn_pool_bwd");
}

void cast_f32_bf16_padded(Tensor src, Tensor dst, int64_t G, int64_t I, int64_t J, int64_t Ip, int64_t Jp) {
  check(src, at::kFloat, G * I * J, "src");
  check(dst, at::kBFloat16, G * Ip * Jp, "dst");
  TORCH_CHECK(Ip >= I && Jp >= J, "padding");
  hip_ok(mnistx::cast_f32_bf16_padded(P<const float>(src), BFm(dst), (int)G, (int)I, (int)J, (int)Ip, (int)Jp,
                                      cur_stream()),
         "cast_f32_bf16_padded");
}

std::vector<int64_t> gemm_tile(int64_t M, int64_t N, bool wgrad) {
  int bm, bn;
  mnistx::gemm_tile((int)M, (int)N, wgrad ? 1 : 0, &bm, &bn);
  return {bm, bn};
}

}  // namespace

void bind_layers(py::module_& m) {
  m.def("dense_fwd", &dense_fwd, py::arg("x"), py::arg("w"), py::arg("out"), py::arg("M"), py::arg("N"), py::arg("K"),
        py::arg("ldx"), py::arg("ldw"), py::arg("ldc"), py::arg("bias"), py::arg("bias_n"), py::arg("relu"),
        py::arg("mask"), py::arg("ldm"), py::arg("tile") = -1);
  m.def("dense_dgrad", &dense_dgrad, py::arg("dy"), py::arg("w"), py::arg("out"), py::arg("M"), py::arg("N"),
        py::arg("K"), py::arg("lddy"), py::arg("ldw"), py::arg("ldc"), py::arg("mask"), py::arg("ldm"),
        py::arg("tile") = -1);
  m.def("dense_wgrad", &dense_wgrad, py::arg("x"), py::arg("dy"), py::arg("slab"), py::arg("Din"), py::arg("Dout"),
        py::arg("B"), py::arg("ldx"), py::arg("lddy"), py::arg("with_bias"), py::arg("splits"), py::arg("tile") = -1);
  m.def("conv_wgrad_pref_splits", &conv_wgrad_pref_splits);
  m.def("dense_wgrad_group", &dense_wgrad_group);
  m.def("conv_fwd", &conv_fwd, py::arg("x"), py::arg("w"), py::arg("out"), py::arg("Nb"), py::arg("H"), py::arg("W"),
        py::arg("C"), py::arg("OH"), py::arg("OW"), py::arg("KH"), py::arg("KW"), py::arg("ph"), py::arg("pw"),
        py::arg("Cout"), py::arg("bias"), py::arg("bias_n"), py::arg("relu"), py::arg("lrn_r") = 0,
        py::arg("lrn_bias") = 0.0, py::arg("lrn_alpha") = 0.0, py::arg("lrn_beta") = 0.0);
  m.def("conv_dgrad", &conv_dgrad);
  m.def("conv_wgrad", &conv_wgrad, py::arg("x"), py::arg("dy"), py::arg("slab"), py::arg("Nb"), py::arg("H"),
        py::arg("W"), py::arg("C"), py::arg("OH"), py::arg("OW"), py::arg("KH"), py::arg("KW"), py::arg("ph"),
        py::arg("pw"), py::arg("Cout"), py::arg("with_bias"), py::arg("splits"), py::arg("lrn_r") = 0,
        py::arg("lrn_bias") = 0.0, py::arg("lrn_alpha") = 0.0, py::arg("lrn_beta") = 0.0);
  m.def("maxpool_fwd", &maxpool_fwd);
  m.def("maxpool_bwd", &maxpool_bwd);
  m.def("lrn_fwd", &lrn_fwd);
  m.def("lrn_bwd", &lrn_bwd);
  m.def("lrn_pool_supported", &lrn_pool_supported);
  m.def("lrn_pool_fwd", &lrn_pool_fwd, py::arg("x"), py::arg("y"), py::arg("arg"), py::arg("Nb"), py::arg("H"),
        py::arg("W"), py::arg("C"), py::arg("r"), py::arg("bias"), py::arg("alpha"), py::arg("beta"),
        py::arg("nonneg") = false);
  m.def("lrn_pool_bwd", &lrn_pool_bwd);
  m.def("lrn_set_packed", [](bool on) { mnistx::lrn_set_packed(on ? 1 : 0); });
  m.def("cast_f32_bf16_padded", &cast_f32_bf16_padded);
  m.def("gemm_tile", &gemm_tile);
  m.def("set_gemm256", &mnistx::set_gemm256, "route the GEMMs that fill the GPU to gemm256.hip (A/B switch)");
  m.def("gemm256_enabled", &mnistx::gemm256_enabled);
  m.def("set_gemm256_debug", [](int64_t b) { mnistx::set_gemm256_debug((int)b); });
  m.def("set_tile192", [](int64_t on) { mnistx::set_tile192((int)on); },
        "A/B switch of gemm.hip's 192-column tiles (MNISTX_TILE192)");
  m.def("set_halo_variants", [](int64_t f, int64_t d) { mnistx::set_halo_variants((int)f, (int)d); });
}
