// _kernels bindings: the fp32 (reference precision) path.
#include "bind/common.h"

namespace {

// ---------------------------------------------------------------- fp32 (reference precision) path
const float* Fo(const optional<Tensor>& t, int64_t need, const char* name) {
  if (!has(t)) return nullptr;
  check(*t, at::kFloat, need, name);
  return P<const float>(*t);
}

void f32_dense_fwd(Tensor x, Tensor w, Tensor y, int64_t M, int64_t N, int64_t K, int64_t ldy, optional<Tensor> bias,
                   bool relu) {
  check(x, at::kFloat, M * K, "x");
  check(w, at::kFloat, K * N, "w");
  TORCH_CHECK(ldy >= N, "ldy");
  check(y, at::kFloat, span(M, ldy, N), "y");
  hip_ok(mnistx::f32_dense_fwd(P<const float>(x), P<const float>(w), (int)M, (int)N, (int)K, Fo(bias, N, "bias"),
                               (int)N, relu ? 1 : 0, P<float>(y), (int)ldy, cur_stream()),
         "f32_dense_fwd");
}

void f32_dense_dgrad(Tensor dy, Tensor w, Tensor dx, int64_t M, int64_t Din, int64_t Dout, optional<Tensor> mask) {
  check(dy, at::kFloat, M * Dout, "dy");
  check(w, at::kFloat, Din * Dout, "w");
  check(dx, at::kFloat, M * Din, "dx");
  hip_ok(mnistx::f32_dense_dgrad(P<const float>(dy), P<const float>(w), (int)M, (int)Din, (int)Dout,
                                 Fo(mask, M * Din, "mask"), P<float>(dx), cur_stream()),
         "f32_dense_dgrad");
}

// returns the split count written (the reduce must sum exactly those partials)
int64_t f32_dense_wgrad(Tensor x, Tensor dy, Tensor slab, int64_t B, int64_t Din, int64_t Dout, int64_t splits) {
  check(x, at::kFloat, B * Din, "x");
  check(dy, at::kFloat, B * Dout, "dy");
  TORCH_CHECK(splits >= 1 && splits <= 65535, "splits");
  check(slab, at::kFloat, splits * (Din + 1) * Dout, "slab");
  int used = (int)splits;
  hip_ok(mnistx::f32_dense_wgrad(P<const float>(x), P<const float>(dy), (int)B, (int)Din, (int)Dout, (int)splits,
                                 P<float>(slab), cur_stream(), &used),
         "f32_dense_wgrad");
  return used;
}

void f32_conv_fwd(Tensor x, Tensor w, Tensor y, int64_t Nb, int64_t H, int64_t W, int64_t C, int64_t OH, int64_t OW,
                  int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t Cout, optional<Tensor> bias, bool relu) {
  check(x, at::kFloat, Nb * H * W * C, "x");
  check(w, at::kFloat, KH * KW * C * Cout, "w");
  check(y, at::kFloat, Nb * OH * OW * Cout, "y");
  hip_ok(mnistx::f32_conv_fwd(P<const float>(x), P<const float>(w), (int)Nb, (int)H, (int)W, (int)C, (int)OH,
                              (int)OW, (int)KH, (int)KW, (int)ph, (int)pw, (int)Cout, Fo(bias, Cout, "bias"),
                              relu ? 1 : 0, P<float>(y), cur_stream()),
         "f32_conv_fwd");
}

void f32_conv_dgrad(Tensor dy, Tensor w, Tensor dx, int64_t Nb, int64_t OH, int64_t OW, int64_t Cout, int64_t H,
                    int64_t W, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t Cin, optional<Tensor> mask) {
  check(dy, at::kFloat, Nb * OH * OW * Cout, "dy");
  check(w, at::kFloat, KH * KW * Cin * Cout, "w");
  check(dx, at::kFloat, Nb * H * W * Cin, "dx");
  hip_ok(mnistx::f32_conv_dgrad(P<const float>(dy), P<const float>(w), (int)Nb, (int)OH, (int)OW, (int)Cout, (int)H,
                                (int)W, (int)KH, (int)KW, (int)ph, (int)pw, (int)Cin,
                                Fo(mask, Nb * H * W * Cin, "mask"), P<float>(dx), cur_stream()),
         "f32_conv_dgrad");
}

void f32_conv_wgrad(Tensor x, Tensor dy, Tensor slab, int64_t Nb, int64_t H, int64_t W, int64_t C, int64_t OH,
                    int64_t OW, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t Cout, int64_t splits) {
  check(x, at::kFloat, Nb * H * W * C, "x");
  check(dy, at::kFloat, Nb * OH * OW * Cout, "dy");
  TORCH_CHECK(splits >= 1 && splits <= 65535, "splits");
  check(slab, at::kFloat, splits * (KH * KW * C + 1) * Cout, "slab");
  hip_ok(mnistx::f32_conv_wgrad(P<const float>(x), P<const float>(dy), (int)Nb, (int)H, (int)W, (int)C, (int)OH,
                                (int)OW, (int)KH, (int)KW, (int)ph, (int)pw, (int)Cout, (int)splits, P<float>(slab),
                                cur_stream()),
         "f32_conv_wgrad");
}

// Split count the fp32 conv weight gradient prefers: the LDS-halo kernel's resident
// grid (one partial per workgroup) when it covers the geometry, else -1 (GEMM rule).
int64_t f32_conv_wgrad_pref_splits(int64_t H, int64_t W, int64_t C, int64_t OH, int64_t OW, int64_t KH, int64_t KW,
                                   int64_t ph, int64_t pw, int64_t Cout) {
  if (mnistx::f32_halo_wgrad_ok((int)H, (int)W, (int)C, (int)OH, (int)OW, (int)KH, (int)KW, (int)ph, (int)pw,
                                (int)Cout))
    return mnistx::f32_halo_wgrad_grid();
  if (mnistx::f32_conv1_ok((int)H, (int)W, (int)C, (int)OH, (int)OW, (int)KH, (int)KW, (int)ph, (int)pw, (int)Cout))
    return mnistx::f32_conv1_wgrad_grid();
  return -1;
}

void f32_maxpool_fwd(Tensor x, Tensor y, Tensor arg, int64_t Nb, int64_t H, int64_t W, int64_t C) {
  const int64_t OH = (H + 1) / 2, OW = (W + 1) / 2;
  check(x, at::kFloat, Nb * H * W * C, "x");
  check(y, at::kFloat, Nb * OH * OW * C, "y");
  check(arg, at::kByte, Nb * OH * OW * C, "arg");
  hip_ok(mnistx::f32_maxpool_fwd(P<const float>(x), (int)Nb, (int)H, (int)W, (int)C, (int)OH, (int)OW, P<float>(y),
                                 P<uint8_t>(arg), cur_stream()),
         "f32_maxpool_fwd");
}

void f32_maxpool_bwd(Tensor dy, Tensor arg, Tensor y, bool relu_mask, Tensor dx, int64_t Nb, int64_t H, int64_t W,
                     int64_t C) {
  const int64_t OH = (H + 1) / 2, OW = (W + 1) / 2;
  check(dy, at::kFloat, Nb * OH * OW * C, "dy");
  check(arg, at::kByte, Nb * OH * OW * C, "arg");
  check(y, at::kFloat, Nb * OH * OW * C, "y");
  check(dx, at::kFloat, Nb * H * W * C, "dx");
  hip_ok(mnistx::f32_maxpool_bwd(P<const float>(dy), P<const uint8_t>(arg), P<const float>(y), relu_mask ? 1 : 0,
                                 (int)Nb, (int)H, (int)W, (int)C, (int)OH, (int)OW, P<float>(dx), cur_stream()),
         "f32_maxpool_bwd");
}

void f32_lrn_fwd(Tensor x, Tensor y, int64_t P_, int64_t C, int64_t r, double bias, double alpha, double beta) {
  TORCH_CHECK(C <= 64, "f32 LRN: C <= 64");
  check(x, at::kFloat, P_ * C, "x");
  check(y, at::kFloat, P_ * C, "y");
  hip_ok(mnistx::f32_lrn_fwd(P<const float>(x), P_, (int)C, (int)r, (float)bias, (float)alpha, (float)beta,
                             P<float>(y), cur_stream()),
         "f32_lrn_fwd");
}

void f32_lrn_bwd(Tensor x, Tensor dy, Tensor dx, int64_t P_, int64_t C, int64_t r, double bias, double alpha,
                 double beta, bool relu_mask) {
  TORCH_CHECK(C <= 64, "f32 LRN: C <= 64");
  check(x, at::kFloat, P_ * C, "x");
  check(dy, at::kFloat, P_ * C, "dy");
  check(dx, at::kFloat, P_ * C, "dx");
  hip_ok(mnistx::f32_lrn_bwd(P<const float>(x), P<const float>(dy), P_, (int)C, (int)r, (float)bias, (float)alpha,
                             (float)beta, relu_mask ? 1 : 0, P<float>(dx), cur_stream()),
         "f32_lrn_bwd");
}

// fp32 conv1 (28x28x1 -> 32, 5x5 SAME) + bias + ReLU + 2x2 max-pool in one kernel, and its
// weight gradient from dL/d pool + the codes (tests/test_f32_gpu.py)
bool f32_conv1_pool_ok(int64_t H, int64_t W, int64_t C, int64_t OH, int64_t OW, int64_t KH, int64_t KW, int64_t ph,
                       int64_t pw, int64_t Cout) {
  return mnistx::f32_conv1_ok((int)H, (int)W, (int)C, (int)OH, (int)OW, (int)KH, (int)KW, (int)ph, (int)pw, (int)Cout);
}
void f32_conv1_fwd_pool(Tensor x, Tensor w, optional<Tensor> bias, Tensor y, Tensor arg, int64_t Nb) {
  check(x, at::kFloat, Nb * 784, "x");
  check(w, at::kFloat, 25 * 32, "w");
  check(y, at::kFloat, Nb * 196 * 32, "y");
  check(arg, at::kByte, Nb * 196 * 32, "arg");
  TORCH_CHECK(aligned(y, 16) && aligned(arg, 4), "y / arg alignment");
  hip_ok(mnistx::f32_conv1_fwd_pool(P<const float>(x), P<const float>(w), (int)Nb, Fo(bias, 32, "bias"), P<float>(y),
                                    P<uint8_t>(arg), cur_stream()),
         "f32_conv1_fwd_pool");
}
int64_t f32_conv1_wgrad_unpool_grid() { return mnistx::f32_conv1_wgrad_unpool_grid(); }
void f32_conv1_wgrad_unpool(Tensor x, Tensor dp, Tensor codes, Tensor slab, int64_t Nb, int64_t splits) {
  check(x, at::kFloat, Nb * 784, "x");
  check(dp, at::kFloat, Nb * 196 * 32, "dp");
  check(codes, at::kByte, Nb * 196 * 32, "codes");
  TORCH_CHECK(splits >= 1 && splits <= 65535, "splits");
  check(slab, at::kFloat, splits * 26 * 32, "slab");
  hip_ok(mnistx::f32_conv1_wgrad_unpool(P<const float>(x), P<const float>(dp), P<const uint8_t>(codes), (int)Nb,
                                        (int)splits, P<float>(slab), cur_stream()),
         "f32_conv1_wgrad_unpool");
}
// with norm1's backward folded in: dn = dL/d norm1, p1 = pool1 (the LRN input), radius 4
void f32_conv1_wgrad_lrn(Tensor x, Tensor dn, Tensor p1, Tensor codes, Tensor slab, int64_t Nb, int64_t splits,
                         double bias, double alpha, double beta) {
  check(x, at::kFloat, Nb * 784, "x");
  check(dn, at::kFloat, Nb * 196 * 32, "dn");
  check(p1, at::kFloat, Nb * 196 * 32, "p1");
  check(codes, at::kByte, Nb * 196 * 32, "codes");
  for (const Tensor* t : {&x, &dn, &p1, &codes})
    TORCH_CHECK(aligned(*t, 16), "x / dn / p1 / codes must be 16-byte aligned");
  TORCH_CHECK(Nb >= 1 && Nb * 196 * 32 * 4 < (int64_t)INT32_MAX * 2, "Nb");
  TORCH_CHECK(splits >= 1 && splits <= 65535, "splits");
  check(slab, at::kFloat, splits * 26 * 32, "slab");
  hip_ok(mnistx::f32_conv1_wgrad_lrn(P<const float>(x), P<const float>(dn), P<const float>(p1), P<const uint8_t>(codes),
                                     (int)Nb, (int)splits, (float)bias, (float)alpha, (float)beta, P<float>(slab),
                                     cur_stream()),
         "f32_conv1_wgrad_lrn");
}

// fp32 LRN + 2x2 max-pool fused (the reference's norm2 -> pool2) and its backward
bool f32_lrn_pool_ok(int64_t H, int64_t W, int64_t C, int64_t r) {
  return mnistx::f32_lrn_pool_ok((int)H, (int)W, (int)C, (int)r);
}
void f32_lrn_pool_fwd(Tensor x, Tensor y, Tensor arg, int64_t Nb, int64_t H, int64_t W, int64_t C, int64_t r,
                      double bias, double alpha, double beta) {
  check(x, at::kFloat, Nb * H * W * C, "x");
  check(y, at::kFloat, Nb * (H / 2) * (W / 2) * C, "y");
  check(arg, at::kByte, Nb * (H / 2) * (W / 2) * C, "arg");
  hip_ok(mnistx::f32_lrn_pool_fwd(P<const float>(x), (int)Nb, (int)H, (int)W, (int)C, (int)r, (float)bias,
                                  (float)alpha, (float)beta, P<float>(y), P<uint8_t>(arg), cur_stream()),
         "f32_lrn_pool_fwd");
}
void f32_lrn_pool_bwd(Tensor x, Tensor dy, Tensor arg, Tensor dx, int64_t Nb, int64_t H, int64_t W, int64_t C,
                      int64_t r, double bias, double alpha, double beta, bool relu_mask) {
  check(x, at::kFloat, Nb * H * W * C, "x");
  check(dy, at::kFloat, Nb * (H / 2) * (W / 2) * C, "dy");
  check(arg, at::kByte, Nb * (H / 2) * (W / 2) * C, "arg");
  check(dx, at::kFloat, Nb * H * W * C, "dx");
  hip_ok(mnistx::f32_lrn_pool_bwd(P<const float>(x), P<const float>(dy), P<const uint8_t>(arg), (int)Nb, (int)H,
                                  (int)W, (int)C, (int)r, (float)bias, (float)alpha, (float)beta, relu_mask ? 1 : 0,
                                  P<float>(dx), cur_stream()),
         "f32_lrn_pool_bwd");
}

void f32_prep_images(Tensor src, Tensor idx, Tensor lab_src, Tensor out, Tensor lab_out, int64_t HW, int64_t Csrc,
                     int64_t Cdst) {
  const int64_t B = idx.numel();
  check(idx, at::kLong, B, "idx");
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kByte && src.is_contiguous(), "src: uint8 GPU tensor");
  TORCH_CHECK(src.numel() % (HW * Csrc) == 0, "src size");
  TORCH_CHECK(Csrc == Cdst || Csrc == 1, "channels: equal or 1 -> C replication");
  check(lab_src, at::kInt, src.numel() / (HW * Csrc), "lab_src");
  check(out, at::kFloat, B * HW * Cdst, "out");
  check(lab_out, at::kInt, B, "lab_out");
  hip_ok(mnistx::f32_prep_images(P<const uint8_t>(src), P<const int64_t>(idx), P<const int32_t>(lab_src), (int)B,
                                 (int)HW, (int)Csrc, (int)Cdst, P<float>(out), P<int32_t>(lab_out), cur_stream()),
         "f32_prep_images");
}

}  // namespace

void bind_f32(py::module_& m) {
  m.def("f32_dense_fwd", &f32_dense_fwd);
  m.def("f32_dense_dgrad", &f32_dense_dgrad);
  m.def("f32_dense_wgrad", &f32_dense_wgrad);
  m.def("f32_wgrad_splits_cap", [](int64_t din, int64_t dout, int64_t b) {
    return (int64_t)mnistx::f32_wgrad_splits_cap((int)din, (int)dout, (int)b);
  }, "slab partials the fp32 256 x 256 weight-gradient path writes for this shape (0: not that path)");
  m.def("f32_conv_fwd", &f32_conv_fwd);
  m.def("f32_conv_dgrad", &f32_conv_dgrad);
  m.def("f32_conv_wgrad", &f32_conv_wgrad);
  m.def("f32_conv_wgrad_pref_splits", &f32_conv_wgrad_pref_splits);
  m.def("set_f32_halo_fwd_variant", [](int64_t v) { mnistx::set_f32_halo_fwd_variant((int)v); });
  m.def("f32_maxpool_fwd", &f32_maxpool_fwd);
  m.def("f32_maxpool_bwd", &f32_maxpool_bwd);
  m.def("f32_lrn_fwd", &f32_lrn_fwd);
  m.def("f32_lrn_bwd", &f32_lrn_bwd);
  m.def("f32_conv1_pool_ok", &f32_conv1_pool_ok);
  m.def("f32_conv1_fwd_pool", &f32_conv1_fwd_pool);
  m.def("f32_conv1_wgrad_unpool_grid", &f32_conv1_wgrad_unpool_grid);
  m.def("f32_conv1_wgrad_unpool", &f32_conv1_wgrad_unpool);
  m.def("f32_conv1_wgrad_lrn", &f32_conv1_wgrad_lrn);
  m.def("f32_lrn_pool_ok", &f32_lrn_pool_ok);
  m.def("f32_lrn_pool_fwd", &f32_lrn_pool_fwd);
  m.def("f32_lrn_pool_bwd", &f32_lrn_pool_bwd);
  m.def("f32_prep_images", &f32_prep_images);
}
