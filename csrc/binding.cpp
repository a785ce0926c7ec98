#include <algorithm>
#include <cctype>
#include <cmath>
// Python bindings for the MNIST HIP kernels (torch extension `_kernels`).
//
// Every entry point validates device, dtype, contiguity and that each buffer is
// large enough for the indices the kernel will form, BEFORE launching: a
// mis-sized operand must raise here, never fault on the GPU.  Launches go to
// the caller's current HIP stream (so they are hipGraph-capturable and honour
// torch.cuda.stream contexts).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "kernels/launchers.h"

namespace {

using at::Tensor;
using c10::optional;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check(const Tensor& t, at::ScalarType dt, int64_t need, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, ": must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, ": expected dtype ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, ": must be contiguous");
  TORCH_CHECK(need >= 0 && t.numel() >= need, name, ": needs ", need, " elements, has ", t.numel());
}

int64_t span(int64_t rows, int64_t ld, int64_t cols) { return rows <= 0 ? 0 : (rows - 1) * ld + cols; }

template <class T>
T* P(const Tensor& t) { return reinterpret_cast<T*>(t.data_ptr()); }
const mnistx::bf16_t* BF(const Tensor& t) { return reinterpret_cast<const mnistx::bf16_t*>(t.data_ptr()); }
mnistx::bf16_t* BFm(const Tensor& t) { return reinterpret_cast<mnistx::bf16_t*>(t.data_ptr()); }

void hip_ok(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, what, " launch failed: ", hipGetErrorString(e));
}

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
  if (bias.has_value() && bias->defined()) {
    check(*bias, at::kFloat, bias_n, "bias");
    ep.bias = P<const float>(*bias);
    ep.bias_n = (int)bias_n;
  }
  ep.relu = relu ? 1 : 0;
  ep.mask = nullptr;
  ep.ldm = 0;
  if (mask.has_value() && mask->defined()) {
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

// lab_src [N] / lab_out [n] (optional, int32): gather the chosen rows' labels in the same launch
void perm_positions(Tensor out, int64_t start, int64_t N, int64_t seed, int64_t h, optional<Tensor> lab_src,
                    optional<Tensor> lab_out) {
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kLong && out.is_contiguous(), "perm_positions: out");
  TORCH_CHECK(N > 0 && h >= 1 && h <= 31 && (1ll << (2 * h)) >= N, "perm_positions: bad domain");
  const bool labs = lab_src.has_value() && lab_src->defined();
  TORCH_CHECK(labs == (lab_out.has_value() && lab_out->defined()), "perm_positions: lab_src and lab_out together");
  if (labs) {
    check(*lab_src, at::kInt, N, "lab_src");
    check(*lab_out, at::kInt, out.numel(), "lab_out");
  }
  hip_ok(mnistx::perm_positions(out.data_ptr<int64_t>(), start, (int)out.numel(), N, (uint32_t)seed, (int)h,
                                cur_stream(), labs ? P<const int32_t>(*lab_src) : nullptr,
                                labs ? P<int32_t>(*lab_out) : nullptr),
         "perm_positions");
}

void prep_images_perm(Tensor src, Tensor lab_src, Tensor out, Tensor lab_out, int64_t B, int64_t start, int64_t seed,
                      int64_t h) {
  TORCH_CHECK(src.dim() == 2 && src.size(1) == 784, "prep_images_perm: [N, 784] uint8 dataset");
  const int64_t N = src.size(0);
  check(src, at::kByte, N * 784, "src");
  check(lab_src, at::kInt, N, "lab_src");
  check(out, at::kBFloat16, B * 784, "out");
  check(lab_out, at::kInt, B, "lab_out");
  TORCH_CHECK(N > 0 && h >= 1 && h <= 31 && (1ll << (2 * h)) >= N, "prep_images_perm: bad domain");
  hip_ok(mnistx::prep_images_perm(P<const uint8_t>(src), P<const int32_t>(lab_src), (int)B, start, N, (uint32_t)seed,
                                  (int)h, BFm(out), P<int32_t>(lab_out), cur_stream()),
         "prep_images_perm");
}

void prep_images(Tensor src, Tensor idx, Tensor lab_src, Tensor out, Tensor lab_out, int64_t HW, int64_t Csrc,
                 int64_t Cdst) {
  const int64_t B = idx.numel();
  TORCH_CHECK((HW * Cdst) % 8 == 0, "HW*C must be a multiple of 8");
  check(idx, at::kLong, B, "idx");
  TORCH_CHECK(src.is_cuda() && src.scalar_type() == at::kByte && src.is_contiguous(), "src: uint8 GPU tensor");
  TORCH_CHECK(src.numel() % (HW * Csrc) == 0, "src size");
  check(lab_src, at::kInt, src.numel() / (HW * Csrc), "lab_src");
  check(out, at::kBFloat16, B * HW * Cdst, "out");
  check(lab_out, at::kInt, B, "lab_out");
  hip_ok(mnistx::prep_images(P<const uint8_t>(src), P<const int64_t>(idx), P<const int32_t>(lab_src), (int)B,
                             (int)HW, (int)Csrc, (int)Cdst, BFm(out), P<int32_t>(lab_out), cur_stream()),
         "prep_images");
}

// the augmentation keys (augment.hip): a ValueError naming key and value, as data/augment.py raises
void augment_keys(const char* op, int64_t pos0, int64_t n, int64_t seed, int64_t shift, double rotate, double scale) {
  TORCH_CHECK_VALUE(shift >= 0 && shift <= mnistx::AUG_MAX_SHIFT, op,
                    ": augment_shift must be an integer with 0 <= augment_shift <= 8, got ", shift);
  TORCH_CHECK_VALUE(std::isfinite(rotate) && rotate >= 0.0 && rotate <= (double)mnistx::AUG_MAX_ROTATE, op,
                    ": augment_rotate must be finite with 0 <= augment_rotate <= 180, got ", rotate);
  TORCH_CHECK_VALUE(std::isfinite(scale) && scale >= 0.0 && scale <= (double)mnistx::AUG_MAX_SCALE, op,
                    ": augment_scale must be finite with 0 <= augment_scale <= 0.5, got ", scale);
  TORCH_CHECK_VALUE(seed >= 0, op, ": augment_seed must be an integer with 0 <= augment_seed < 2^63, got ", seed);
  TORCH_CHECK_VALUE(pos0 >= 0 && pos0 <= INT64_MAX - n, op, ": pos0 must be >= 0 with pos0 + n below 2^63, got ", pos0);
}

// the elastic keys: the displacement scale, and the half table of the smoothing Gaussian as
// data/augment.py elastic_weights computes it (its one source: the kernels take the table, not sigma)
void elastic_alpha_ok(const char* op, double alpha) {
  TORCH_CHECK_VALUE(std::isfinite(alpha) && alpha >= 0.0 && alpha <= (double)mnistx::AUG_MAX_ELASTIC_ALPHA, op,
                    ": elastic_alpha must be finite with 0 <= elastic_alpha <= 64, got ", alpha);
}

void elastic_table_ok(const char* op, const Tensor& w) {
  TORCH_CHECK_VALUE(w.device().is_cpu() && w.scalar_type() == at::kFloat && w.dim() == 1 && w.is_contiguous() &&
                        w.numel() >= mnistx::AUG_MIN_ELASTIC_TAPS && w.numel() <= mnistx::AUG_MAX_ELASTIC_TAPS,
                    op, ": elastic_weights must be a 1-D CPU float32 tensor of ", mnistx::AUG_MIN_ELASTIC_TAPS, " to ",
                    mnistx::AUG_MAX_ELASTIC_TAPS, " entries (w_0 .. w_K)");
  const float* p = w.data_ptr<float>();
  double sum = 0.0;
  for (int64_t k = 0; k < w.numel(); ++k) {
    TORCH_CHECK_VALUE(std::isfinite(p[k]) && p[k] >= 0.f, op, ": elastic_weights must be finite and >= 0, got ", p[k],
                      " at ", k);
    sum += (k ? 2.0 : 1.0) * (double)p[k];
  }
  TORCH_CHECK_VALUE(std::fabs(sum - 1.0) <= 1e-5, op, ": elastic_weights must sum to 1 (w_0 + 2 sum w_k), got ", sum);
}

void augment_images(Tensor src, Tensor idx, Tensor lab_src, Tensor out, Tensor lab_out, int64_t Csrc, int64_t Cdst,
                    int64_t pos0, int64_t seed, int64_t shift, double rotate, double scale, double elastic_alpha,
                    optional<Tensor> elastic_weights) {
  const int64_t nb = idx.numel();
  augment_keys("augment_images", pos0, nb, seed, shift, rotate, scale);
  elastic_alpha_ok("augment_images", elastic_alpha);
  if (elastic_weights.has_value()) elastic_table_ok("augment_images", *elastic_weights);
  TORCH_CHECK_VALUE(elastic_alpha == 0.0 || elastic_weights.has_value(),
                    "augment_images: elastic_weights is required when elastic_alpha > 0");
  TORCH_CHECK((Csrc == 1 && Cdst == 1) || (Csrc == 3 && Cdst == 3) || (Csrc == 1 && Cdst == 3),
              "augment_images: (Csrc, Cdst) must be (1, 1), (3, 3) or (1, 3), got (", Csrc, ", ", Cdst, ")");
  TORCH_CHECK(src.dim() == 2 && src.size(1) == 784 * Csrc, "augment_images: src must be a [N, ", 784 * Csrc,
              "] uint8 dataset");
  const int64_t N = src.size(0);
  check(src, at::kByte, N * 784 * Csrc, "src");
  check(idx, at::kLong, nb, "idx");
  check(lab_src, at::kInt, N, "lab_src");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 || out.scalar_type() == at::kFloat,
              "augment_images: out must be bf16 or fp32, got ", out.scalar_type());
  TORCH_CHECK(out.dim() >= 1 && nb <= out.size(0), "augment_images: ", nb, " indices for an out of ",
              out.dim() >= 1 ? out.size(0) : 0, " rows");
  TORCH_CHECK(out.dim() >= 1 && out.numel() == out.size(0) * 784 * Cdst, "augment_images: out must be [B, 784 * ", Cdst,
              "]");
  check(out, out.scalar_type(), nb * 784 * Cdst, "out");
  check(lab_out, at::kInt, nb, "lab_out");
  TORCH_CHECK(nb < ((int64_t)1 << 31) / (784 * 3), "augment_images: batch too large");
  TORCH_CHECK(idx.device() == src.device() && lab_src.device() == src.device() && out.device() == src.device() &&
                  lab_out.device() == src.device(),
              "augment_images: every buffer must be on one device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(src.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "augment_images: src and out must be 16-byte aligned");
  if (elastic_alpha != 0.0) {
    hip_ok(mnistx::augment_images_elastic(P<const uint8_t>(src), P<const int64_t>(idx), P<const int32_t>(lab_src),
                                          (int)nb, (int)Csrc, (int)Cdst, pos0, seed, (int)shift, (float)rotate,
                                          (float)scale, (float)elastic_alpha, elastic_weights->data_ptr<float>(),
                                          (int)elastic_weights->numel(), out.data_ptr(),
                                          out.scalar_type() == at::kFloat, P<int32_t>(lab_out), cur_stream()),
           "augment_images (elastic)");
    return;
  }
  // elastic_alpha = 0: the affine kernel with its arguments, whatever table came along
  hip_ok(mnistx::augment_images(P<const uint8_t>(src), P<const int64_t>(idx), P<const int32_t>(lab_src), (int)nb,
                                (int)Csrc, (int)Cdst, pos0, seed, (int)shift, (float)rotate, (float)scale,
                                out.data_ptr(), out.scalar_type() == at::kFloat, P<int32_t>(lab_out), cur_stream()),
         "augment_images");
}

// the 16-bit draws of the elastic fields of positions pos0 .. pos0 + n - 1 as augment_images fills
// them: out int32 [n, 2, 784]
void augment_elastic_draws(Tensor out, int64_t pos0, int64_t seed) {
  TORCH_CHECK(out.dim() == 3 && out.size(1) == 2 && out.size(2) == 784,
              "augment_elastic_draws: out must be [n, 2, 784] int32");
  const int64_t n = out.size(0);
  augment_keys("augment_elastic_draws", pos0, n, seed, 0, 0.0, 0.0);
  check(out, at::kInt, n * 1568, "out");
  TORCH_CHECK(n < ((int64_t)1 << 20), "augment_elastic_draws: n too large");
  hip_ok(mnistx::augment_elastic_draws(P<int32_t>(out), (int)n, pos0, seed, cur_stream()), "augment_elastic_draws");
}

// the displacement field alpha * d of those positions as augment_images adds it: out fp32 [n, 2, 784]
void augment_elastic_field(Tensor out, int64_t pos0, int64_t seed, double elastic_alpha, Tensor elastic_weights) {
  TORCH_CHECK(out.dim() == 3 && out.size(1) == 2 && out.size(2) == 784,
              "augment_elastic_field: out must be [n, 2, 784] fp32");
  const int64_t n = out.size(0);
  augment_keys("augment_elastic_field", pos0, n, seed, 0, 0.0, 0.0);
  elastic_alpha_ok("augment_elastic_field", elastic_alpha);
  elastic_table_ok("augment_elastic_field", elastic_weights);
  check(out, at::kFloat, n * 1568, "out");
  TORCH_CHECK(n < ((int64_t)1 << 20), "augment_elastic_field: n too large");
  hip_ok(mnistx::augment_elastic_field(P<float>(out), (int)n, pos0, seed, (float)elastic_alpha,
                                       elastic_weights.data_ptr<float>(), (int)elastic_weights.numel(), cur_stream()),
         "augment_elastic_field");
}

// (tx, ty, theta, s) of positions pos0 .. pos0 + n - 1 as augment_images draws them: out fp32 [n, 4]
void augment_params(Tensor out, int64_t pos0, int64_t seed, int64_t shift, double rotate, double scale) {
  TORCH_CHECK(out.dim() == 2 && out.size(1) == 4, "augment_params: out must be [n, 4] fp32");
  const int64_t n = out.size(0);
  augment_keys("augment_params", pos0, n, seed, shift, rotate, scale);
  check(out, at::kFloat, n * 4, "out");
  TORCH_CHECK(n < ((int64_t)1 << 31), "augment_params: n too large");
  hip_ok(mnistx::augment_params(P<float>(out), (int)n, pos0, seed, (int)shift, (float)rotate, (float)scale,
                                cur_stream()),
         "augment_params");
}

// The tables of the mixing bindings (data/mix.py lam_table / side_table), device tensors: validated
// for dtype, length and device (ValueError); both None is a ValueError too.
struct MixTables {
  const float* T = nullptr;
  const int32_t* S = nullptr;
};
MixTables mix_tables(const char* op, const optional<Tensor>& lam_table, const optional<Tensor>& side_table,
                     const Tensor& on, int64_t pos0, int64_t n, int64_t seed, int64_t thr_p) {
  TORCH_CHECK_VALUE(pos0 >= 0 && n >= 0 && pos0 <= std::numeric_limits<int64_t>::max() - n, op,
                    ": pos0 must be >= 0 with pos0 + n <= 2^63, got ", pos0);
  TORCH_CHECK_VALUE(seed >= 0, op, ": seed must be >= 0 and below 2^63, got ", seed);
  TORCH_CHECK_VALUE(thr_p >= 0 && thr_p <= 65536, op, ": thr_p must be in [0, 65536], got ", thr_p);
  const bool ht = lam_table.has_value() && lam_table->defined(), hs = side_table.has_value() && side_table->defined();
  TORCH_CHECK_VALUE(ht || hs, op, ": lam_table (mixup) or side_table (CutMix) is required, got neither");
  MixTables t;
  if (ht) {
    TORCH_CHECK_VALUE(lam_table->scalar_type() == at::kFloat && lam_table->dim() == 1 && lam_table->numel() == 1025 &&
                          lam_table->is_contiguous() && lam_table->device() == on.device(),
                      op, ": lam_table must be a contiguous float32 tensor of 1025 entries on the buffer's device");
    t.T = P<const float>(*lam_table);
  }
  if (hs) {
    TORCH_CHECK_VALUE(side_table->scalar_type() == at::kInt && side_table->dim() == 1 && side_table->numel() == 1024 &&
                          side_table->is_contiguous() && side_table->device() == on.device(),
                      op, ": side_table must be a contiguous int32 tensor of 1024 entries on the buffer's device");
    t.S = P<const int32_t>(*side_table);
  }
  return t;
}

// mixup / CutMix in place on images [>= nb, 784, cdst] bf16 (mix.hip); labels2 / lam [>= nb] receive the
// second label and the weight of rows < nb
void mix_images(Tensor images, Tensor labels, Tensor labels2, Tensor lam, int64_t nb, int64_t cdst, int64_t pos0,
                int64_t seed, int64_t thr_p, optional<Tensor> lam_table, optional<Tensor> side_table) {
  const MixTables t = mix_tables("mix_images", lam_table, side_table, images, pos0, nb, seed, thr_p);
  TORCH_CHECK_VALUE(cdst == 1 || cdst == 3, "mix_images: cdst must be 1 or 3, got ", cdst);
  TORCH_CHECK(nb < ((int64_t)1 << 31) / (784 * 3), "mix_images: batch too large");
  check(images, at::kBFloat16, nb * 784 * cdst, "images");
  check(labels, at::kInt, nb, "labels");
  check(labels2, at::kInt, nb, "labels2");
  check(lam, at::kFloat, nb, "lam");
  TORCH_CHECK(labels.device() == images.device() && labels2.device() == images.device() &&
                  lam.device() == images.device(),
              "mix_images: every buffer must be on one device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(images.data_ptr()) % 16 == 0, "mix_images: images must be 16-byte aligned");
  hip_ok(mnistx::mix_images(BFm(images), P<const int32_t>(labels), P<int32_t>(labels2), P<float>(lam), (int)nb,
                            (int)cdst, pos0, seed, thr_p, t.T, t.S, cur_stream()),
         "mix_images");
}

// what mix_images draws for positions pos0 .. pos0 + n - 1: out int32 [n, 6] = (kind, lam bits, x0, x1, y0, y1)
void mix_params(Tensor out, int64_t pos0, int64_t seed, int64_t thr_p, optional<Tensor> lam_table,
                optional<Tensor> side_table) {
  TORCH_CHECK(out.dim() == 2 && out.size(1) == 6, "mix_params: out must be [n, 6] int32");
  const int64_t n = out.size(0);
  const MixTables t = mix_tables("mix_params", lam_table, side_table, out, pos0, n, seed, thr_p);
  check(out, at::kInt, n * 6, "out");
  TORCH_CHECK(n < ((int64_t)1 << 28), "mix_params: n too large");
  hip_ok(mnistx::mix_params(P<int32_t>(out), (int)n, pos0, seed, thr_p, t.T, t.S, cur_stream()), "mix_params");
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
  const bool h2 = labels2.has_value() && labels2->defined(), hl = lam.has_value() && lam->defined();
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
  if (!(teacher.has_value() && teacher->defined())) return a;
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
  const MixArgs mx = mix_args(labels2, lam, B, labels.has_value() && labels->defined() ? &*labels : nullptr, "softmax_ce");
  const DistillArgs ds = distill_args(teacher_logits, teacher_ld, distill_alpha, distill_temperature, B, NC, logits, eps,
                                      mx.labels2 != nullptr, false, "softmax_ce");
  TORCH_CHECK_VALUE(!ds.on || (labels.has_value() && labels->defined()), "softmax_ce: teacher_logits needs labels");
  TORCH_CHECK(ldl >= NC, "ldl < NC");
  check(logits, at::kFloat, B * ldl, "logits");   // whole padded rows (vector loads)
  const int32_t* lab = nullptr;
  if (labels.has_value() && labels->defined()) {
    check(*labels, at::kInt, B, "labels");
    lab = P<const int32_t>(*labels);
  }
  TORCH_CHECK(eps == 0.f || lab != nullptr, "softmax_ce: label_smoothing needs labels");
  mnistx::bf16_t* dl = nullptr;
  if (dlogits.has_value() && dlogits->defined()) {
    TORCH_CHECK(lab != nullptr, "dlogits needs labels");
    TORCH_CHECK(ldd >= NC, "ldd < NC");
    check(*dlogits, at::kBFloat16, B * ldd, "dlogits");
    TORCH_CHECK(ldd == ldl || ldd >= NC, "ldd");
    dl = BFm(*dlogits);
  }
  float* st = nullptr;
  if (stats.has_value() && stats->defined()) {
    check(*stats, at::kFloat, 8, "stats");
    st = P<float>(*stats);
  }
  float* pr = nullptr;
  if (probs.has_value() && probs->defined()) {
    check(*probs, at::kFloat, B * NC, "probs");
    pr = P<float>(*probs);
  }
  float* wk = nullptr;
  if (work.has_value() && work->defined()) {
    check(*work, at::kFloat, mnistx::CE_WORK_FLOATS, "work");
    wk = P<float>(*work);
  }
  float* db = nullptr;
  if (dbias.has_value() && dbias->defined()) {
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
  TORCH_CHECK_VALUE(!ds.on || (dl.has_value() && dl->defined()),
                    "ce_tail: teacher_logits is a training quantity and needs dl");
  TORCH_CHECK(mnistx::ce_tail_supported(192, (int)nc, (int)std::max<int64_t>(nb, 1)), "ce_tail: unsupported geometry");
  check(x, at::kBFloat16, nb * 192, "x");
  check(w5t, at::kBFloat16, 16 * 192, "w5t");
  check(b5, at::kFloat, nc, "b5");
  check(labels, at::kInt, nb, "labels");
  check(logits, at::kFloat, nb * 16, "logits");
  check(stats, at::kFloat, 8, "stats");
  for (const Tensor* t : {&x, &w5t, &logits})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "ce_tail: operands must be 16-byte aligned");
  const bool has_work = work.has_value() && work->defined();
  if (has_work) check(*work, at::kFloat, mnistx::CE_WORK_FLOATS, "work");
  mnistx::bf16_t *pdl = nullptr, *pdx = nullptr;
  if (dl.has_value() && dl->defined()) {
    TORCH_CHECK(dx.has_value() && dx->defined(), "ce_tail: dl needs dx");
    check(*dl, at::kBFloat16, nb * 16, "dl");
    check(*dx, at::kBFloat16, nb * 192, "dx");
    for (const Tensor* t : {&*dl, &*dx})
      TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "ce_tail: gradients must be 16-byte aligned");
    pdl = BFm(*dl);
    pdx = BFm(*dx);
  }
  float* db = nullptr;
  if (dbias.has_value() && dbias->defined()) {
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
  TORCH_CHECK_VALUE(!ds.on || (dl.has_value() && dl->defined()),
                    "mlp_head: teacher_logits is a training quantity and needs dl");
  mnistx::HeadDrop hd{};
  if (dropout != 0.0) {   // 0 launches what is launched without the key
    TORCH_CHECK_VALUE(drop_step.has_value() && drop_step->defined(), "mlp_head: dropout needs drop_step");
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
  const bool has_work = work.has_value() && work->defined();   // none: order-dependent atomics
  if (has_work) check(*work, at::kFloat, mnistx::CE_WORK_FLOATS, "work");
  for (const Tensor* t : {&x, &w3t, &w4t, &w5t, &h3, &h4, &logits})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "mlp_head: operands must be 16-byte aligned");
  mnistx::bf16_t *pdl = nullptr, *pdh4 = nullptr, *pdh3 = nullptr, *pdx = nullptr;
  if (dl.has_value() && dl->defined()) {
    TORCH_CHECK(dh4.has_value() && dh3.has_value() && dx.has_value(), "mlp_head: dl needs dh4, dh3, dx");
    check(*dl, at::kBFloat16, nb * 16, "dl");
    check(*dh4, at::kBFloat16, nb * 88, "dh4");
    check(*dh3, at::kBFloat16, nb * 120, "dh3");
    check(*dx, at::kBFloat16, nb * 400, "dx");
    for (const Tensor* t : {&*dl, &*dh4, &*dh3, &*dx})
      TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 8 == 0, "mlp_head: gradients must be 8-byte aligned");
    pdl = BFm(*dl);
    pdh4 = BFm(*dh4);
    pdh3 = BFm(*dh3);
    pdx = BFm(*dx);
  }
  float* db = nullptr;
  if (dbias.has_value() && dbias->defined()) {
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
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, op, ": the buffer must be 16-byte aligned");
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

mnistx::RedSpec red_spec(Tensor slab, int64_t splits, int64_t M, int64_t N, int64_t G, int64_t Ipad, int64_t I,
                         int64_t J, int64_t bias_row, Tensor wdst, const Tensor* bdst, double scale) {
  check(slab, at::kFloat, splits * M * N, "slab");
  TORCH_CHECK(I <= Ipad && J <= N && G * Ipad <= M, "reduce geometry");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(slab.data_ptr()) % 16 == 0, "slab must be 16-byte aligned");
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
  const Tensor* bp = (bdst.has_value() && bdst->defined()) ? &*bdst : nullptr;
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

// segs: int64 tensor [nseg, 14] on CPU:
//   off, n, G, I, J, Ip, Jp, bf_off, wd_bits(float32 as int), track_l2, bft_off, Jt, It, 0
mnistx::FinArgs prep_fin(Tensor step, Tensor stats, optional<Tensor> l2, optional<Tensor> wds, int64_t nw,
                         optional<Tensor> loss_ema, int64_t n_ema, int64_t batch, bool increment,
                         optional<Tensor> l2_ranges, optional<Tensor> ce_work, int64_t ce_nblk);

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
  TORCH_CHECK(!(scheduled && guard.has_value() && guard->defined()),
              "fused_optimizer: lr_schedule '", lr_schedule, "' / warmup_steps ", warmup_steps,
              " cannot be combined with a push guard (parameter-server mode)");
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
    TORCH_CHECK(slot2.has_value() && slot2->defined(), "fused_optimizer: rule '", rule, "' needs slot2");
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
  if (l2.has_value() && l2->defined()) {
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
    op.b1 = (float)beta1;
    op.omb1 = (float)(1.0 - beta1);
    op.b2 = (float)beta2;
    op.omb2 = (float)(1.0 - beta2);
    op.eps = (float)epsilon.value_or(rule_id == mnistx::OPT_LAMB ? 1e-6 : 1e-8);
    op.log_b1 = beta1 > 0 ? std::log(beta1) : -1e300;   // beta = 0: b^t = 0, the correction is 1
    op.log_b2 = beta2 > 0 ? std::log(beta2) : -1e300;
  } else if (rule_id == mnistx::OPT_RMSPROP) {
    op.b2 = (float)rmsprop_decay;
    op.omb2 = (float)(1.0 - rmsprop_decay);
    op.eps = (float)epsilon.value_or(1e-10);
  } else if (rule_id == mnistx::OPT_LARS) {
    op.eps = (float)epsilon.value_or(0.0);
  }
  if (guard.has_value() && guard->defined()) {   // PS push guard: int64 stamp on the device
    check(*guard, at::kLong, 1, "guard");
    TORCH_CHECK(guard_err.has_value() && guard_err->defined(), "guard needs guard_err");
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
    TORCH_CHECK(gnorm.has_value() && gnorm->defined(), "fused_optimizer: clip_norm needs gnorm");
    TORCH_CHECK(!(guard.has_value() && guard->defined()),
                "fused_optimizer: clip_norm cannot be combined with a push guard (parameter-server mode)");
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
    TORCH_CHECK(!(guard.has_value() && guard->defined()), "fused_optimizer: rule '", rule,
                "' cannot be combined with a push guard (parameter-server mode)");
    TORCH_CHECK(tnorm.has_value() && tnorm->defined(), "fused_optimizer: rule '", rule, "' needs tnorm");
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
    TORCH_CHECK(N > 0 && h >= 1 && h <= 31 && (1ll << (2 * h)) >= N, "perm: bad domain");
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
    TORCH_CHECK(mom.has_value() && mom->defined() && slot2.has_value() && slot2->defined() && step.has_value() &&
                    step->defined(), "var_norms: lamb needs mom, slot2 and step");
    check(*mom, at::kFloat, total, "mom");
    check(*slot2, at::kFloat, total, "slot2");
    check(*step, at::kLong, 1, "step");
    TORCH_CHECK(mom->device() == params.device() && slot2->device() == params.device() &&
                    step->device() == params.device(), "mom / slot2 / step: on the parameters' device");
    TORCH_CHECK(beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1, "lamb: beta1, beta2 in [0, 1)");
    op.b1 = (float)beta1;
    op.omb1 = (float)(1.0 - beta1);
    op.b2 = (float)beta2;
    op.omb2 = (float)(1.0 - beta2);
    op.log_b1 = beta1 > 0 ? std::log(beta1) : -1e300;
    op.log_b2 = beta2 > 0 ? std::log(beta2) : -1e300;
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

// The exponent start table of a limits tensor (summary.hip), built from its host copy once: the
// order and size checks and the one download happen when a tensor (or a changed version of it) is
// first seen.  An entry holds its limits tensor, so the address cannot be reused while it is cached.
struct SummaryLimits {
  Tensor limits, start;
  uint32_t version;
};
Tensor summary_start(const Tensor& limits) {
  // never destroyed: device tensors must not be freed after the runtime has shut down
  static std::vector<SummaryLimits>& cache = *new std::vector<SummaryLimits>();
  const bool versioned = !limits.is_inference();   // an inference tensor has no version: checked every time
  const uint32_t ver = versioned ? limits._version() : 0u;
  for (const auto& c : cache)
    if (versioned && c.limits.data_ptr() == limits.data_ptr() && c.limits.numel() == limits.numel() &&
        c.version == ver)
      return c.start;
  const int64_t NB = limits.numel();
  TORCH_CHECK_VALUE(NB >= 2 && NB <= mnistx::SUMMARY_MAX_LIMITS, "limits: needs 2 <= NB <= ",
                    mnistx::SUMMARY_MAX_LIMITS, ", has ", NB);
  const Tensor h = limits.cpu();
  const double* p = h.data_ptr<double>();
  for (int64_t i = 0; i < NB; ++i) {
    TORCH_CHECK_VALUE(std::isfinite(p[i]), "limits: must be finite");
    TORCH_CHECK_VALUE(i == 0 || p[i - 1] < p[i], "limits: must be strictly ascending");
  }
  Tensor tab = at::empty({512}, at::TensorOptions().dtype(at::kShort));
  mnistx::summary_start_table(p, (int)NB, reinterpret_cast<uint16_t*>(tab.data_ptr()));
  if (cache.size() >= 4) cache.erase(cache.begin());
  cache.push_back({limits, tab.to(limits.device()), ver});
  return cache.back().start;
}

// counts [nseg, NB + 1] / stats [nseg, 4] = min, max, sum, sum of squares of every segment
// (offset, rows, cols, row_stride) of src against the ascending float64 limits (launchers.h).
void summary_stats(Tensor src, Tensor segs, Tensor limits, Tensor counts, Tensor stats, Tensor scratch,
                   double divisor) {
  TORCH_CHECK_VALUE(src.is_cuda() && src.is_contiguous(), "src: a contiguous GPU tensor");
  const bool bf = src.scalar_type() == at::kBFloat16;
  TORCH_CHECK_VALUE(bf || src.scalar_type() == at::kFloat, "src: expected float32 or bfloat16, got ",
                    src.scalar_type());
  TORCH_CHECK_VALUE(!segs.is_cuda() && segs.scalar_type() == at::kLong && segs.dim() == 2 && segs.size(1) == 4 &&
                        segs.is_contiguous(), "segs: CPU int64 [n,4] = (offset, rows, cols, row_stride)");
  TORCH_CHECK_VALUE(limits.is_cuda() && limits.scalar_type() == at::kDouble && limits.dim() == 1 &&
                        limits.is_contiguous(), "limits: a contiguous float64 [NB] GPU tensor");
  const int64_t nseg = segs.size(0), NB = limits.numel(), total = src.numel();
  TORCH_CHECK_VALUE(std::isfinite(divisor) && (float)divisor > 0.f && std::isfinite((float)divisor),
                    "divisor: must be finite and > 0");
  TORCH_CHECK_VALUE(nseg < (int64_t)1 << 20, "segs: too many segments");
  std::vector<mnistx::SummarySeg> sv(nseg);
  auto a = segs.accessor<int64_t, 2>();
  for (int64_t i = 0; i < nseg; ++i) {
    mnistx::SummarySeg& s = sv[i];
    s.off = a[i][0];
    s.rows = a[i][1];
    s.cols = a[i][2];
    s.stride = a[i][3];
    TORCH_CHECK_VALUE(s.off >= 0 && s.rows >= 0 && s.cols >= 0 && s.stride >= 0, "segment ", i, ": negative field");
    TORCH_CHECK_VALUE(s.cols <= s.stride, "segment ", i, ": cols ", s.cols, " > row_stride ", s.stride);
    TORCH_CHECK_VALUE(s.rows < ((int64_t)1 << 31) && s.cols < ((int64_t)1 << 31) && s.stride < ((int64_t)1 << 31) &&
                          s.rows * s.cols < ((int64_t)1 << 31), "segment ", i, ": 2^31 elements or more");
    if (s.rows > 0 && s.cols > 0)
      TORCH_CHECK_VALUE(s.off <= total && span(s.rows, s.stride, s.cols) <= total - s.off, "segment ", i,
                        ": ends past src (", total, " elements)");
  }
  TORCH_CHECK_VALUE(counts.is_cuda() && counts.scalar_type() == at::kInt && counts.is_contiguous() &&
                        counts.numel() >= nseg * (NB + 1), "counts: a contiguous int32 GPU tensor of nseg * (NB + 1)");
  TORCH_CHECK_VALUE(stats.is_cuda() && stats.scalar_type() == at::kDouble && stats.is_contiguous() &&
                        stats.numel() >= nseg * 4, "stats: a contiguous float64 GPU tensor of nseg * 4");
  TORCH_CHECK_VALUE(scratch.is_cuda() && scratch.scalar_type() == at::kDouble && scratch.is_contiguous() &&
                        scratch.numel() >= mnistx::summary_scratch_size((int)nseg),
                    "scratch: a contiguous float64 GPU tensor of summary_scratch_size(nseg) = ",
                    mnistx::summary_scratch_size((int)nseg));
  TORCH_CHECK_VALUE(limits.device() == src.device() && counts.device() == src.device() &&
                        stats.device() == src.device() && scratch.device() == src.device(),
                    "limits / counts / stats / scratch: on the source's device");
  const Tensor start = summary_start(limits);
  hip_ok(mnistx::summary_stats(src.data_ptr(), bf, sv.data(), (int)nseg, P<const double>(limits),
                               reinterpret_cast<const uint16_t*>(start.data_ptr()), (int)NB, (float)divisor,
                               P<int>(counts), P<double>(stats), P<double>(scratch), cur_stream()),
         "summary_stats");
}

// Confusion matrix, rank histogram and calibration sums of logits[:nb] added to acc_i / acc_f
// (eval_metrics.hip; the layout is eval_metrics_layout's).  Every refusal is a ValueError raised
// before anything is launched.
void eval_metrics(Tensor logits, optional<Tensor> labels, int64_t nb, int64_t n_classes, Tensor acc_i, Tensor acc_f,
                  Tensor scratch, optional<Tensor> rows, double temperature, int64_t n_bins) {
  TORCH_CHECK_VALUE(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2,
                    "logits: a contiguous 2-D GPU tensor [B, ld], got ", logits.dim(), " dimension(s)");
  const bool bf = logits.scalar_type() == at::kBFloat16;
  TORCH_CHECK_VALUE(bf || logits.scalar_type() == at::kFloat, "logits: expected float32 or bfloat16, got ",
                    logits.scalar_type());
  const int64_t B = logits.size(0), ld = logits.size(1);
  TORCH_CHECK_VALUE(n_classes >= 2 && n_classes <= mnistx::EVAL_MAX_CLASSES, "n_classes: needs 2 <= NC <= ",
                    mnistx::EVAL_MAX_CLASSES, ", got ", n_classes);
  TORCH_CHECK_VALUE(n_classes <= ld, "n_classes: ", n_classes, " > the logits' row length ", ld);
  TORCH_CHECK_VALUE(nb >= 0 && nb <= B, "nb: needs 0 <= nb <= B = ", B, ", got ", nb);
  TORCH_CHECK_VALUE(B < ((int64_t)1 << 31) - 256, "logits: 2^31 rows or more");
  TORCH_CHECK_VALUE(std::isfinite(temperature) && temperature > 0.0 && (float)temperature > 0.f &&
                        std::isfinite((float)temperature) && std::isfinite(1.0f / (float)temperature),
                    "temperature: must be finite and > 0 (and so must 1 / T in fp32), got ", temperature);
  TORCH_CHECK_VALUE(n_bins >= 1 && n_bins <= mnistx::EVAL_MAX_BINS, "n_bins: needs 1 <= NB <= ",
                    mnistx::EVAL_MAX_BINS, ", got ", n_bins);
  const mnistx::EvalLayout lay = mnistx::eval_metrics_layout((int)n_classes, (int)n_bins);
  const int32_t* lab = nullptr;
  if (labels.has_value() && labels->defined()) {
    TORCH_CHECK_VALUE(labels->is_cuda() && labels->scalar_type() == at::kInt && labels->is_contiguous() &&
                          labels->numel() >= nb && labels->device() == logits.device(),
                      "labels: a contiguous int32 tensor of at least nb = ", nb, " elements on the logits' device, has ",
                      labels->numel(), " of ", labels->scalar_type());
    lab = P<const int32_t>(*labels);
  }
  TORCH_CHECK_VALUE(acc_i.is_cuda() && acc_i.scalar_type() == at::kLong && acc_i.is_contiguous() &&
                        acc_i.numel() >= lay.size_i,
                    "acc_i: a contiguous int64 GPU tensor of ", lay.size_i, " elements, has ", acc_i.numel(), " of ",
                    acc_i.scalar_type());
  TORCH_CHECK_VALUE(acc_f.is_cuda() && acc_f.scalar_type() == at::kDouble && acc_f.is_contiguous() &&
                        acc_f.numel() >= lay.size_f,
                    "acc_f: a contiguous float64 GPU tensor of ", lay.size_f, " elements, has ", acc_f.numel(), " of ",
                    acc_f.scalar_type());
  const int64_t ns = mnistx::eval_metrics_scratch_size((int)n_bins);
  TORCH_CHECK_VALUE(scratch.is_cuda() && scratch.scalar_type() == at::kDouble && scratch.is_contiguous() &&
                        scratch.numel() >= ns,
                    "scratch: a contiguous float64 GPU tensor of eval_metrics_scratch_size(n_bins) = ", ns, ", has ",
                    scratch.numel(), " of ", scratch.scalar_type());
  int32_t* rw = nullptr;
  if (rows.has_value() && rows->defined()) {
    TORCH_CHECK_VALUE(rows->is_cuda() && rows->scalar_type() == at::kInt && rows->is_contiguous() &&
                          rows->numel() >= nb * 4 && rows->device() == logits.device() &&
                          reinterpret_cast<uintptr_t>(rows->data_ptr()) % 16 == 0,
                      "rows: a contiguous 16-byte aligned int32 tensor of at least nb * 4 = ", nb * 4,
                      " elements on the logits' device, has ", rows->numel(), " of ", rows->scalar_type());
    rw = P<int32_t>(*rows);
  }
  TORCH_CHECK_VALUE(acc_i.device() == logits.device() && acc_f.device() == logits.device() &&
                        scratch.device() == logits.device(), "acc_i / acc_f / scratch: on the logits' device");
  TORCH_CHECK_VALUE(reinterpret_cast<uintptr_t>(acc_i.data_ptr()) % 8 == 0 &&
                        reinterpret_cast<uintptr_t>(acc_f.data_ptr()) % 8 == 0 &&
                        reinterpret_cast<uintptr_t>(scratch.data_ptr()) % 8 == 0 &&
                        reinterpret_cast<uintptr_t>(logits.data_ptr()) % (bf ? 2 : 4) == 0,
                    "logits / acc_i / acc_f / scratch: must be aligned to their element size");
  if (nb == 0) return;
  hip_ok(mnistx::eval_metrics(logits.data_ptr(), bf, ld, lab, (int)nb, (int)n_classes, (float)temperature, (int)n_bins,
                              P<int64_t>(acc_i), P<double>(acc_f), P<double>(scratch), rw, cur_stream()),
         "eval_metrics");
}

pybind11::dict eval_metrics_layout(int64_t n_classes, int64_t n_bins) {
  TORCH_CHECK_VALUE(n_classes >= 2 && n_classes <= mnistx::EVAL_MAX_CLASSES, "n_classes: needs 2 <= NC <= ",
                    mnistx::EVAL_MAX_CLASSES, ", got ", n_classes);
  TORCH_CHECK_VALUE(n_bins >= 1 && n_bins <= mnistx::EVAL_MAX_BINS, "n_bins: needs 1 <= NB <= ",
                    mnistx::EVAL_MAX_BINS, ", got ", n_bins);
  const mnistx::EvalLayout l = mnistx::eval_metrics_layout((int)n_classes, (int)n_bins);
  pybind11::dict d;
  d["confusion"] = l.confusion;
  d["rank_hist"] = l.rank_hist;
  d["bin_count"] = l.bin_count;
  d["bin_correct"] = l.bin_correct;
  d["counts"] = l.counts;
  d["size_i"] = l.size_i;
  d["bin_conf_sum"] = l.bin_conf_sum;
  d["nll_sum"] = l.nll_sum;
  d["brier_sum"] = l.brier_sum;
  d["size_f"] = l.size_f;
  return d;
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
  if (loss_ema.has_value() && loss_ema->defined()) {
    check(*loss_ema, at::kFloat, 3 * n_ema, "loss_ema");
    f.loss_ema = P<float>(*loss_ema);
    f.n_ema = (int)n_ema;
  }
  if (nw > 0 && l2_ranges.has_value() && l2_ranges->defined()) {
    check(*l2_ranges, at::kInt, 3 * nw, "l2_ranges");
    f.l2r = P<const int>(*l2_ranges);
    // partials follow the nw per-weight slots (binding fused_optimizer: l2n = max track index)
  }
  f.l2base = (int)nw;
  if (ce_nblk > 0) {
    TORCH_CHECK(ce_work.has_value() && ce_work->defined() && ce_nblk <= 1024, "ce_work needed for ce_nblk > 0");
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

void cast_f32_bf16_padded(Tensor src, Tensor dst, int64_t G, int64_t I, int64_t J, int64_t Ip, int64_t Jp) {
  check(src, at::kFloat, G * I * J, "src");
  check(dst, at::kBFloat16, G * Ip * Jp, "dst");
  TORCH_CHECK(Ip >= I && Jp >= J, "padding");
  hip_ok(mnistx::cast_f32_bf16_padded(P<const float>(src), BFm(dst), (int)G, (int)I, (int)J, (int)Ip, (int)Jp,
                                      cur_stream()),
         "cast_f32_bf16_padded");
}

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

std::vector<int64_t> gemm_tile(int64_t M, int64_t N, bool wgrad) {
  int bm, bn;
  mnistx::gemm_tile((int)M, (int)N, wgrad ? 1 : 0, &bm, &bn);
  return {bm, bn};
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
  if (u8.has_value() && u8->defined()) {
    TORCH_CHECK(mnistx::convpool_u8_input(cfg), "convpool: uint8 input only for first layers (Cin 1, or 3 at 28x28)");
    TORCH_CHECK(idx.has_value() && idx->defined(), "convpool: uint8 input needs idx");
    check(*u8, at::kByte, hwc, "u8");
    TORCH_CHECK(u8->numel() % hwc == 0 && u8->numel() < (int64_t)INT32_MAX,
                "u8: [n, H*W*C] images, < 2 GB (the kernels address it through one buffer resource)");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(u8->data_ptr()) % 4 == 0, "u8 must be 4-byte aligned");
    check(*idx, at::kLong, B, "idx");
    src.u8 = P<const uint8_t>(*u8);
    src.idx = P<const int64_t>(*idx);
    src.n = (int)(u8->numel() / hwc);       // the kernel clamps every index into [0, n)
  } else if (idx.has_value() && idx->defined()) {
    // x is the resident bf16 dataset [n, H*W*C] (normalised once), gathered through idx
    TORCH_CHECK(mnistx::convpool_u8_input(cfg), "convpool: dataset input only for first layers (Cin 1, or 3 at 28x28)");
    check(x, at::kBFloat16, hwc, "x (dataset)");
    TORCH_CHECK(x.numel() % hwc == 0 && x.numel() * 2 < (int64_t)INT32_MAX,
                "x (dataset): [n, H*W*C] bf16 images, < 2 GB (one buffer resource)");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 8 == 0, "x (dataset) must be 8-byte aligned");
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
  if (lrn_out.has_value() && lrn_out->defined()) {
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
  if (lrn_p.has_value() && lrn_p->defined()) {
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

// LeNet-5 conv1+pool1+conv2+pool2 forward on banded MFMA tiles (lenet_band.hip).
// x: bf16 images [n, 784] gathered through idx, or the batch itself [B, 784] (idx None).
void lenet_band_fwd(Tensor x, Tensor w1, Tensor b1, int64_t b1n, Tensor w2, Tensor b2, int64_t B, Tensor p2,
                    Tensor arg2, optional<Tensor> p1, optional<Tensor> arg1, optional<Tensor> idx,
                    optional<Tensor> prof) {
  mnistx::XSrc src{nullptr, nullptr, nullptr, 0};
  if (x.scalar_type() == at::kByte) {   // uint8 images, normalised x/255 - 0.5 in the kernel
    check(x, at::kByte, 784, "x");
    TORCH_CHECK(x.numel() % 784 == 0 && x.numel() < (int64_t)INT32_MAX, "x: [n, 784] uint8 images, < 2 GB");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 4 == 0, "x must be 4-byte aligned");
    src.u8 = P<const uint8_t>(x);
  } else {
    check(x, at::kBFloat16, 784, "x");
    TORCH_CHECK(x.numel() % 784 == 0 && x.numel() * 2 < (int64_t)INT32_MAX, "x: [n, 784] bf16 images, < 2 GB");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, "x must be 16-byte aligned");
    src.x = BF(x);
  }
  src.n = (int)(x.numel() / 784);
  if (idx.has_value() && idx->defined()) {
    check(*idx, at::kLong, B, "idx");
    src.idx = P<const int64_t>(*idx);
  } else {
    TORCH_CHECK(src.n >= B, "x: needs B images without idx");
  }
  check(w1, at::kBFloat16, 5 * 5 * 8, "w1");
  check(b1, at::kFloat, b1n, "b1");
  TORCH_CHECK(b1n >= 0 && b1n <= 8, "b1n");
  check(w2, at::kBFloat16, 5 * 5 * 8 * 16, "w2");
  check(b2, at::kFloat, 16, "b2");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(w1.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(w2.data_ptr()) % 16 == 0,
              "w1 / w2 must be 16-byte aligned");
  check(p2, at::kBFloat16, B * 400, "p2");
  check(arg2, at::kByte, B * 400, "arg2");
  mnistx::bf16_t* pp1 = nullptr;
  uint8_t* pa1 = nullptr;
  if (p1.has_value() && p1->defined()) {   // with arg1: the convpool layouts; without: combined records
    check(*p1, at::kBFloat16, B * 14 * 14 * 8, "p1");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(p1->data_ptr()) % 16 == 0, "p1 must be 16-byte aligned");
    pp1 = BFm(*p1);
    if (arg1.has_value() && arg1->defined()) {
      check(*arg1, at::kByte, B * 14 * 14 * 4, "arg1");
      pa1 = P<uint8_t>(*arg1);
    }
  }
  unsigned long long* pr = nullptr;
  if (prof.has_value() && prof->defined()) {   // experiments: int64[4] clock sums
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
  mnistx::XSrc src{nullptr, nullptr, nullptr, 0};
  if (x.scalar_type() == at::kByte) {
    check(x, at::kByte, 784, "x");
    TORCH_CHECK(x.numel() % 784 == 0 && x.numel() < (int64_t)INT32_MAX, "x: [n, 784] uint8 images, < 2 GB");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 4 == 0, "x must be 4-byte aligned");
    src.u8 = P<const uint8_t>(x);
  } else {
    check(x, at::kBFloat16, 784, "x");
    TORCH_CHECK(x.numel() % 784 == 0 && x.numel() * 2 < (int64_t)INT32_MAX, "x: [n, 784] bf16 images, < 2 GB");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 8 == 0, "x must be 8-byte aligned");
    src.x = BF(x);
  }
  src.n = (int)(x.numel() / 784);
  if (idx.has_value() && idx->defined()) {
    check(*idx, at::kLong, B, "idx");
    src.idx = P<const int64_t>(*idx);
  } else {
    TORCH_CHECK(src.n >= B, "x: needs B images without idx");
  }
  TORCH_CHECK(B >= 1 && B * 196 * 16 < (int64_t)INT32_MAX, "B");
  check(p1, at::kBFloat16, B * 196 * 8, "p1");
  check(dp2, at::kBFloat16, B * 400, "dp2");
  check(arg2, at::kByte, B * 400, "arg2");
  check(w2, at::kBFloat16, 5 * 5 * 8 * 16, "w2");
  for (const Tensor* t : {&p1, &dp2, &w2})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "p1 / dp2 / w2 must be 16-byte aligned");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(arg2.data_ptr()) % 8 == 0, "arg2 alignment");
  const int res = mnistx::lenet_bwd_blocks((int)B);
  TORCH_CHECK(res > 0, "lenet_bwd: occupancy query failed");
  TORCH_CHECK(grid >= 1 && grid <= res, "lenet_bwd: grid must be in [1, ", res, "] (one block per CU, <= tiles)");
  check(slab1, at::kFloat, grid * 32 * 8, "slab1");
  check(slab2, at::kFloat, grid * 208 * 16, "slab2");
  unsigned long long* pr = nullptr;
  if (prof.has_value() && prof->defined()) {
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
  TORCH_CHECK(cin == 1 || !(u8.has_value() && u8->defined()),
              "refc1_wgrad: 3 channels read bf16 (the batch, or the dataset through idx) only");
  const auto src = cp_src(x, u8, idx, cfg, B, 784 * cin);
  if (src.x) TORCH_CHECK(reinterpret_cast<uintptr_t>(src.x) % 8 == 0, "x must be 8-byte aligned");
  const int64_t np = B * 196 * 32;
  check(dn, at::kBFloat16, np, "dn");
  check(p1, at::kBFloat16, np, "p1");
  check(arg, at::kByte, np, "arg");
  for (const Tensor* t : {&dn, &p1})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "dn / p1 must be 16-byte aligned");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(arg.data_ptr()) % 8 == 0, "arg must be 8-byte aligned");
  TORCH_CHECK(lrn_beta == 0.75, "refc1_wgrad: LRN beta 0.75 only");
  const int res = mnistx::refc1_wgrad_blocks((int)B);
  TORCH_CHECK(res > 0, "refc1_wgrad: occupancy query failed");
  TORCH_CHECK(grid >= 1 && grid <= res, "refc1_wgrad: grid must be in [1, ", res, "] (one block per CU, <= tiles)");
  check(slab, at::kFloat, grid * (cin == 1 ? 48 : 80) * 32, "slab");
  hip_ok(mnistx::refc1_wgrad(src, BF(dn), BF(p1), P<const uint8_t>(arg), (int)B, (float)lrn_bias, (float)lrn_alpha,
                             (float)lrn_beta, P<float>(slab), (int)grid, cur_stream(), (int)cin),
         "refc1_wgrad");
}

// ---------------------------------------------------------------- fp32 (reference precision) path
const float* Fo(const optional<Tensor>& t, int64_t need, const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
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
  TORCH_CHECK(((uintptr_t)y.data_ptr() % 16) == 0 && ((uintptr_t)arg.data_ptr() % 4) == 0, "y / arg alignment");
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
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "x / dn / p1 / codes must be 16-byte aligned");
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

void f32_softmax_ce(Tensor logits, int64_t ldl, optional<Tensor> labels, int64_t B, int64_t NC, double scale,
                    optional<Tensor> dlogits, int64_t ldd, optional<Tensor> stats, optional<Tensor> probs,
                    optional<Tensor> work, double label_smoothing, optional<Tensor> teacher_logits, int64_t teacher_ld,
                    double distill_alpha, double distill_temperature) {
  const float eps = smoothing_arg(label_smoothing, "f32_softmax_ce");
  const DistillArgs ds = distill_args(teacher_logits, teacher_ld, distill_alpha, distill_temperature, B, NC, logits, eps,
                                      false, false, "f32_softmax_ce");
  TORCH_CHECK_VALUE(!ds.on || (labels.has_value() && labels->defined()), "f32_softmax_ce: teacher_logits needs labels");
  TORCH_CHECK(ldl >= NC, "ldl < NC");
  check(logits, at::kFloat, span(B, ldl, NC), "logits");
  const int32_t* lab = nullptr;
  if (labels.has_value() && labels->defined()) {
    check(*labels, at::kInt, B, "labels");
    lab = P<const int32_t>(*labels);
  }
  float* dl = nullptr;
  if (dlogits.has_value() && dlogits->defined()) {
    TORCH_CHECK(lab != nullptr && ldd >= NC, "dlogits needs labels and ldd >= NC");
    check(*dlogits, at::kFloat, B * ldd, "dlogits");
    dl = P<float>(*dlogits);
  }
  float* st = nullptr;
  if (stats.has_value() && stats->defined()) {
    check(*stats, at::kFloat, 8, "stats");
    st = P<float>(*stats);
  }
  float* pr = nullptr;
  if (probs.has_value() && probs->defined()) {
    check(*probs, at::kFloat, B * NC, "probs");
    pr = P<float>(*probs);
  }
  float* wk = nullptr;
  if (work.has_value() && work->defined()) {
    check(*work, at::kFloat, mnistx::CE_WORK_FLOATS, "work");
    wk = P<float>(*work);
  }
  TORCH_CHECK(eps == 0.f || lab != nullptr, "f32_softmax_ce: label_smoothing needs labels");
  hip_ok(mnistx::f32_softmax_ce(P<const float>(logits), (int)ldl, lab, (int)B, (int)NC, (float)scale, dl, (int)ldd,
                                st, pr, wk, cur_stream(), eps, ds.on ? &ds.d : nullptr),
         "f32_softmax_ce");
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

PYBIND11_MODULE(_kernels, m) {
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
  m.def("f32_softmax_ce", &f32_softmax_ce, py::arg("logits"), py::arg("ldl"), py::arg("labels"), py::arg("B"),
        py::arg("NC"), py::arg("scale"), py::arg("dlogits"), py::arg("ldd"), py::arg("stats"), py::arg("probs"),
        py::arg("work") = py::none(), py::arg("label_smoothing") = 0.0, py::arg("teacher_logits") = py::none(), py::arg("teacher_ld") = 0,
        py::arg("distill_alpha") = 0.0, py::arg("distill_temperature") = 1.0);
  m.def("f32_prep_images", &f32_prep_images);
  // test hook: cap every persistent kernel's grid (0 = off) so small-batch oracle tests run
  // the multi-iteration (several tiles per block) paths the benchmark batches run
  m.def("set_grid_cap", [](int64_t n) { mnistx::set_grid_cap((int)n); });
  // pin / unpin host memory the caller mapped itself (the PS shm data plane's slots, so the
  // worker's gradient / parameter copies are DMA, not staged through a bounce buffer)
  m.def("host_register", [](uintptr_t addr, int64_t nbytes) {
    return hipHostRegister((void*)addr, (size_t)nbytes, hipHostRegisterDefault) == hipSuccess;
  });
  m.def("host_unregister", [](uintptr_t addr) { return hipHostUnregister((void*)addr) == hipSuccess; });
  m.def("set_gemm256", &mnistx::set_gemm256, "route the GEMMs that fill the GPU to gemm256.hip (A/B switch)");
  m.def("gemm256_enabled", &mnistx::gemm256_enabled);
  m.def("set_gemm256_debug", [](int64_t b) { mnistx::set_gemm256_debug((int)b); });
  m.def("set_reserve_cus", [](int64_t n) { mnistx::set_reserve_cus((int)n); });
  m.def("reserve_cus", []() { return (int64_t)mnistx::reserve_cus(); });
  m.def("clock_mark", [](Tensor out, int64_t slot) {
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kLong && out.is_contiguous() && slot >= 0 &&
                    slot < out.numel(), "clock_mark: int64 GPU buffer with the slot in range");
    hip_ok(mnistx::clock_mark((uint64_t*)out.data_ptr<int64_t>(), (int)slot, cur_stream()), "clock_mark");
  });
  m.def("coresidency_probe", [](Tensor out, int64_t blocks, int64_t threads, int64_t lds_bytes, int64_t spin_ticks) {
    TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kLong && out.is_contiguous() && out.numel() >= 2 * blocks,
                "coresidency_probe: int64 GPU buffer of 2 * blocks stamps");
    hip_ok(mnistx::coresidency_probe((uint64_t*)out.data_ptr<int64_t>(), (int)blocks, (int)threads, (int)lds_bytes,
                                     (int)spin_ticks, cur_stream()), "coresidency_probe");
  });
  m.def("grid_cap", []() { return (int64_t)mnistx::grid_cap(); });
  m.doc() = "MI355X (gfx950) HIP kernels for the MNIST trainer";
  m.def("dense_fwd", &dense_fwd, py::arg("x"), py::arg("w"), py::arg("out"), py::arg("M"), py::arg("N"), py::arg("K"),
        py::arg("ldx"), py::arg("ldw"), py::arg("ldc"), py::arg("bias"), py::arg("bias_n"), py::arg("relu"),
        py::arg("mask"), py::arg("ldm"), py::arg("tile") = -1);
  m.def("dense_dgrad", &dense_dgrad, py::arg("dy"), py::arg("w"), py::arg("out"), py::arg("M"), py::arg("N"),
        py::arg("K"), py::arg("lddy"), py::arg("ldw"), py::arg("ldc"), py::arg("mask"), py::arg("ldm"),
        py::arg("tile") = -1);
  m.def("set_tile192", [](int64_t on) { mnistx::set_tile192((int)on); },
        "A/B switch of gemm.hip's 192-column tiles (MNISTX_TILE192)");
  m.def("set_reduce_fused", [](int64_t on) { mnistx::set_reduce_fused((int)on); },
        "A/B switch of the one-launch split-K reduce (MNISTX_REDUCE_FUSED)");
  m.def("reduce_fused_enabled", []() { return mnistx::reduce_fused_enabled() != 0; });
  m.def("dense_wgrad", &dense_wgrad, py::arg("x"), py::arg("dy"), py::arg("slab"), py::arg("Din"), py::arg("Dout"),
        py::arg("B"), py::arg("ldx"), py::arg("lddy"), py::arg("with_bias"), py::arg("splits"), py::arg("tile") = -1);
  m.def("conv_fwd", &conv_fwd, py::arg("x"), py::arg("w"), py::arg("out"), py::arg("Nb"), py::arg("H"), py::arg("W"),
        py::arg("C"), py::arg("OH"), py::arg("OW"), py::arg("KH"), py::arg("KW"), py::arg("ph"), py::arg("pw"),
        py::arg("Cout"), py::arg("bias"), py::arg("bias_n"), py::arg("relu"), py::arg("lrn_r") = 0,
        py::arg("lrn_bias") = 0.0, py::arg("lrn_alpha") = 0.0, py::arg("lrn_beta") = 0.0);
  m.def("set_f32_halo_fwd_variant", [](int64_t v) { mnistx::set_f32_halo_fwd_variant((int)v); });
  m.def("set_halo_variants", [](int64_t f, int64_t d) { mnistx::set_halo_variants((int)f, (int)d); });
  m.def("conv_dgrad", &conv_dgrad);
  m.def("conv_wgrad", &conv_wgrad, py::arg("x"), py::arg("dy"), py::arg("slab"), py::arg("Nb"), py::arg("H"),
        py::arg("W"), py::arg("C"), py::arg("OH"), py::arg("OW"), py::arg("KH"), py::arg("KW"), py::arg("ph"),
        py::arg("pw"), py::arg("Cout"), py::arg("with_bias"), py::arg("splits"), py::arg("lrn_r") = 0,
        py::arg("lrn_bias") = 0.0, py::arg("lrn_alpha") = 0.0, py::arg("lrn_beta") = 0.0);
  m.def("prep_images", &prep_images);
  m.def("dense_wgrad_group", &dense_wgrad_group);
  m.def("conv_wgrad_pref_splits", &conv_wgrad_pref_splits);
  m.def("perm_positions", &perm_positions, py::arg("out"), py::arg("start"), py::arg("N"), py::arg("seed"), py::arg("h"),
        py::arg("lab_src") = py::none(), py::arg("lab_out") = py::none());
  m.def("prep_images_perm", &prep_images_perm);
  m.def("maxpool_fwd", &maxpool_fwd);
  m.def("maxpool_bwd", &maxpool_bwd);
  m.def("lrn_fwd", &lrn_fwd);
  m.def("lrn_bwd", &lrn_bwd);
  m.def("lrn_pool_supported", &lrn_pool_supported);
  m.def("lrn_pool_fwd", &lrn_pool_fwd, py::arg("x"), py::arg("y"), py::arg("arg"), py::arg("Nb"), py::arg("H"),
        py::arg("W"), py::arg("C"), py::arg("r"), py::arg("bias"), py::arg("alpha"), py::arg("beta"),
        py::arg("nonneg") = false);
  m.def("lrn_set_packed", [](bool on) { mnistx::lrn_set_packed(on ? 1 : 0); });
  m.def("lrn_pool_bwd", &lrn_pool_bwd);
  m.def("softmax_ce", &softmax_ce, py::arg("logits"), py::arg("ldl"), py::arg("labels"), py::arg("B"), py::arg("NC"),
        py::arg("scale"), py::arg("dlogits"), py::arg("ldd"), py::arg("stats"), py::arg("probs"),
        py::arg("work") = py::none(), py::arg("defer_stats") = false, py::arg("dbias") = py::none(),
        py::arg("label_smoothing") = 0.0, py::arg("labels2") = py::none(), py::arg("lam") = py::none(), py::arg("teacher_logits") = py::none(), py::arg("teacher_ld") = 0,
        py::arg("distill_alpha") = 0.0, py::arg("distill_temperature") = 1.0);
  m.def("softmax_ce_dbias_blocks",
        [](int64_t B, int64_t ldl) { return (int64_t)mnistx::softmax_ce_dbias_blocks((int)B, (int)ldl); });
  m.def("splitk_reduce", &splitk_reduce);
  m.def("splitk_reduce_multi", &splitk_reduce_multi);
  m.def("mlp_head_supported", &mlp_head_supported);
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
  m.def("augment_images", &augment_images, py::arg("src"), py::arg("idx"), py::arg("lab_src"), py::arg("out"),
        py::arg("lab_out"), py::arg("Csrc"), py::arg("Cdst"), py::arg("pos0"), py::arg("seed"), py::arg("shift"),
        py::arg("rotate"), py::arg("scale"), py::arg("elastic_alpha") = 0.0, py::arg("elastic_weights") = py::none());
  m.def("augment_elastic_draws", &augment_elastic_draws, py::arg("out"), py::arg("pos0"), py::arg("seed"));
  m.def("augment_elastic_field", &augment_elastic_field, py::arg("out"), py::arg("pos0"), py::arg("seed"),
        py::arg("elastic_alpha"), py::arg("elastic_weights"));
  m.def("mix_images", &mix_images, py::arg("images"), py::arg("labels"), py::arg("labels2"), py::arg("lam"),
        py::arg("nb"), py::arg("cdst"), py::arg("pos0"), py::arg("seed"), py::arg("thr_p"),
        py::arg("lam_table") = py::none(), py::arg("side_table") = py::none());
  m.def("mix_params", &mix_params, py::arg("out"), py::arg("pos0"), py::arg("seed"), py::arg("thr_p"),
        py::arg("lam_table") = py::none(), py::arg("side_table") = py::none());
  m.def("augment_params", &augment_params, py::arg("out"), py::arg("pos0"), py::arg("seed"), py::arg("shift"),
        py::arg("rotate"), py::arg("scale"));
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
  m.def("lr_at_steps", &lr_at_steps, py::arg("steps"), py::arg("out"), py::arg("lr0"), py::arg("decay_rate"),
        py::arg("decay_steps"), py::kw_only(), py::arg("lr_schedule") = "staircase", py::arg("warmup_steps") = 0,
        py::arg("lr_total_steps") = 0, py::arg("lr_end") = 0.0, py::arg("lr_power") = 1.0,
        "out[i] = the learning rate the optimizer launch applies at global step steps[i] (the device's own function)");
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
  m.def("summary_stats", &summary_stats, py::arg("src"), py::arg("segs"), py::arg("limits"), py::arg("counts"),
        py::arg("stats"), py::arg("scratch"), py::arg("divisor") = 1.0,
        "per segment (offset, rows, cols, row_stride) of src: counts[s, lower_bound(limits, v / divisor)] "
        "(column NB: NaN, +-inf, above the last limit) and stats[s] = min, max, sum, sum of squares");
  m.def("summary_scratch_size", [](int64_t nseg) { return (int64_t)mnistx::summary_scratch_size((int)nseg); });
  m.def("summary_max_blocks", []() { return (int64_t)mnistx::summary_max_blocks(); });
  m.def("eval_metrics", &eval_metrics, py::arg("logits"), py::arg("labels"), py::arg("nb"), py::arg("n_classes"),
        py::arg("acc_i"), py::arg("acc_f"), py::arg("scratch"), py::arg("rows") = py::none(),
        py::arg("temperature") = 1.0, py::arg("n_bins") = 15,
        "adds the confusion matrix, rank histogram, reliability bins and NLL / Brier sums of logits[:nb] to "
        "acc_i (int64) / acc_f (float64), laid out as eval_metrics_layout says; rows [B, 4] int32: per-row "
        "(pred, rank, bin, bits of conf)");
  m.def("eval_metrics_layout", &eval_metrics_layout, py::arg("n_classes"), py::arg("n_bins") = 15,
        "offsets of every accumulator in acc_i / acc_f, and their sizes size_i / size_f");
  m.def("eval_metrics_scratch_size", [](int64_t n_bins) {
    TORCH_CHECK_VALUE(n_bins >= 1 && n_bins <= mnistx::EVAL_MAX_BINS, "n_bins: needs 1 <= NB <= ",
                      mnistx::EVAL_MAX_BINS, ", got ", n_bins);
    return (int64_t)mnistx::eval_metrics_scratch_size((int)n_bins);
  }, py::arg("n_bins") = 15);
  m.def("eval_metrics_max_blocks", []() { return (int64_t)mnistx::eval_metrics_max_blocks(); });
  m.def("set_opt_fin_fused", [](int64_t on) { mnistx::set_opt_fin_fused((int)on); },
        "A/B switch of the optimizer launch running the step's finalize (MNISTX_OPT_FIN_FUSED)");
  m.def("opt_fin_fused_enabled", []() { return mnistx::opt_fin_fused_enabled() != 0; });
  m.def("fused_optimizer_blocks", [](Tensor segs) {
    TORCH_CHECK(!segs.is_cuda() && segs.scalar_type() == at::kLong && segs.dim() == 2, "segs: CPU int64 [n,14]");
    auto a = segs.accessor<int64_t, 2>();
    std::vector<mnistx::OptSeg> sv(segs.size(0));
    for (int64_t i = 0; i < segs.size(0); ++i) sv[i].n = a[i][1];
    return (int64_t)mnistx::fused_optimizer_blocks(sv.data(), (int)sv.size());
  });
  m.def("finalize_step", &finalize_step, py::arg("step"), py::arg("stats"), py::arg("l2"), py::arg("wds"),
        py::arg("nw"), py::arg("loss_ema"), py::arg("n_ema"), py::arg("batch"), py::arg("increment"),
        py::arg("l2_ranges") = py::none(), py::arg("ce_work") = py::none(), py::arg("ce_nblk") = 0);
  m.def("mlp_head_blocks", [](int64_t nb) { return (int64_t)mnistx::mlp_head_blocks((int)nb); });
  m.def("cast_f32_bf16_padded", &cast_f32_bf16_padded);
  m.def("convpool_supported", &convpool_supported);
  m.def("convpool_rows", &convpool_rows);
  m.def("gemm_tile", &gemm_tile);
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
  m.def("convpool_dgrad", &convpool_dgrad, py::arg("dP"), py::arg("arg"), py::arg("w"), py::arg("dx"), py::arg("B"),
        py::arg("cin"), py::arg("cout"), py::arg("ks"), py::arg("pad"), py::arg("h"), py::arg("w_"),
        py::arg("grid_cap") = 0);
  m.def("convpool_arg_bytes", &convpool_arg_bytes);
  m.def("convpool_has_dgrad", &convpool_has_dgrad);
  m.def("convpool_wgrad_grid", &convpool_wgrad_grid);
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
  m.attr("ARCH") = "gfx950";
}
