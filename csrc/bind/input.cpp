// _kernels bindings: the batch on its way in (permutation, image preparation, augmentation, mixup / CutMix)
// and what is read back for the observer (device summaries, evaluation metrics).
#include "bind/common.h"

namespace {

// lab_src [N] / lab_out [n] (optional, int32): gather the chosen rows' labels in the same launch
void perm_positions(Tensor out, int64_t start, int64_t N, int64_t seed, int64_t h, optional<Tensor> lab_src,
                    optional<Tensor> lab_out) {
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kLong && out.is_contiguous(), "perm_positions: out");
  perm_domain("perm_positions", N, h);
  const bool labs = has(lab_src);
  TORCH_CHECK(labs == has(lab_out), "perm_positions: lab_src and lab_out together");
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
  perm_domain("prep_images_perm", N, h);
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
  TORCH_CHECK(aligned(src, 16) && aligned(out, 16), "augment_images: src and out must be 16-byte aligned");
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
  const bool ht = has(lam_table), hs = has(side_table);
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
  TORCH_CHECK(aligned(images, 16), "mix_images: images must be 16-byte aligned");
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
  if (has(labels)) {
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
  if (has(rows)) {
    TORCH_CHECK_VALUE(rows->is_cuda() && rows->scalar_type() == at::kInt && rows->is_contiguous() &&
                          rows->numel() >= nb * 4 && rows->device() == logits.device() && aligned(*rows, 16),
                      "rows: a contiguous 16-byte aligned int32 tensor of at least nb * 4 = ", nb * 4,
                      " elements on the logits' device, has ", rows->numel(), " of ", rows->scalar_type());
    rw = P<int32_t>(*rows);
  }
  TORCH_CHECK_VALUE(acc_i.device() == logits.device() && acc_f.device() == logits.device() &&
                        scratch.device() == logits.device(), "acc_i / acc_f / scratch: on the logits' device");
  TORCH_CHECK_VALUE(aligned(acc_i, 8) && aligned(acc_f, 8) && aligned(scratch, 8) && aligned(logits, bf ? 2 : 4),
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

}  // namespace

void bind_input(py::module_& m) {
  m.def("perm_positions", &perm_positions, py::arg("out"), py::arg("start"), py::arg("N"), py::arg("seed"), py::arg("h"),
        py::arg("lab_src") = py::none(), py::arg("lab_out") = py::none());
  m.def("prep_images_perm", &prep_images_perm);
  m.def("prep_images", &prep_images);
  m.def("augment_images", &augment_images, py::arg("src"), py::arg("idx"), py::arg("lab_src"), py::arg("out"),
        py::arg("lab_out"), py::arg("Csrc"), py::arg("Cdst"), py::arg("pos0"), py::arg("seed"), py::arg("shift"),
        py::arg("rotate"), py::arg("scale"), py::arg("elastic_alpha") = 0.0, py::arg("elastic_weights") = py::none());
  m.def("augment_elastic_draws", &augment_elastic_draws, py::arg("out"), py::arg("pos0"), py::arg("seed"));
  m.def("augment_elastic_field", &augment_elastic_field, py::arg("out"), py::arg("pos0"), py::arg("seed"),
        py::arg("elastic_alpha"), py::arg("elastic_weights"));
  m.def("augment_params", &augment_params, py::arg("out"), py::arg("pos0"), py::arg("seed"), py::arg("shift"),
        py::arg("rotate"), py::arg("scale"));
  m.def("mix_images", &mix_images, py::arg("images"), py::arg("labels"), py::arg("labels2"), py::arg("lam"),
        py::arg("nb"), py::arg("cdst"), py::arg("pos0"), py::arg("seed"), py::arg("thr_p"),
        py::arg("lam_table") = py::none(), py::arg("side_table") = py::none());
  m.def("mix_params", &mix_params, py::arg("out"), py::arg("pos0"), py::arg("seed"), py::arg("thr_p"),
        py::arg("lam_table") = py::none(), py::arg("side_table") = py::none());
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
}
