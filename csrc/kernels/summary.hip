// TensorBoard summary statistics on the device (obs/device_summary.py, the chief's Monitor):
// for every segment of one source tensor, the histogram against an ascending table of float64
// limits plus min / max / sum / sum of squares, so that a write of the training summaries moves
// a few KB to the host instead of every weight, gradient and sampled activation.
//
//   summary_stats_k   block b walks chunks [b * per, (b + 1) * per) of the (segment, 512-element
//                     chunk) decomposition in order, as grad_sqnorm_k does.  Bucket counts go to
//                     an LDS histogram (integer atomics) whose non-zero bins are added to the
//                     global counts (integer atomics: order-independent) whenever the block leaves
//                     a segment; the moments are float64 per thread, reduced in a fixed order and
//                     stored as the (segment, block) partial in scratch.
//   summary_finish_k  one block per segment combines the partials of the blocks that walked one of
//                     its chunks, in block order.
// No float atomics, no ticket, no fence, no host sync: two calls give the same bits.
//
// A value counts in column i < NB when it is finite and i is its lower_bound index in limits (the
// first i with limits[i] >= v); NaN, +-inf and finite values above limits[NB - 1] count in column
// NB and stay out of the moments.  The search starts from a table indexed by the fp32 exponent
// (built on the host from the limits that were passed in, summary_start_table): lower_bound is
// monotone, so the index of a value lies between those of its binade's two ends, and the binary
// search runs over that range only (TF's 1.1^k limits: at most 8 per binade).
#include "common.h"
#include "launchers.h"

#include <algorithm>

namespace mnistx {
namespace {

constexpr int SUM_TPB = 256;
constexpr int SUM_CHUNK = 512;                    // elements per chunk: two per thread
constexpr int SUM_EPT = SUM_CHUNK / SUM_TPB;
constexpr int SUM_BLOCKS = 1024;                  // grid cap = partials per segment in scratch
constexpr int SUM_GROUP = 32;                     // segments per launch (table by value)
constexpr int SUM_WAVES = SUM_TPB / 64;

struct SumSeg {
  int64_t off;
  int rows, cols, stride;
  int chunk0;          // first chunk of this segment in the launch's chunk list
  FastDiv fcols;
};
struct SumTable {
  SumSeg s[SUM_GROUP];
  int n;
  int nchunks;
  int per;             // chunks per block
  int seg0;            // index of s[0] in counts / stats / scratch
};

DEV double shfl_xor_d(double v, int o) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __shfl_xor((uint32_t)u, o, 64), hi = __shfl_xor((uint32_t)(u >> 32), o, 64);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

template <typename T>
DEV float load_val(const T* src, int64_t i);
template <>
DEV float load_val<float>(const float* src, int64_t i) { return src[i]; }
template <>
DEV float load_val<bf16_t>(const bf16_t* src, int64_t i) { return bf2f(src[i]); }

// v / d rounded once to fp32 (numpy's float32 / int), whatever the build's fp32 division and
// contraction flags: the float64 quotient of two fp32 values rounded to fp32 is the correctly
// rounded fp32 quotient (53 >= 2 * 24 + 2 bits: the second rounding never meets a new tie)
DEV float div_rn(float v, double d) { return (float)((double)v / d); }

// lower_bound of the finite value f (= v) in lim[0 .. NB): NB when f > lim[NB - 1]
DEV int bucket_of(float f, double v, const double* lim, const uint16_t* start) {
  const uint32_t bits = __float_as_uint(f);
  const int e = (bits >> 23) & 0xff;    // <= 254: f is finite
  int lo, hi;
  if (bits >> 31) {
    lo = start[256 + e + 1];
    hi = start[256 + e];
  } else {
    lo = start[e];
    hi = start[e + 1];
  }
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (lim[mid] >= v) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// scratch: per (segment, block) {min, max, sum, sum of squares}
DEV double* sum_part(double* scratch, int seg, int blk) { return scratch + ((size_t)seg * SUM_BLOCKS + blk) * 4; }

template <typename T, bool DIV>
__global__ __launch_bounds__(SUM_TPB) void summary_stats_k(const T* __restrict__ src, SumTable tab,
                                                           const double* __restrict__ limits,
                                                           const uint16_t* __restrict__ start_g, int NB, double divisor,
                                                           int* __restrict__ counts, double* __restrict__ scratch) {
  __shared__ double lim[SUMMARY_MAX_LIMITS];
  __shared__ int hist[SUMMARY_MAX_LIMITS + 1];
  __shared__ uint16_t start[512];
  __shared__ double red[4][SUM_WAVES];
  const int tid = threadIdx.x;
  for (int i = tid; i < NB; i += SUM_TPB) lim[i] = limits[i];
  for (int i = tid; i <= NB; i += SUM_TPB) hist[i] = 0;
  for (int i = tid; i < 512; i += SUM_TPB) start[i] = start_g[i];
  __syncthreads();

  const int c0 = min(tab.nchunks, (int)blockIdx.x * tab.per), c1 = min(tab.nchunks, c0 + tab.per);
  int si = 0, c = c0;
  while (c < c1) {   // block-uniform
    while (si + 1 < tab.n && c >= tab.s[si + 1].chunk0) ++si;
    const SumSeg& S = tab.s[si];
    const int n = S.rows * S.cols;                 // < 2^31 (checked by the binding)
    const int cend = min(c1, si + 1 < tab.n ? tab.s[si + 1].chunk0 : tab.nchunks);
    const bool flat = S.cols == S.stride;
    double vmin = INFINITY, vmax = -INFINITY, vsum = 0.0, vsq = 0.0;
    for (; c < cend; ++c) {
      const int lo = (c - S.chunk0) * SUM_CHUNK;
      float f[SUM_EPT];
      bool ok[SUM_EPT];
      // out-of-range elements load the segment's first element and are never counted
#pragma unroll
      for (int u = 0; u < SUM_EPT; ++u) {
        const int e = lo + u * SUM_TPB + tid;
        ok[u] = e < n;
        const int ee = ok[u] ? e : 0;
        int64_t idx = S.off + ee;
        if (!flat) {
          const int r = S.fcols.div(ee);
          idx = S.off + (int64_t)r * S.stride + (ee - r * S.cols);
        }
        f[u] = load_val<T>(src, idx);
      }
#pragma unroll
      for (int u = 0; u < SUM_EPT; ++u) {
        float x = f[u];
        if constexpr (DIV) x = div_rn(x, divisor);
        const double v = (double)x;
        int b = NB;
        if (((__float_as_uint(x) >> 23) & 0xff) != 0xff) b = bucket_of(x, v, lim, start);
        if (ok[u] && b < NB) {
          vmin = fmin(vmin, v);
          vmax = fmax(vmax, v);
          vsum += v;
          vsq += v * v;
        }
        // the lanes that share the first active lane's bin add their number at once (half of a
        // post-ReLU activation is one bin); the others add one each
        if (ok[u]) {
          const int b0 = __builtin_amdgcn_readfirstlane(b);
          const uint64_t same = __ballot(b == b0);
          if (b != b0) {
            atomicAdd(&hist[b], 1);
          } else if ((int)__lane_id() == __ffsll((long long)same) - 1) {
            atomicAdd(&hist[b0], (int)__popcll(same));
          }
        }
      }
    }
    // the block leaves segment si: its partial moments, in a fixed order, and its counts
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      vmin = fmin(vmin, shfl_xor_d(vmin, o));
      vmax = fmax(vmax, shfl_xor_d(vmax, o));
      vsum += shfl_xor_d(vsum, o);
      vsq += shfl_xor_d(vsq, o);
    }
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = vmin;
      red[1][tid >> 6] = vmax;
      red[2][tid >> 6] = vsum;
      red[3][tid >> 6] = vsq;
    }
    __syncthreads();   // also: every LDS histogram add of this segment is done
    if (tid == 0) {
      double a = red[0][0], b = red[1][0], s = red[2][0], q = red[3][0];
#pragma unroll
      for (int w = 1; w < SUM_WAVES; ++w) {
        a = fmin(a, red[0][w]);
        b = fmax(b, red[1][w]);
        s += red[2][w];
        q += red[3][w];
      }
      double* p = sum_part(scratch, tab.seg0 + si, blockIdx.x);
      p[0] = a;
      p[1] = b;
      p[2] = s;
      p[3] = q;
    }
    int* dst = counts + (size_t)(tab.seg0 + si) * (NB + 1);
    for (int i = tid; i <= NB; i += SUM_TPB) {
      const int h = hist[i];
      if (h) {
        atomicAdd(&dst[i], h);
        hist[i] = 0;
      }
    }
    __syncthreads();   // red and hist are free again
  }
}

// stats[seg] from the partials of the blocks that walked one of the segment's chunks: thread t
// takes blocks b_lo + t, b_lo + t + SUM_TPB, ... in order, then the lanes, then the waves in order
__global__ __launch_bounds__(SUM_TPB) void summary_finish_k(SumTable tab, const double* __restrict__ scratch,
                                                            double* __restrict__ stats) {
  __shared__ double red[4][SUM_WAVES];
  const int si = blockIdx.x, tid = threadIdx.x;
  const int c_lo = tab.s[si].chunk0, c_hi = si + 1 < tab.n ? tab.s[si + 1].chunk0 : tab.nchunks;
  double vmin = INFINITY, vmax = -INFINITY, vsum = 0.0, vsq = 0.0;
  if (c_hi > c_lo) {
    const int b_hi = (c_hi - 1) / tab.per;
    for (int blk = c_lo / tab.per + tid; blk <= b_hi; blk += SUM_TPB) {
      const double* p = sum_part(const_cast<double*>(scratch), tab.seg0 + si, blk);
      vmin = fmin(vmin, p[0]);
      vmax = fmax(vmax, p[1]);
      vsum += p[2];
      vsq += p[3];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    vmin = fmin(vmin, shfl_xor_d(vmin, o));
    vmax = fmax(vmax, shfl_xor_d(vmax, o));
    vsum += shfl_xor_d(vsum, o);
    vsq += shfl_xor_d(vsq, o);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = vmin;
    red[1][tid >> 6] = vmax;
    red[2][tid >> 6] = vsum;
    red[3][tid >> 6] = vsq;
  }
  __syncthreads();
  if (tid == 0) {
    double a = red[0][0], b = red[1][0], s = red[2][0], q = red[3][0];
#pragma unroll
    for (int w = 1; w < SUM_WAVES; ++w) {
      a = fmin(a, red[0][w]);
      b = fmax(b, red[1][w]);
      s += red[2][w];
      q += red[3][w];
    }
    double* d = stats + (size_t)(tab.seg0 + si) * 4;
    d[0] = a;
    d[1] = b;
    d[2] = s;
    d[3] = q;
  }
}

template <typename T>
hipError_t launch_group(const T* src, const SumTable& tab, const double* limits, const uint16_t* start, int NB,
                        float divisor, int* counts, double* scratch, double* stats, hipStream_t st) {
  if (tab.nchunks > 0) {
    const int grid = (tab.nchunks + tab.per - 1) / tab.per;
    if (divisor != 1.f)
      hipLaunchKernelGGL((summary_stats_k<T, true>), dim3(grid), dim3(SUM_TPB), 0, st, src, tab, limits, start, NB,
                         (double)divisor, counts, scratch);
    else
      hipLaunchKernelGGL((summary_stats_k<T, false>), dim3(grid), dim3(SUM_TPB), 0, st, src, tab, limits, start, NB,
                         1.0, counts, scratch);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(summary_finish_k, dim3(tab.n), dim3(SUM_TPB), 0, st, tab, scratch, stats);
  return hipGetLastError();
}

}  // namespace

int summary_max_blocks() { return SUM_BLOCKS; }
int64_t summary_scratch_size(int nseg) { return (int64_t)std::max(nseg, 0) * SUM_BLOCKS * 4; }

void summary_start_table(const double* limits, int NB, uint16_t* start) {
  auto lb = [&](double v) { return (uint16_t)(std::lower_bound(limits, limits + NB, v) - limits); };
  // [e]: the index of the smallest value >= 0 with biased exponent e (0: zero and the denormals);
  // [256 + e]: of the negative value nearest zero with that exponent; e = 255: past every finite fp32
  for (int e = 0; e < 256; ++e) {
    const double edge = e == 0 ? 0.0 : std::ldexp(1.0, e - 127);
    start[e] = lb(edge);
    start[256 + e] = lb(-edge);
  }
}

hipError_t summary_stats(const void* src, bool src_bf16, const SummarySeg* segs, int nseg, const double* limits,
                         const uint16_t* start, int NB, float divisor, int* counts, double* stats, double* scratch,
                         hipStream_t st) {
  if (nseg <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)nseg * (NB + 1) * sizeof(int), st);
  if (e != hipSuccess) return e;
  for (int g0 = 0; g0 < nseg; g0 += SUM_GROUP) {
    SumTable tab{};
    tab.n = std::min(SUM_GROUP, nseg - g0);
    tab.seg0 = g0;
    int64_t nc = 0;
    for (int i = 0; i < tab.n; ++i) {
      const SummarySeg& h = segs[g0 + i];
      SumSeg& s = tab.s[i];
      s.off = h.off;
      s.rows = (int)h.rows;
      s.cols = (int)h.cols;
      s.stride = (int)h.stride;
      s.chunk0 = (int)nc;
      s.fcols = FastDiv((uint32_t)std::max<int64_t>(h.cols, 1));
      nc += (h.rows * h.cols + SUM_CHUNK - 1) / SUM_CHUNK;   // < 2^22 each
    }
    tab.nchunks = (int)nc;
    tab.per = std::max(1, (int)((nc + SUM_BLOCKS - 1) / SUM_BLOCKS));
    e = src_bf16 ? launch_group((const bf16_t*)src, tab, limits, start, NB, divisor, counts, scratch, stats, st)
                 : launch_group((const float*)src, tab, limits, start, NB, divisor, counts, scratch, stats, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mnistx
