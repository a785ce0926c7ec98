// Evaluation metrics on the device (obs/eval_metrics.py is the host reference and the definition):
// confusion matrix, rank histogram of the true class, reliability bins, NLL and Brier sums of a
// batch of logits, added to accumulators the caller zeroed, so that a pass over a split brings
// a few hundred bytes to the host instead of every probability row.
//
//   eval_metrics_k       block b walks the 256-row chunks [b * per, (b + 1) * per) in order; a lane
//                        owns a row and reads its NC logits with the widest vector loads the row
//                        alignment allows (16 / 8 / 4 bytes, then single elements: the columns
//                        NC .. ld - 1 are never read).  Integer counts go to an LDS table (integer
//                        atomics) that is added to the global int64 accumulators (integer atomics:
//                        order-independent) when the block is done.  The float64 sums are formed
//                        from the chunk's per-row values staged in LDS: thread t < NB adds the
//                        confidences of bin t, thread NB the NLLs, thread NB + 1 the Brier scores,
//                        each in row order, and stores its (block, t) partial in scratch.
//   eval_metrics_finish_k thread t adds the partials of entry t to acc_f[t] in block order (staged
//                        through LDS 32 blocks at a time).
// No float atomics, no ticket, no fence, no host sync: two passes from zeroed accumulators give
// the same bits.
//
// Per-row arithmetic is fp32 with every operation rounded on its own (no contraction), accurate
// expf / logf, and correctly rounded quotients.
#include "common.h"
#include "launchers.h"

#include <algorithm>

namespace mnistx {
namespace {

constexpr int EM_TPB = 256;          // rows per chunk: one per lane
constexpr int EM_BLOCKS = 1024;      // grid cap = partials per entry in scratch
constexpr int EM_FIN_TPB = 256;      // >= EVAL_MAX_BINS + 2
constexpr int EM_FIN_CHUNK = 32;     // blocks whose partials are staged at a time

// a / b rounded once to fp32: the float64 quotient of two fp32 values rounded to fp32 is the
// correctly rounded fp32 quotient (53 >= 2 * 24 + 2 bits), whatever the build's division flags
DEV float div_rn(float a, float b) { return (float)((double)a / (double)b); }

template <typename T>
struct Elem;
template <>
struct Elem<float> {
  static DEV float get(uint32_t w, int) { return __uint_as_float(w); }
};
template <>
struct Elem<bf16_t> {
  static DEV float get(uint32_t w, int half) { return half ? __uint_as_float(w & 0xffff0000u) : __uint_as_float(w << 16); }
};

// v[0 .. NC) = row[0 .. NC) widened to fp32.  vwb: the widest load in bytes (a power of two
// between sizeof(T) and 16) at which row + any multiple of it is aligned.  Level by level from
// the widest: every aligned group of that width that lies wholly below NC and past what the
// wider levels took.  c is a compile-time index after unrolling; done / NC / vwb are uniform.
template <typename T, int NCP>
DEV void load_row(const T* __restrict__ row, int NC, int vwb, float (&v)[NCP]) {
  constexpr int ES = (int)sizeof(T);
  constexpr int E16 = 16 / ES, E8 = 8 / ES, E4 = 4 / ES;
  int done = 0;
  if (vwb >= 16) {
#pragma unroll
    for (int c = 0; c + E16 <= NCP; c += E16)
      if (c + E16 <= NC) {
        const u32x4 w = *reinterpret_cast<const u32x4*>(row + c);
#pragma unroll
        for (int j = 0; j < E16; ++j) v[c + j] = Elem<T>::get(w[j * ES / 4], j & 1);
      }
    done = NC / E16 * E16;
  }
  if (vwb >= 8) {
#pragma unroll
    for (int c = 0; c + E8 <= NCP; c += E8)
      if (c >= done && c + E8 <= NC) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(row + c);
#pragma unroll
        for (int j = 0; j < E8; ++j) v[c + j] = Elem<T>::get(w[j * ES / 4], j & 1);
      }
    done = NC / E8 * E8;
  }
  if (vwb >= 4) {
#pragma unroll
    for (int c = 0; c + E4 <= NCP; c += E4)
      if (c >= done && c + E4 <= NC) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(row + c);
#pragma unroll
        for (int j = 0; j < E4; ++j) v[c + j] = Elem<T>::get(w, j & 1);
      }
    done = NC / E4 * E4;
  }
  if constexpr (ES == 2) {
#pragma unroll
    for (int c = 0; c < NCP; ++c)
      if (c >= done && c < NC) v[c] = bf2f(row[c]);
  }
}

struct EmArgs {
  const void* logits;
  const int32_t* labels;     // or null
  int64_t ld;
  int nb, NC, NB, vwb;
  int nchunks, per;          // 256-row chunks, chunks per block
  float inv_t;               // 1 / T in fp32
  EvalLayout lay;
  unsigned long long* acc_i;
  double* scratch;           // [grid][NB + 2]
  int32_t* rows;             // [B][4] or null
};

template <typename T, int NCP>
__global__ __launch_bounds__(EM_TPB) void eval_metrics_k(EmArgs a) {
  // every fp32 operation below rounds on its own: q * q + brier must not become one fma
#pragma clang fp contract(off)
  // the block's integer accumulators, laid out as acc_i (EvalLayout offsets)
  __shared__ int hist[(EVAL_MAX_CLASSES + 1) * EVAL_MAX_CLASSES + EVAL_MAX_CLASSES + 2 * EVAL_MAX_BINS + 3];
  // per row of the chunk: confidence, NLL, Brier score, bin (-1: the row adds to no float sum)
  __shared__ f32x4 stage[EM_TPB];
  const int tid = threadIdx.x;
  const int NC = a.NC, NB = a.NB;
  const int n_i = (int)a.lay.size_i;
  for (int i = tid; i < n_i; i += EM_TPB) hist[i] = 0;
  __syncthreads();

  const T* __restrict__ logits = static_cast<const T*>(a.logits);
  const int c0 = min(a.nchunks, (int)blockIdx.x * a.per), c1 = min(a.nchunks, c0 + a.per);
  int n_rows = 0, n_lab = 0, n_bad = 0;
  double part = 0.0;     // thread t's float64 entry, over the block's rows in order
  for (int ch = c0; ch < c1; ++ch) {   // block-uniform
    const int r = ch * EM_TPB + tid;   // nchunks * 256 < 2^31 (checked by the binding)
    f32x4 st = {0.f, 0.f, 0.f, __int_as_float(-1)};
    if (r < a.nb) {
      float v[NCP];
      load_row<T, NCP>(logits + (size_t)r * a.ld, NC, a.vwb, v);
      const int y0 = a.labels ? a.labels[r] : -1;
      const bool lab = y0 >= 0 && y0 < NC;
      const int y = lab ? y0 : -1;
      bool bad = false;
      float mx = v[0], ly = v[0];
      int pred = 0;
#pragma unroll
      for (int c = 0; c < NCP; ++c)
        if (c < NC) {
          bad |= ((__float_as_uint(v[c]) >> 23) & 0xff) == 0xff;
          if (c > 0 && v[c] > mx) {
            mx = v[c];
            pred = c;
          }
          if (c == y) ly = v[c];
        }
      int rec_pred = -1, rec_rank = -1, rec_bin = -1;
      uint32_t rec_conf = 0x7fc00000u;
      ++n_rows;
      if (bad) {
        ++n_bad;
      } else {
        int rank = 0;
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < NCP; ++c)
          if (c < NC) {
            rank += (v[c] > ly || (c < y && v[c] == ly)) ? 1 : 0;
            v[c] = expf((v[c] - mx) * a.inv_t);
            se = se + v[c];
          }
        const float conf = div_rn(1.f, se);
        rec_pred = pred;
        rec_conf = __float_as_uint(conf);
        if (lab) {
          ++n_lab;
          const float dy = (ly - mx) * a.inv_t;
          const float nll = logf(se) - dy;
          float brier = 0.f;
#pragma unroll
          for (int c = 0; c < NCP; ++c)
            if (c < NC) {
              const float q = div_rn(v[c], se) - (c == y ? 1.f : 0.f);
              const float q2 = q * q;
              brier = brier + q2;
            }
          const int bin = min(NB - 1, (int)(conf * (float)NB));   // conf in (0, 1]
          rec_rank = rank;
          rec_bin = bin;
          atomicAdd(&hist[a.lay.confusion + y * NC + pred], 1);
          atomicAdd(&hist[a.lay.rank_hist + rank], 1);
          atomicAdd(&hist[a.lay.bin_count + bin], 1);
          if (rank == 0) atomicAdd(&hist[a.lay.bin_correct + bin], 1);
          st = f32x4{conf, nll, brier, __int_as_float(bin)};
        } else {
          atomicAdd(&hist[a.lay.confusion + NC * NC + pred], 1);
        }
      }
      if (a.rows) {
        typedef int i32x4 __attribute__((ext_vector_type(4)));
        *reinterpret_cast<i32x4*>(a.rows + (size_t)r * 4) = i32x4{rec_pred, rec_rank, rec_bin, (int)rec_conf};
      }
    }
    stage[tid] = st;
    __syncthreads();
    if (tid < NB + 2) {
      for (int i = 0; i < EM_TPB; ++i) {
        const f32x4 s = stage[i];     // one address for the whole wave: a broadcast read
        const int b = __float_as_int(s[3]);
        if (b >= 0) {
          if (tid < NB) {
            if (b == tid) part += (double)s[0];
          } else {
            part += (double)(tid == NB ? s[1] : s[2]);
          }
        }
      }
    }
    __syncthreads();   // stage is free again
  }
  if (tid < NB + 2) a.scratch[(size_t)blockIdx.x * (NB + 2) + tid] = part;

  // the three row counters: lanes, then one LDS add per wave
  n_rows = warp_sum_i(n_rows);
  n_lab = warp_sum_i(n_lab);
  n_bad = warp_sum_i(n_bad);
  if ((tid & 63) == 0) {
    atomicAdd(&hist[a.lay.counts + 0], n_rows);
    atomicAdd(&hist[a.lay.counts + 1], n_lab);
    atomicAdd(&hist[a.lay.counts + 2], n_bad);
  }
  __syncthreads();
  for (int i = tid; i < n_i; i += EM_TPB) {
    const int h = hist[i];
    if (h) atomicAdd(&a.acc_i[i], (unsigned long long)h);
  }
}

// acc_f[t] += the partials of entry t, in block order.  The partials of EM_FIN_CHUNK blocks at a
// time are staged in LDS by the whole block (coalesced, every load in flight at once: one thread
// per entry reading them from global memory one after the other costs a load latency per block);
// thread t then adds its entry's staged values in block order.
__global__ __launch_bounds__(EM_FIN_TPB) void eval_metrics_finish_k(const double* __restrict__ scratch, int grid, int n,
                                                                    double* __restrict__ acc_f) {
  __shared__ double part[EM_FIN_CHUNK * (EVAL_MAX_BINS + 2)];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int b0 = 0; b0 < grid; b0 += EM_FIN_CHUNK) {   // block-uniform
    const int nblk = min(EM_FIN_CHUNK, grid - b0);
    const int m = nblk * n;                            // contiguous in scratch from b0 * n
    for (int i = t; i < m; i += EM_FIN_TPB) part[i] = scratch[(size_t)b0 * n + i];
    __syncthreads();
    if (t < n)
      for (int j = 0; j < nblk; ++j) s += part[j * n + t];
    __syncthreads();   // part is free again
  }
  if (t < n) acc_f[t] += s;
}

template <typename T>
void launch_main(int NC, int grid, const EmArgs& a, hipStream_t st) {
  if (NC <= 16)
    hipLaunchKernelGGL((eval_metrics_k<T, 16>), dim3(grid), dim3(EM_TPB), 0, st, a);
  else if (NC <= 32)
    hipLaunchKernelGGL((eval_metrics_k<T, 32>), dim3(grid), dim3(EM_TPB), 0, st, a);
  else
    hipLaunchKernelGGL((eval_metrics_k<T, 64>), dim3(grid), dim3(EM_TPB), 0, st, a);
}

}  // namespace

EvalLayout eval_metrics_layout(int NC, int NB) {
  EvalLayout l{};
  l.confusion = 0;
  l.rank_hist = (NC + 1) * NC;
  l.bin_count = l.rank_hist + NC;
  l.bin_correct = l.bin_count + NB;
  l.counts = l.bin_correct + NB;
  l.size_i = l.counts + 3;
  l.bin_conf_sum = 0;
  l.nll_sum = NB;
  l.brier_sum = NB + 1;
  l.size_f = NB + 2;
  return l;
}

int eval_metrics_max_blocks() { return EM_BLOCKS; }
int64_t eval_metrics_scratch_size(int NB) { return (int64_t)EM_BLOCKS * (std::max(NB, 0) + 2); }

hipError_t eval_metrics(const void* logits, bool logits_bf16, int64_t ld, const int32_t* labels, int nb, int NC,
                        float temperature, int NB, int64_t* acc_i, double* acc_f, double* scratch, int32_t* rows,
                        hipStream_t st) {
  if (nb <= 0) return hipSuccess;
  EmArgs a{};
  a.logits = logits;
  a.labels = labels;
  a.ld = ld;
  a.nb = nb;
  a.NC = NC;
  a.NB = NB;
  // the widest load at which every row start (and every multiple of the width past it) is aligned
  const int es = logits_bf16 ? 2 : 4;
  const uint64_t align = (uint64_t)reinterpret_cast<uintptr_t>(logits) | (uint64_t)(ld * es) | 16u;
  a.vwb = (int)(align & (~align + 1));
  a.nchunks = (nb + EM_TPB - 1) / EM_TPB;
  int grid = cap_grid(std::min(a.nchunks, EM_BLOCKS));
  a.per = (a.nchunks + grid - 1) / grid;
  grid = (a.nchunks + a.per - 1) / a.per;      // every block walks at least one chunk
  a.inv_t = 1.0f / temperature;
  a.lay = eval_metrics_layout(NC, NB);
  a.acc_i = reinterpret_cast<unsigned long long*>(acc_i);
  a.scratch = scratch;
  a.rows = rows;
  if (logits_bf16) launch_main<bf16_t>(NC, grid, a, st);
  else launch_main<float>(NC, grid, a, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(eval_metrics_finish_k, dim3(1), dim3(EM_FIN_TPB), 0, st, scratch, grid, NB + 2, acc_f);
  return hipGetLastError();
}

}  // namespace mnistx
