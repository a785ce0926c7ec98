// Split-K slab reduce (K3 tail): the generic kernel, the multi-tensor partial and reduce
// passes, and the one-launch form that hands over with the last-block ticket (ticket.h).
// Owns the ticket buffers (red_tickets) that the optimizer's finalize ticket shares.
#include "common.h"
#include "launchers.h"
#include "ticket.h"
#include "tpb.h"

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <tuple>
#include <vector>

namespace mnistx {
namespace {

// ------------------------------------------------------------------ split-K reduce
// dst weights [G][I][J] <- sum_s slab[s][g*Ipad + i][j] ; bias[j] <- sum_s slab[s][bias_row][j]
// Fixed summation order (deterministic).  Few slabs: one thread per output;
// many slabs (per-block partials of the fused conv kernels): one wave per
// output, lanes stride the slabs, then a wave reduction.
DEV int64_t reduce_row(int64_t t, int64_t nw, int G, int Ipad, int I, int J, int bias_row, int& j) {
  if (t < nw) {
    j = (int)(t % J);
    const int64_t gi = t / J;
    const int i = (int)(gi % I);
    const int g = (int)(gi / I);
    return (int64_t)g * Ipad + i;
  }
  j = (int)(t - nw);
  return bias_row;
}

__global__ void splitk_reduce_k(const float* __restrict__ slab, int S, int M, int N, int G, int Ipad, int I, int J,
                                int bias_row, float* __restrict__ wdst, float* __restrict__ bdst, float scale) {
  const int64_t nw = (int64_t)G * I * J;
  const int64_t total = nw + (bdst ? J : 0);
  const int64_t ss = (int64_t)M * N;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    int j;
    const int64_t row = reduce_row(t, nw, G, Ipad, I, J, bias_row, j);
    float s = 0.f;
    const float* p = slab + row * N + j;
    for (int z = 0; z < S; ++z) s += p[z * ss];
    if (t < nw) wdst[t] = s * scale;
    else bdst[j] = s * scale;
  }
}

// Coalesced variant (N % 4 == 0), multi-tensor: ONE launch reduces the split-K
// slabs of several layers (RedTable, block ranges per descriptor), so a backward
// pass pays one reduce launch per gradient bucket instead of two per layer.
// Each lane owns 4 consecutive slab columns of one row (one 16-byte load per
// split), the 4 waves of a block take every 4th split, and the 4 partial sums
// are combined in a fixed order (deterministic).  Splits z*zstride, z < S, are
// summed (zstride > 1 after the partial pass).
constexpr int RED_CHUNK = 64;
struct RedDesc {
  float* slab;
  float* wdst;
  float* bdst;
  int64_t nq;        // M * N / 4 quads per split
  int S, M, N, G, Ipad, I, J, bias_row;
  int qb, sb;        // reduce blocks; partial-pass split blocks (0 = no partial pass)
  int tick0;         // first ticket of this descriptor's quad blocks (fused launch, partial pass)
  float scale;
};
struct RedTable {
  RedDesc d[MAXRED];
  int pblk0[MAXRED + 1];  // partial-pass block prefix
  int rblk0[MAXRED + 1];  // reduce-pass block prefix
  int n;
};

DEV int red_find(const int* blk0, int n, int b) {
  int k = 0;
  for (int i = 1; i < n; ++i) k = b >= blk0[i] ? i : k;
  return k;
}

// the reduced quad qd (4 consecutive slab columns of one row) -> weight / bias destination
DEV void red_emit(const RedDesc& D, int64_t qd, const f32x4 t) {
  const int NQ = D.N >> 2;
  const int row = (int)(qd / NQ), j0 = (int)(qd - (int64_t)row * NQ) * 4;
  if (row == D.bias_row) {
    if (D.bdst)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
        if (j0 + jj < D.J) D.bdst[j0 + jj] = t[jj] * D.scale;
    return;
  }
  const int g = row / D.Ipad, i = row - g * D.Ipad;
  if (g >= D.G || i >= D.I) return;
  float* d = D.wdst + ((int64_t)g * D.I + i) * D.J;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj)
    if (j0 + jj < D.J) d[j0 + jj] = t[jj] * D.scale;
}

// block b of the reduce pass: 64 quads, the 4 waves take every 4th split
DEV void red_reduce_block(const RedTable& tab, int b, f32x4 (*part)[64]) {
  const int k = red_find(tab.rblk0, tab.n, b);
  const RedDesc& D = tab.d[k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nq = D.nq;
  const int64_t qd = (int64_t)(b - tab.rblk0[k]) * 64 + lane;
  const int S = D.sb ? D.sb : D.S;
  const int64_t zs = (int64_t)(D.sb ? RED_CHUNK : 1) * nq;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (qd < nq) {
    const f32x4* p = (const f32x4*)D.slab + qd;
    int z = wave;
    for (; z + 12 < S; z += 16) {
      const f32x4 a = p[z * zs], b2 = p[(z + 4) * zs];
      const f32x4 c = p[(z + 8) * zs], d = p[(z + 12) * zs];
      acc += a;
      acc += b2;
      acc += c;
      acc += d;
    }
    for (; z < S; z += 4) acc += p[z * zs];
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave != 0 || qd >= nq) return;
  red_emit(D, qd, ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]);
}

__global__ __launch_bounds__(256) void splitk_reduce4_k(RedTable tab) {
  __shared__ f32x4 part[4][64];
  red_reduce_block(tab, blockIdx.x, part);
}

// First pass for many splits over a small output: block (q, s) of a descriptor
// sums splits [64 s, 64 s + 64) of its 64 quads and stores the sum IN PLACE in
// split 64 s (only this block reads or writes that range), so the reduce pass
// has S/64 splits.  COH: the store goes to the coherence point (fused launch).
template <bool COH>
DEV const RedDesc& red_partial_block(const RedTable& tab, int b, f32x4 (*part)[64], int& qblk, int64_t& qd_out) {
  const int k = red_find(tab.pblk0, tab.n, b);
  const RedDesc& D = tab.d[k];
  const int local = b - tab.pblk0[k];
  qblk = local % D.qb;
  const int sblk = local / D.qb;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nq = D.nq;
  const int64_t qd = (int64_t)qblk * 64 + lane;
  qd_out = qd;
  const int z0 = sblk * RED_CHUNK, z1 = min(D.S, z0 + RED_CHUNK);
  f32x4* p = (f32x4*)D.slab + qd;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (qd < nq) {
    // all 16 loads in flight at once (a dependent chain was latency-bound), summed in order
    constexpr int PER = RED_CHUNK / 4;
    f32x4 v[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int z = z0 + wave + 4 * u;
      v[u] = z < z1 ? p[(int64_t)z * nq] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) acc += v[u];
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && qd < nq) {
    const f32x4 t = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    if constexpr (COH) {
      float* d = (float*)(p + (int64_t)z0 * nq);
#pragma unroll
      for (int j = 0; j < 4; ++j) st_coh(d + j, t[j]);
    } else {
      p[(int64_t)z0 * nq] = t;
    }
  }
  return D;
}

__global__ __launch_bounds__(256) void splitk_partial4_k(RedTable tab) {
  __shared__ f32x4 part[4][64];
  int qblk;
  int64_t qd;
  red_partial_block<false>(tab, blockIdx.x, part, qblk, qd);
}

// ONE launch for both passes (the partial pass's blocks first, then the reduce blocks of the
// descriptors without one): wave 0 of the block that stores the last of a quad block's sb
// partials (coherent stores, then a ticket) sums them in split order (coherent loads) and
// emits.  The winner resets its ticket to 0.
__global__ __launch_bounds__(256) void splitk_fused4_k(RedTable tab, int* __restrict__ tickets) {
  __shared__ f32x4 part[4][64];
  const int pb = tab.pblk0[MAXRED];
  if ((int)blockIdx.x >= pb) {
    red_reduce_block(tab, (int)blockIdx.x - pb, part);
    return;
  }
  int qblk;
  int64_t qd;
  const RedDesc& D = red_partial_block<true>(tab, blockIdx.x, part, qblk, qd);
  if (threadIdx.x >= 64) return;   // wave 0 stored the partials
  int* tk = tickets + D.tick0 + qblk;
  int last = 0;
  if (threadIdx.x == 0) last = take_ticket(tk) == D.sb - 1;
  last = __shfl(last, 0, 64);
  if (!last) return;
  if (threadIdx.x == 0) *tk = 0;
  if (qd >= D.nq) return;
  const float* p = (const float*)((const f32x4*)D.slab + qd);
  const int64_t zs = (int64_t)RED_CHUNK * D.nq * 4;
  f32x4 acc = {ld_coh(p), ld_coh(p + 1), ld_coh(p + 2), ld_coh(p + 3)};
  for (int z = 1; z < D.sb; ++z) {
    const float* q = p + z * zs;
    acc += f32x4{ld_coh(q), ld_coh(q + 1), ld_coh(q + 2), ld_coh(q + 3)};
  }
  red_emit(D, qd, acc);
}

}  // namespace

// Tickets of the fused reduce (one int per partial-pass quad block of a launch: at most
// OPT_TICKET_SLOT) and of the optimizer's finalize (slot OPT_TICKET_SLOT; ticket.h): one zeroed buffer per
// (device, stream), left zeroed by every launch, so launches on different streams (the
// executor's overlapped side-stream reduces) never share a ticket, and launches on one
// stream are ordered.  nullptr (the two-launch path) when disabled (MNISTX_REDUCE_FUSED=0)
// or while the stream is being captured (graphs keep the two launches).
static int g_reduce_fused = -1;
void set_reduce_fused(int on) { g_reduce_fused = on; }
int reduce_fused_enabled() {
  if (g_reduce_fused < 0) {
    const char* e = getenv("MNISTX_REDUCE_FUSED");
    g_reduce_fused = (e && *e) ? atoi(e) != 0 : 1;
  }
  return g_reduce_fused;
}
int* red_tickets(hipStream_t st, bool any_use) {
  if (!any_use && !reduce_fused_enabled()) return nullptr;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  static std::mutex mu;
  static std::vector<std::tuple<int, hipStream_t, int*>> bufs;
  std::lock_guard<std::mutex> lk(mu);
  for (const auto& b : bufs)
    if (std::get<0>(b) == dev && std::get<1>(b) == st) return std::get<2>(b);
  int* p = nullptr;
  const size_t bytes = TICKET_INTS * sizeof(int);
  if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
  if (hipMemset(p, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return nullptr;
  bufs.emplace_back(dev, st, p);
  return p;
}

hipError_t splitk_reduce_multi(const RedSpec* specs, int n, hipStream_t st) {
  if (n < 1) return hipSuccess;
  // one-split slabs (small batches: K below pick_splits' min_k) take the same multi-tensor
  // launch -- its S = 1 sum is the slab itself -- instead of one generic launch per tensor
  // (LeNet-5 at B = 128: 5 launches, ~31 us of a ~100 us step)
  bool vec = true;
  for (int i = 0; i < n; ++i) vec = vec && specs[i].N % 4 == 0 && specs[i].splits >= 1;
  if (!vec) {  // generic path, one launch per tensor
    for (int i = 0; i < n; ++i) {
      const RedSpec& r = specs[i];
      const int64_t total = (int64_t)r.G * r.I * r.J + (r.bdst ? r.J : 0);
      hipLaunchKernelGGL(splitk_reduce_k, dim3(nblocks(total, TPB, 8192)), dim3(TPB), 0, st, r.slab, r.splits, r.M,
                         r.N, r.G, r.Ipad, r.I, r.J, r.bias_row, r.wdst, r.bdst, r.scale);
    }
    return hipGetLastError();
  }
  int* tickets = red_tickets(st);
  for (int i0 = 0; i0 < n; i0 += MAXRED) {
    RedTable tab;
    tab.n = std::min(MAXRED, n - i0);
    int pb = 0, rb = 0, tk = 0;
    const bool fused = tickets != nullptr;
    for (int i = 0; i < tab.n; ++i) {
      const RedSpec& r = specs[i0 + i];
      RedDesc& D = tab.d[i];
      D.slab = r.slab;
      D.wdst = r.wdst;
      D.bdst = r.bdst;
      D.nq = (int64_t)r.M * (r.N / 4);
      D.S = r.splits;
      D.M = r.M;
      D.N = r.N;
      D.G = r.G;
      D.Ipad = r.Ipad;
      D.I = r.I;
      D.J = r.J;
      D.bias_row = r.bias_row;
      D.scale = r.scale;
      D.qb = (int)((D.nq + 63) / 64);
      D.sb = (D.S > RED_CHUNK && D.qb < RED_MAX_QB) ? (D.S + RED_CHUNK - 1) / RED_CHUNK : 0;
      D.tick0 = tk;
      tab.pblk0[i] = pb;
      tab.rblk0[i] = rb;
      pb += D.sb ? D.qb * D.sb : 0;
      tk += D.sb ? D.qb : 0;
      rb += (fused && D.sb) ? 0 : D.qb;   // fused: the partial pass finishes its own quads
    }
    for (int i = tab.n; i <= MAXRED; ++i) {
      tab.pblk0[i] = pb;
      tab.rblk0[i] = rb;
    }
    if (fused) {
      if (pb + rb > 0) hipLaunchKernelGGL(splitk_fused4_k, dim3(pb + rb), dim3(256), 0, st, tab, tickets);
      continue;
    }
    if (pb > 0) hipLaunchKernelGGL(splitk_partial4_k, dim3(pb), dim3(256), 0, st, tab);
    hipLaunchKernelGGL(splitk_reduce4_k, dim3(rb), dim3(256), 0, st, tab);
  }
  return hipGetLastError();
}

hipError_t splitk_reduce(float* slab, int splits, int M, int N, int G, int Ipad, int I, int J, int bias_row,
                         float* wdst, float* bdst, float scale, hipStream_t st) {
  const RedSpec r{slab, wdst, bdst, splits, M, N, G, Ipad, I, J, bias_row, scale};
  return splitk_reduce_multi(&r, 1, st);
}

}  // namespace mnistx
