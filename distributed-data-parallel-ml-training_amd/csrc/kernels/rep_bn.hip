// RepVGG training block, the part that is not a GEMM (Ding et al. 2021), for gfx950: bf16 NHWC
// activations, fp32 statistics, parameters and arithmetic. Over M = N * P * Q rows of K channels
//   y = relu( bn3(z3) + bn1(z1) [+ bn0(x)] ),   bn_b(z) = sc_b * z + sh_b,  sc_b = gamma_b * is_b,
//                                               sh_b = beta_b - mu_b * sc_b
// z3 / z1 the outputs of the block's 3x3 and 1x1 convs, x the block input (identity branch, only
// when the shapes allow it). Backward, with g = dy where the STORED y is > 0, else 0:
//   S = sum g,  T_b = sum g * (z_b - mu_b)                      per channel over the M rows
//   dbeta_b = S,  dgamma_b = is_b * T_b,  k1 = S / M,  k2_b = is_b * T_b / M
//   dz_b = sc_b * (g - k1 - (z_b - mu_b) * is_b * k2_b)
// The sums are centred (z - mu, mu from the forward's table) so that sum g * z - mu * sum g is
// never formed in fp32. g depends on the backward's inputs alone: nothing is recomputed from the
// three branch inputs to decide the ReLU.
//
// No MFMA: there is no matrix product here. No float atomics in the backward; the forward's
// statistics of y follow the conv epilogues' replica convention (one atomic add per channel per
// block into stat_rep(block); the deterministic build gives every block its own replica).
//
// Design: one work split for every kernel of the file.
//   * The row of K channels is nv = K / 8 16-byte vectors. CL = the largest divisor of nv that is
//     at most 8 (128 contiguous bytes) is the number of chunk lanes of a block, nslab = nv / CL
//     the channel slabs: 48 channels -> 6 lanes, 96 -> 6 x 2 slabs, 192 -> 8 x 3, 320 -> 8 x 5,
//     1280 -> 8 x 20. A block
//     is (row block, slab); thread tid = slot * CL + lane owns ONE vector column for the whole
//     launch, so its per-channel coefficients stay in registers, and walks the rows
//     r0 + slot, r0 + slot + nslots, ... of its row block (nslots = 256 / CL; 256 % CL threads
//     idle). Consecutive threads read consecutive 16 bytes of a row, consecutive slots
//     consecutive rows: with nslab == 1 a block reads whole contiguous rows, and the slabs of a
//     row block are neighbouring blocks.
//   * Rows are dealt to row blocks in equal contiguous ranges; the host caps the grid (forward
//     and apply 2048 blocks, reduce 512) and a block loops. One row (the 1x1 tail) is one block
//     per slab with one live slot; 256 x 112 x 112 rows are 2048 blocks of some 1500 rows each.
//     The backward's two row-block counts are also held to sqrt(M / 32) and four times that, so
//     that the apply blocks' re-reads of the partials stay an eighth of the activation bytes (an
//     earlier cut without that limit spent most of the backward there: 1.49 ms for 256 x 14 x 14
//     x 256, three branches).
//   * Forward, rep_fwd_kernel: the prologue sums the statistics replicas of the block's channels
//     in replica order and forms the three scales and the ONE summed shift in LDS (row block 0
//     also writes the three coefficient tables and updates the running statistics); the loop
//     keeps 4 rows x 3 inputs of 16-byte loads in flight, y = max(fma(z3, sc3, fma(z1, sc1,
//     fma(x, sc0, sh))), 0), one 16-byte store per row. With ``ostats`` the lane also sums the
//     rounded y and its square; lanes -> LDS -> slots added in order -> one atomic per channel.
//   * rep_stats_kernel: the same loop over x alone, for an identity branch whose producer did not
//     emit the statistics (preceded by a clear kernel: hipMemsetAsync is not captured).
//   * Backward 1, rep_bwd_reduce_kernel: S and T_b in lane registers, slots added in LDS in slot
//     order, plain stores of the block's partials [row block][slab][4][8 CL].
//   * Backward 2, rep_bwd_apply_kernel: the prologue adds the partials of the block's channels in
//     row-block order (thread j owns one (sum, channel), so the order is fixed), derives k1 and
//     is_b * k2_b, row block 0 writes k1 / k2 into the tables and adds dgamma / dbeta onto the
//     gradient arena; the loop streams dz3, dz1 and the identity gradient, which goes into the
//     buffer the two conv DGRADs then accumulate into.
//
// Resource usage: compiler output of -Rpass-analysis=kernel-resource-usage for gfx950 at -O3,
// NOT a measurement; <2 branches> / <3 branches>:
//   rep_fwd_kernel:          79 / 105 VGPRs,  scratch 0, LDS 1 KB,  6 / 4 waves / SIMD
//   ... with ostats:         96 / 122 VGPRs,  scratch 0, LDS 17 KB, 5 / 4 waves / SIMD
//   rep_stats_kernel:        40 VGPRs,        scratch 0, LDS 16 KB, 8 waves / SIMD
//   rep_bwd_reduce_kernel:   84 / 108 VGPRs,  scratch 0, LDS 8 KB,  5 / 4 waves / SIMD
//   rep_bwd_apply_kernel:    106 / 140 VGPRs, scratch 0, LDS 1 KB,  4 / 3 waves / SIMD
// No kernel of this file uses scratch.
//
// Limits (ddp_rep_bn_ok): K % 8 == 0, N, P, Q >= 1, N * P * Q * K below 2^31. A K / 8 without a
// divisor in 2..8 runs with CL = 1: correct, one vector per row per block.
// Out of scope: a backward from running statistics, a one-launch backward for the 2x2 / 1x1 tails.
#include "common.h"
#include "api.h"
#include "norm_tile.h"

#include <algorithm>

namespace ddp_amd {
namespace rep {

using namespace tile;  // F8, cvt8, pack8, ldf8

enum { kSc = 0, kSh = 1, kMu = 2, kIs = 3, kK1 = 4, kK2 = 5 };  // coef table rows (bn_act.hip)
constexpr int kMaxCL = 8;          // chunk lanes at most: a block reads 128 contiguous bytes of a row
constexpr int kMaxW = 8 * kMaxCL;  // channels of the widest slab

struct Plan {
  int CL, nslots, nslab, W;  // chunk lanes, lane slots, slabs, channels of a slab (8 CL)
  int nrb, rpb;              // row blocks, rows of a row block
  FastDiv dCL, dSlab;
};

// This thread's place: block = rb * nslab + slab, thread = slot * CL + cl. Idle threads (past
// the last whole slot) have live == false and touch no activation.
struct Lane {
  int rb, slab, slot, cl, c0;
  int r0, r1;
  bool live;
};

__device__ __forceinline__ Lane locate(const Plan& p, int M) {
  Lane l;
  l.rb = fast_div((int)blockIdx.x, p.dSlab);
  l.slab = blockIdx.x - l.rb * p.nslab;
  l.slot = fast_div((int)threadIdx.x, p.dCL);
  l.cl = threadIdx.x - l.slot * p.CL;
  l.live = l.slot < p.nslots;
  l.c0 = (l.slab * p.CL + l.cl) * 8;
  l.r0 = l.rb * p.rpb;
  l.r1 = min(M, l.r0 + p.rpb);
  return l;
}

__device__ __forceinline__ uint4 ld16(const unsigned short* p, size_t off, bool ok) {
  uint4 u = {0u, 0u, 0u, 0u};
  if (ok) u = *reinterpret_cast<const uint4*>(p + off);
  return u;
}

// One branch's BatchNorm of channel c from its statistics replicas (or the running statistics):
// the expressions of bn_act.hip finalize_fwd_ch. ``owner``: this block writes the table and the
// running statistics.
__device__ __forceinline__ void finalize(const RepBnArgs& a, const RepBranch& br, int c, float M,
                                         bool owner, float& sc, float& sh) {
  const int K = a.K;
  float mu, is;
  if (a.use_running) {
    mu = br.running_mean[c];
    is = rsqrtf(br.running_var[c] + br.eps);
  } else {
    float s1 = 0.f, s2 = 0.f;
    for (int r = 0; r < kStatRep; ++r) {
      s1 += br.stats[(size_t)r * 2 * K + c];
      s2 += br.stats[(size_t)r * 2 * K + K + c];
    }
    mu = s1 / M;
    const float var = fmaxf(s2 / M - mu * mu, 0.f);
    is = rsqrtf(var + br.eps);
    if (owner && br.running_mean) {
      const float unbiased = M > 1.f ? var * M / (M - 1.f) : var;
      br.running_mean[c] = (1.f - br.momentum) * br.running_mean[c] + br.momentum * mu;
      br.running_var[c] = (1.f - br.momentum) * br.running_var[c] + br.momentum * unbiased;
    }
  }
  sc = br.gamma[c] * is;
  sh = br.beta[c] - mu * sc;
  if (owner) {
    br.coef[kSc * K + c] = sc;
    br.coef[kSh * K + c] = sh;
    br.coef[kMu * K + c] = mu;
    br.coef[kIs * K + c] = is;
  }
}

// The block's per-channel (sum, sum of squares) from the lanes' registers: [thread][16] in LDS,
// one thread per (chunk lane, moment, channel) adds the slots in order, then one add into the
// block's replica. red: 256 * 16 floats. All 256 threads call it.
__device__ __forceinline__ void emit_stats(float* red, const float* s1, const float* s2,
                                           float* stats, const Lane& l, const Plan& p, int K) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[tid * 16 + e] = s1[e];
    red[tid * 16 + 8 + e] = s2[e];
  }
  __syncthreads();
  float* st = stats + (size_t)stat_rep(blockIdx.x) * 2 * K;
  for (int t = tid; t < p.CL * 16; t += 256) {
    const int rcl = t >> 4, j = t & 15;
    float v = 0.f;
    for (int s = 0; s < p.nslots; ++s) v += red[(s * p.CL + rcl) * 16 + j];
    const int ch = (l.slab * p.CL + rcl) * 8 + (j & 7);
    atomicAdd(st + (j >> 3) * K + ch, stat_val(v, blockIdx.x));
  }
}

__device__ __forceinline__ void add_moments(const F8& r, float* s1, float* s2) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    s1[e] += r.v[e];
    s2[e] = __builtin_fmaf(r.v[e], r.v[e], s2[e]);
  }
}

// ------------------------------------------------------------------ forward
constexpr int kFwdRows = 4;  // rows of loads a lane keeps in flight

template <int NB, bool STATS>
__global__ __launch_bounds__(256) void rep_fwd_kernel(RepBnArgs a, Plan p) {
  __shared__ float tab[4 * kMaxW];  // sc3 | sc1 | sc0 | summed shift of the slab's channels
  __shared__ float red[STATS ? 256 * 16 : 1];
  const int K = a.K, M = a.N * a.P * a.Q;
  const Lane l = locate(p, M);

  for (int c = threadIdx.x; c < p.W; c += 256) {
    const int ch = l.slab * p.W + c;
    float sh = 0.f;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float sc, shb;
      finalize(a, a.br[b], ch, (float)M, l.rb == 0, sc, shb);
      tab[b * kMaxW + c] = sc;
      sh = b == 0 ? shb : sh + shb;  // (sh3 + sh1) + sh0
    }
    tab[3 * kMaxW + c] = sh;
  }
  __syncthreads();

  float s1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float s2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (l.live) {
    F8 sc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) sc[b] = ldf8(tab + b * kMaxW + l.cl * 8);
    const F8 sh = ldf8(tab + 3 * kMaxW + l.cl * 8);
    const int step = p.nslots;
    for (int r = l.r0 + l.slot; r < l.r1; r += kFwdRows * step) {
      uint4 u[NB][kFwdRows];
#pragma unroll
      for (int j = 0; j < kFwdRows; ++j) {
        const int rr = r + j * step;
        const size_t off = (size_t)rr * K + l.c0;
#pragma unroll
        for (int b = 0; b < NB; ++b) u[b][j] = ld16(a.br[b].z, off, rr < l.r1);
      }
#pragma unroll
      for (int j = 0; j < kFwdRows; ++j) {
        const int rr = r + j * step;
        if (rr >= l.r1) break;
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = sh.v[e];
#pragma unroll
        for (int b = NB - 1; b >= 0; --b) {
          const F8 z = cvt8(u[b][j]);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = __builtin_fmaf(z.v[e], sc[b].v[e], o[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = fmaxf(o[e], 0.f);
        const uint4 y = pack8(o);
        *reinterpret_cast<uint4*>(a.y + (size_t)rr * K + l.c0) = y;
        if (STATS) add_moments(cvt8(y), s1, s2);
      }
    }
  }
  if (STATS) emit_stats(red, s1, s2, a.ostats, l, p, K);
}

__global__ __launch_bounds__(256) void rep_clear_kernel(float* dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = 0.f;
}

__global__ __launch_bounds__(256) void rep_stats_kernel(const unsigned short* x, int M, int K,
                                                        float* stats, Plan p) {
  __shared__ float red[256 * 16];
  const Lane l = locate(p, M);
  float s1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float s2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (l.live) {
    const int step = p.nslots;
    for (int r = l.r0 + l.slot; r < l.r1; r += kFwdRows * step) {
      uint4 u[kFwdRows];
#pragma unroll
      for (int j = 0; j < kFwdRows; ++j) {
        const int rr = r + j * step;
        u[j] = ld16(x, (size_t)rr * K + l.c0, rr < l.r1);  // (zeros past the end add nothing)
      }
#pragma unroll
      for (int j = 0; j < kFwdRows; ++j) add_moments(cvt8(u[j]), s1, s2);
    }
  }
  emit_stats(red, s1, s2, stats, l, p, K);
}

// ------------------------------------------------------------------ backward
constexpr int kBwdRows = 2;

// g = dy where the stored y is positive
__device__ __forceinline__ F8 masked(uint4 dy, uint4 y) {
  F8 g = cvt8(dy);
  const F8 m = cvt8(y);
#pragma unroll
  for (int e = 0; e < 8; ++e) g.v[e] = m.v[e] > 0.f ? g.v[e] : 0.f;
  return g;
}

template <int NB>
__global__ __launch_bounds__(256) void rep_bwd_reduce_kernel(RepBnArgs a, Plan p) {
  __shared__ float red[256 * 8];
  const int K = a.K, M = a.N * a.P * a.Q, tid = threadIdx.x;
  const Lane l = locate(p, M);
  float acc[1 + NB][8];  // S, T3, T1 (, T0)
#pragma unroll
  for (int q = 0; q < 1 + NB; ++q)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[q][e] = 0.f;
  if (l.live) {
    F8 mu[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) mu[b] = ldf8(a.br[b].coef + kMu * K + l.c0);
    const int step = p.nslots;
    for (int r = l.r0 + l.slot; r < l.r1; r += kBwdRows * step) {
      uint4 ud[kBwdRows], uy[kBwdRows], u[NB][kBwdRows];
#pragma unroll
      for (int j = 0; j < kBwdRows; ++j) {
        const int rr = r + j * step;
        const bool ok = rr < l.r1;
        const size_t off = (size_t)rr * K + l.c0;
        ud[j] = ld16(a.dy, off, ok);
        uy[j] = ld16(a.y, off, ok);  // (y = 0 past the end: g = 0)
#pragma unroll
        for (int b = 0; b < NB; ++b) u[b][j] = ld16(a.br[b].z, off, ok);
      }
#pragma unroll
      for (int j = 0; j < kBwdRows; ++j) {
        const F8 g = masked(ud[j], uy[j]);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[0][e] += g.v[e];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const F8 z = cvt8(u[b][j]);
#pragma unroll
          for (int e = 0; e < 8; ++e)
            acc[1 + b][e] = __builtin_fmaf(g.v[e], z.v[e] - mu[b].v[e], acc[1 + b][e]);
        }
      }
    }
  }
  // the block's slots added in slot order, sum by sum
  float* dst = a.ws + (size_t)blockIdx.x * 4 * p.W;
#pragma unroll
  for (int q = 0; q < 1 + NB; ++q) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid * 8 + e] = acc[q][e];
    __syncthreads();
    for (int t = tid; t < p.W; t += 256) {
      const int rcl = t >> 3, e = t & 7;
      float v = 0.f;
      for (int s = 0; s < p.nslots; ++s) v += red[(s * p.CL + rcl) * 8 + e];
      dst[q * p.W + t] = v;
    }
  }
}

// nrb_red: row blocks of the reduce launch that wrote the partials
template <int NB>
__global__ __launch_bounds__(256) void rep_bwd_apply_kernel(RepBnArgs a, Plan p, int nrb_red) {
  __shared__ float tab[4 * kMaxW];  // S | T3 | T1 | T0, then k1 | w3 | w1 | w0 (w = is * k2)
  const int K = a.K, M = a.N * a.P * a.Q, W = p.W;
  const Lane l = locate(p, M);

  // ---- the partials of this slab in row-block order: thread j owns (sum q, channel c)
  const size_t step = (size_t)p.nslab * 4 * W;
  for (int j = threadIdx.x; j < (1 + NB) * W; j += 256) {
    const int q = fast_div(j >> 3, p.dCL), c = j - q * W;
    const float* src = a.ws + ((size_t)l.slab * 4 + q) * W + c;
    float v[4] = {0.f, 0.f, 0.f, 0.f};  // four loads in flight; the order is fixed all the same
    int r = 0;
    for (; r + 4 <= nrb_red; r += 4)
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] += src[(r + i) * step];
    for (; r < nrb_red; ++r) v[0] += src[r * step];
    tab[q * kMaxW + c] = (v[0] + v[1]) + (v[2] + v[3]);
  }
  __syncthreads();
  const float inv_m = 1.f / (float)M;
  for (int c = threadIdx.x; c < W; c += 256) {
    const int ch = l.slab * W + c;
    const float S = tab[c], k1 = S * inv_m;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const RepBranch& br = a.br[b];
      const float is = br.coef[kIs * K + ch];
      const float s2 = is * tab[(1 + b) * kMaxW + c];  // sum g * xhat
      const float k2 = s2 * inv_m;
      tab[(1 + b) * kMaxW + c] = is * k2;
      if (l.rb == 0) {  // one writer per channel: plain accumulate into the arena
        br.coef[kK1 * K + ch] = k1;
        br.coef[kK2 * K + ch] = k2;
        br.dgamma[ch] += s2;
        br.dbeta[ch] += S;
      }
    }
    tab[c] = k1;
  }
  __syncthreads();
  if (!l.live) return;

  // ---- dz_b = sc_b * (g - k1 - (z_b - mu_b) * w_b)
  const F8 k1 = ldf8(tab + l.cl * 8);
  F8 sc[NB], mu[NB], w[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    sc[b] = ldf8(a.br[b].coef + kSc * K + l.c0);
    mu[b] = ldf8(a.br[b].coef + kMu * K + l.c0);
    w[b] = ldf8(tab + (1 + b) * kMaxW + l.cl * 8);
  }
  const int nstep = p.nslots;
  for (int r = l.r0 + l.slot; r < l.r1; r += kBwdRows * nstep) {
    uint4 ud[kBwdRows], uy[kBwdRows], u[NB][kBwdRows];
#pragma unroll
    for (int j = 0; j < kBwdRows; ++j) {
      const int rr = r + j * nstep;
      const bool ok = rr < l.r1;
      const size_t off = (size_t)rr * K + l.c0;
      ud[j] = ld16(a.dy, off, ok);
      uy[j] = ld16(a.y, off, ok);
#pragma unroll
      for (int b = 0; b < NB; ++b) u[b][j] = ld16(a.br[b].z, off, ok);
    }
#pragma unroll
    for (int j = 0; j < kBwdRows; ++j) {
      const int rr = r + j * nstep;
      if (rr >= l.r1) break;
      F8 g = masked(ud[j], uy[j]);
#pragma unroll
      for (int e = 0; e < 8; ++e) g.v[e] -= k1.v[e];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const F8 z = cvt8(u[b][j]);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          o[e] = sc[b].v[e] * __builtin_fmaf(-(z.v[e] - mu[b].v[e]), w[b].v[e], g.v[e]);
        *reinterpret_cast<uint4*>(a.br[b].dz + (size_t)rr * K + l.c0) = pack8(o);
      }
    }
  }
}

// ------------------------------------------------------------------ host side
static bool shape_ok(int N, int P, int Q, int K) {
  if (N < 1 || P < 1 || Q < 1 || K < 8 || K % 8) return false;
  return (long long)N * P * Q * K < 0x80000000ll;
}

// ``cap``: blocks of the launch at most; ``rows``: rows a lane handles per loop iteration (a
// block is not given less than one iteration of every slot while rows remain); ``nrb_max``: row
// blocks at most (0: no further limit)
static Plan plan(int M, int K, int cap, int rows, int nrb_max = 0) {
  Plan p{};
  const int nv = K / 8;
  p.CL = 1;
  for (int cl = std::min(kMaxCL, nv); cl > 1; --cl)
    if (nv % cl == 0) { p.CL = cl; break; }
  p.nslots = 256 / p.CL;
  p.nslab = nv / p.CL;
  p.W = p.CL * 8;
  const int per = p.nslots * rows;
  const int want = (M + per - 1) / per;
  int nrb = std::min(want, cap / p.nslab);
  if (nrb_max > 0) nrb = std::min(nrb, nrb_max);
  nrb = std::max(1, nrb);
  p.rpb = (M + nrb - 1) / nrb;
  p.nrb = (M + p.rpb - 1) / p.rpb;
  p.dCL = make_fastdiv(p.CL);
  p.dSlab = make_fastdiv(p.nslab);
  return p;
}

// the deterministic build keeps one replica per block: block ids stay below kStatRep (4096)
constexpr int kCapStream = 2048, kCapReduce = 512;

// Every apply block adds the reduce launch's partials of its channels again: nrb_apply *
// nrb_reduce * 16 K bytes in all, against some 16 M K bytes of activations. The two row-block
// counts are held to nrb_reduce = sqrt(M / 32) and nrb_apply = 4 nrb_reduce, an eighth of the
// activation bytes; the narrow slabs supply the rest of the grid.
static int reduce_rows(int M) {
  int n = 1;
  while ((long long)(n + 1) * (n + 1) * 32 <= M) ++n;
  return n;
}
static Plan reduce_plan(int M, int K) { return plan(M, K, kCapReduce, kBwdRows, reduce_rows(M)); }
static Plan apply_plan(int M, int K) { return plan(M, K, kCapStream, kBwdRows, 4 * reduce_rows(M)); }
static size_t ws_need(const Plan& p) { return (size_t)p.nrb * p.nslab * 4 * p.W; }

}  // namespace rep
}  // namespace ddp_amd

using namespace ddp_amd;

extern "C" int ddp_rep_bn_ok(int N, int P, int Q, int K) { return rep::shape_ok(N, P, Q, K) ? 1 : 0; }

extern "C" size_t ddp_rep_bn_ws_elems(int N, int P, int Q, int K) {
  if (!rep::shape_ok(N, P, Q, K)) return 0;
  return rep::ws_need(rep::reduce_plan(N * P * Q, K));
}

extern "C" int ddp_rep_bn_fwd(const RepBnArgs* ap, hipStream_t st) {
  if (!ap || !rep::shape_ok(ap->N, ap->P, ap->Q, ap->K) || ap->nbr < 2 || ap->nbr > 3) return -1;
  const RepBnArgs& a = *ap;
  if (!a.y) return -1;
  for (int b = 0; b < a.nbr; ++b) {
    const RepBranch& br = a.br[b];
    if (!br.z || !br.gamma || !br.beta || !br.coef) return -1;
    if (a.use_running ? (!br.running_mean || !br.running_var) : !br.stats) return -1;
  }
  const rep::Plan p = rep::plan(a.N * a.P * a.Q, a.K, rep::kCapStream, rep::kFwdRows);
  const dim3 grid(p.nrb * p.nslab), block(256);
  if (a.nbr == 3) {
    if (a.ostats) hipLaunchKernelGGL((rep::rep_fwd_kernel<3, true>), grid, block, 0, st, a, p);
    else hipLaunchKernelGGL((rep::rep_fwd_kernel<3, false>), grid, block, 0, st, a, p);
  } else {
    if (a.ostats) hipLaunchKernelGGL((rep::rep_fwd_kernel<2, true>), grid, block, 0, st, a, p);
    else hipLaunchKernelGGL((rep::rep_fwd_kernel<2, false>), grid, block, 0, st, a, p);
  }
  return (int)hipGetLastError();
}

extern "C" int ddp_rep_bn_bwd(const RepBnArgs* ap, hipStream_t st) {
  if (!ap || !rep::shape_ok(ap->N, ap->P, ap->Q, ap->K) || ap->nbr < 2 || ap->nbr > 3) return -1;
  const RepBnArgs& a = *ap;
  if (!a.y || !a.dy || !a.ws) return -1;
  for (int b = 0; b < a.nbr; ++b) {
    const RepBranch& br = a.br[b];
    if (!br.z || !br.coef || !br.dz || !br.dgamma || !br.dbeta) return -1;
  }
  const int M = a.N * a.P * a.Q;
  const rep::Plan pr = rep::reduce_plan(M, a.K);
  if (rep::ws_need(pr) > a.ws_elems) return -2;
  const rep::Plan pa = rep::apply_plan(M, a.K);
  const dim3 gr(pr.nrb * pr.nslab), ga(pa.nrb * pa.nslab), block(256);
  if (a.nbr == 3) {
    hipLaunchKernelGGL((rep::rep_bwd_reduce_kernel<3>), gr, block, 0, st, a, pr);
    hipLaunchKernelGGL((rep::rep_bwd_apply_kernel<3>), ga, block, 0, st, a, pa, pr.nrb);
  } else {
    hipLaunchKernelGGL((rep::rep_bwd_reduce_kernel<2>), gr, block, 0, st, a, pr);
    hipLaunchKernelGGL((rep::rep_bwd_apply_kernel<2>), ga, block, 0, st, a, pa, pr.nrb);
  }
  return (int)hipGetLastError();
}

extern "C" int ddp_rep_bn_stats(const void* x, int N, int P, int Q, int K, float* stats,
                                hipStream_t st) {
  if (!rep::shape_ok(N, P, Q, K) || !x || !stats) return -1;
  if ((long long)kStatRep * 2 * K >= 0x80000000ll) return -1;
  const int M = N * P * Q, n = kStatRep * 2 * K;
  const rep::Plan p = rep::plan(M, K, rep::kCapStream, rep::kFwdRows);
  hipLaunchKernelGGL(rep::rep_clear_kernel, dim3((n + 255) / 256), dim3(256), 0, st, stats, n);
  hipLaunchKernelGGL(rep::rep_stats_kernel, dim3(p.nrb * p.nslab), dim3(256), 0, st,
                     reinterpret_cast<const unsigned short*>(x), M, K, stats, p);
  return (int)hipGetLastError();
}
