// GroupNorm + ReLU (+ 2x2 max-pool) for gfx950, forward and backward, on a tile that stays in
// registers (bf16 NHWC activations, fp32 parameters and arithmetic):
//   y  = pool2x2?(relu?(gamma_c * (z - mu_{n,g}) * is_{n,g} + beta_c)),  is = rsqrt(var + eps)
//   dz = is * (dxhat - A / m - xhat * B / m),  dxhat = dyb * gamma_c,  A / B the group's sums of
//        dxhat / dxhat * xhat over its m = Cg * P * Q elements, dyb the gradient routed to the
//        window's first maximum and through the ReLU mask.
//
// No MFMA: there is no matrix product here, about 20 VALU operations per element each way.
//
// Design:
//   * A GroupNorm group is local: the Cg channels of ONE image. BatchNorm's statistics span the
//     batch and need conv-epilogue atomics, a finalize launch and a second streaming pass
//     (bn_act.hip); here a workgroup owns one image and a slab of whole groups and does the whole
//     layer in one launch: z (backward: z and dy) is read from memory once, y / dz written once.
//   * Where the tile lives. The served tile is at most 8192 elements per slab unit (kBudget):
//     32 fp32 values in each of 256 lanes, i.e. four 16-byte vectors per lane. The backward
//     holds two such tiles (xhat and dxhat, 64 VGPRs). That fits the register file with three
//     to four waves per SIMD left (below), so the tile is kept in REGISTERS, not in LDS: the statistics
//     passes (sum, centred sum of squares, then the output) re-read registers for free, and LDS
//     carries only the cross-lane sums (at most 32 KB). An LDS tile would add a write and two to
//     three reads of every element for nothing: no lane ever needs another lane's elements.
//   * Lane layout. A lane owns one 8-channel chunk (one 16-byte access) of up to four pixels.
//     tid = slot * CL + chunk lane: the CL chunk lanes of a pixel are consecutive, then
//     consecutive pixels, so a wave reads runs of CL * 16 contiguous bytes. Unpooled, a lane's
//     pixels are slot + j * (256 / CL), j = 0..3; pooled, they are the four pixels of ONE 2x2
//     window in row-major order, so the max, the first-maximum position and the gradient routing
//     happen in one lane's registers (the layout conv_l0.hip arrived at).
//   * Slab width CL (chunk lanes, 8 channels each): the widest divisor of C / 8, a multiple of
//     the lanes of one group, at most 64, whose tile fits four vectors per lane. A 32x32 image
//     (VGG layer 0) gets CL = 1: 8 blocks per image that each use 16 B of every 128-byte line;
//     xcd_remap puts the slabs of an image on the same XCD so that the line's other seven
//     readers find it in that L2. 16x16 gets CL = 4, 8x8 and below whole lines (CL >= 8). CL need
//     not be a power of two (C = 40: CL = 5, 51 slots, one idle lane).
//   * Group sums. Cg < 8: a lane's vector holds 8 / Cg whole groups, whose sums are formed in
//     the lane. Cg >= 8: a group spans Cg / 8 adjacent lanes, combined first with DPP adds
//     (quad_perm, row_half_mirror: no LDS). Then the lanes that hold other pixels of the same
//     channels meet in LDS: every 16th slot is added by one lane (in slot order), then the 16
//     results by every lane (in slot order): a fixed order whatever the launch, at most 32
//     serial LDS reads instead of 256, two barriers per sum. The variance is the centred sum
//     of (z - mu)^2 over the resident tile: no E[z^2] - mu^2 cancellation.
//   * The backward recomputes xhat and the pre-activation from z and the forward's (mu, is)
//     table with the forward's own expression: no masks or indices are saved. A and B are built
//     from the per-channel sums (A = sum_c gamma_c * sum dyb), which dgamma / dbeta need anyway.
//   * Per-channel sums (dgamma, dbeta and the producing conv's bias gradient dbias = sum dz, which
//     is NOT zero under GroupNorm) go as fp32 partials [N][3][C] into the workspace; the finish
//     kernel adds them over n in a fixed order into the gradient arena: no float atomics.
//
// Resource usage: compiler output of -Rpass-analysis=kernel-resource-usage for gfx950 at -O3,
// NOT a measurement; the range over the eight <CGL, POOL> instantiations of each kernel:
//   gn_fwd_kernel:     60 .. 77 VGPRs,  scratch 0, LDS 2 .. 16 KB,  6 .. 8 waves / SIMD
//   gn_bwd_kernel:    112 .. 129 VGPRs, scratch 0, LDS 16 .. 32 KB, 3 .. 4 waves / SIMD
//                     (<1, pool>: 129 VGPRs, 3 waves; every other one at most 127, 4 waves)
//   gn_finish_kernel:  29 VGPRs,        scratch 0, LDS 1 KB,        8 waves / SIMD
// No kernel of this file uses scratch.
//
// Limits (ddp_gn_ok): C % 8 == 0, C % groups == 0, Cg = C / groups a power of two <= 64, even P
// and Q with the pool, max(8, Cg) * P * Q <= 8192, tensors below 2^31 elements. Larger images
// would need a streaming variant.
#include "common.h"
#include "api.h"
#include "norm_tile.h"

#include <algorithm>

namespace ddp_amd {
namespace gn {

using namespace tile;  // F8, cvt8, pack8, ldf8, xhat_of, pre_of

constexpr int kBudget = 8192;  // resident elements of one slab unit: 4 vectors x 8 x 256 lanes
constexpr int kFold = 16;      // slots added by one lane in the first LDS phase

struct Plan {
  int CL, nslots, nslab, lpg, Wo;  // chunk lanes, pixel slots, slabs per image, lanes per group
  float inv_m;                     // 1 / (Cg * P * Q)
  FastDiv dCL, dWo, dSlab;
};

// This thread's place in the tile. Idle lanes (past the last whole slot, when CL does not divide
// 256) take slot = nslots, chunk lane 0: they add zeros, read live cells and write nothing.
struct Lane {
  int n, slot, cl, chunk;
  bool live;    // the lane exists in the layout
  bool ok[4];   // its vector j lies in the image
  int pix[4];   // ... at this pixel (p * Q + q)
};

template <bool POOL>
__device__ __forceinline__ Lane locate(const GnArgs& a, const Plan& p) {
  Lane l;
  const int blk = xcd_remap(blockIdx.x, gridDim.x);
  l.n = fast_div(blk, p.dSlab);
  const int slab = blk - l.n * p.nslab;
  l.slot = fast_div((int)threadIdx.x, p.dCL);
  l.cl = threadIdx.x - l.slot * p.CL;
  l.live = l.slot < p.nslots;
  if (!l.live) { l.slot = p.nslots; l.cl = 0; }
  l.chunk = slab * p.CL + l.cl;
  if (POOL) {
    const int wp = fast_div(l.slot, p.dWo), wq = l.slot - wp * p.Wo;
    const bool v = l.live && l.slot < (a.P >> 1) * p.Wo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      l.ok[j] = v;
      l.pix[j] = (2 * wp + (j >> 1)) * a.Q + 2 * wq + (j & 1);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      l.pix[j] = l.slot + j * p.nslots;
      l.ok[j] = l.live && l.pix[j] < a.P * a.Q;
    }
  }
  return l;
}

// v[i] <- the sum of v[i] over every lane of the block with this lane's chunk lane, in a fixed
// order, delivered to all of them. lds: 2 * NV * 256 floats, [value][lane] (conflict-free).
template <int NV>
__device__ __forceinline__ void slot_sum(float (&v)[NV], float* lds, const Lane& l, const Plan& p) {
  float* A = lds;
  float* B = lds + NV * 256;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < NV; ++i) A[i * 256 + tid] = v[i];
  __syncthreads();
  const int rows = min(kFold, p.nslots);
  if (l.slot < rows) {  // (an idle lane's slot is nslots >= rows)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      float t = A[i * 256 + tid];
      for (int s = l.slot + kFold; s < p.nslots; s += kFold) t += A[i * 256 + s * p.CL + l.cl];
      B[i * 256 + tid] = t;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    float t = B[i * 256 + l.cl];
    for (int s = 1; s < rows; ++s) t += B[i * 256 + s * p.CL + l.cl];
    v[i] = t;
  }
  // (the next call's first barrier separates these reads from its writes of B)
}

// ... preceded, for a group that spans lpg = 2, 4, 8 adjacent lanes, by their DPP sum (CL and
// nslots * CL are multiples of lpg, so the lanes of a group are aligned and all live or all
// idle). Must be called by all 256 threads.
template <int NV>
__device__ __forceinline__ void group_sum(float (&v)[NV], float* lds, const Lane& l, const Plan& p) {
  if (p.lpg >= 2) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += dpp_f<0xB1>(v[i]);
  }
  if (p.lpg >= 4) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += dpp_f<0x4E>(v[i]);
  }
  if (p.lpg >= 8) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += dpp_f<0x141>(v[i]);
  }
  slot_sum<NV>(v, lds, l, p);
}

// the tile's z as fp32 (zeros outside the image)
__device__ __forceinline__ void load_tile(const unsigned short* base, const Lane& l, int C,
                                          F8 (&t)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint4 u = {0u, 0u, 0u, 0u};
    if (l.ok[j]) u = *reinterpret_cast<const uint4*>(base + (size_t)l.pix[j] * C);
    t[j] = cvt8(u);
  }
}

// CGL = min(Cg, 8): channels of one group inside a lane's vector; NG = 8 / CGL groups per lane
template <int CGL, bool POOL>
__global__ __launch_bounds__(256) void gn_fwd_kernel(GnArgs a, Plan p) {
  constexpr int NG = 8 / CGL;
  __shared__ float lds[2 * NG * 256];
  const Lane l = locate<POOL>(a, p);
  const int C = a.C, c0 = l.chunk * 8;
  const size_t img = (size_t)l.n * a.P * a.Q * C;
  F8 z[4];
  load_tile(a.z + img + c0, l, C, z);

  // ---- mean
  float mu[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) mu[g] = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) mu[e / CGL] += (z[0].v[e] + z[1].v[e]) + (z[2].v[e] + z[3].v[e]);
  group_sum<NG>(mu, lds, l, p);
#pragma unroll
  for (int g = 0; g < NG; ++g) mu[g] *= p.inv_m;

  // ---- centred variance from the resident tile
  float is[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) is[g] = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = l.ok[j] ? z[j].v[e] - mu[e / CGL] : 0.f;
      t = __builtin_fmaf(d, d, t);
    }
    is[e / CGL] += t;
  }
  group_sum<NG>(is, lds, l, p);
#pragma unroll
  for (int g = 0; g < NG; ++g) is[g] = rsqrtf(is[g] * p.inv_m + a.eps);

  if (l.live && l.slot == 0 && (l.cl & (p.lpg - 1)) == 0) {
    // one lane per group: Cg < 8 the chunk's NG groups, else the group of chunk / lpg
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int gi = CGL < 8 ? l.chunk * NG + g : l.chunk / p.lpg;
      float* t = a.table + ((size_t)l.n * a.groups + gi) * 2;
      t[0] = mu[g];
      t[1] = is[g];
    }
  }

  // ---- normalise, ReLU, pool from the resident copy
  const F8 ga = ldf8(a.gamma + c0), be = ldf8(a.beta + c0);
  float o[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = pre_of(xhat_of(z[j].v[e], mu[e / CGL], is[e / CGL]), ga.v[e], be.v[e]);
      o[j][e] = a.relu ? fmaxf(v, 0.f) : v;
    }
  if (POOL) {
    if (!l.ok[0]) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[0][e] = fmaxf(fmaxf(o[0][e], o[1][e]), fmaxf(o[2][e], o[3][e]));
    unsigned short* y = a.y + (size_t)l.n * (a.P >> 1) * p.Wo * C + c0;
    *reinterpret_cast<uint4*>(y + (size_t)l.slot * C) = pack8(o[0]);
  } else {
    unsigned short* y = a.y + img + c0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (l.ok[j]) *reinterpret_cast<uint4*>(y + (size_t)l.pix[j] * C) = pack8(o[j]);
  }
}

template <int CGL, bool POOL>
__global__ __launch_bounds__(256) void gn_bwd_kernel(GnArgs a, Plan p) {
  constexpr int NG = 8 / CGL;
  constexpr int NV = 2 * NG > 8 ? 2 * NG : 8;
  __shared__ float lds[2 * NV * 256];
  const Lane l = locate<POOL>(a, p);
  const int C = a.C, c0 = l.chunk * 8;
  const size_t img = (size_t)l.n * a.P * a.Q * C;
  F8 x[4];  // z, then xhat
  load_tile(a.z + img + c0, l, C, x);
  F8 d[4];  // dy routed and masked (dyb), then dxhat
  if (POOL) {
    uint4 u = {0u, 0u, 0u, 0u};
    if (l.ok[0])
      u = *reinterpret_cast<const uint4*>(a.dy + (size_t)l.n * (a.P >> 1) * p.Wo * C + c0 +
                                          (size_t)l.slot * C);
    d[0] = cvt8(u);
  } else {
    load_tile(a.dy + img + c0, l, C, d);
  }

  float mu[NG], is[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int gi = CGL < 8 ? l.chunk * NG + g : l.chunk / p.lpg;
    const float* t = a.table + ((size_t)l.n * a.groups + gi) * 2;
    mu[g] = t[0];
    is[g] = t[1];
  }
  const F8 ga = ldf8(a.gamma + c0), be = ldf8(a.beta + c0);

  // ---- xhat, the recomputed pre-activation, the gradient's route; per-channel sums of this lane
  float sg[8], sb[8];  // sum dyb * xhat, sum dyb
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float pre[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j].v[e] = xhat_of(x[j].v[e], mu[e / CGL], is[e / CGL]);
      pre[j] = pre_of(x[j].v[e], ga.v[e], be.v[e]);
    }
    if (POOL) {
      // the window's first maximum in row-major order (strict >), of the activation
      const float g0 = d[0].v[e];
      int arg = 0;
      float best = a.relu ? fmaxf(pre[0], 0.f) : pre[0];
#pragma unroll
      for (int j = 1; j < 4; ++j) {
        const float v = a.relu ? fmaxf(pre[j], 0.f) : pre[j];
        if (v > best) { best = v; arg = j; }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        d[j].v[e] = (j == arg && (!a.relu || pre[j] > 0.f)) ? g0 : 0.f;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (a.relu && !(pre[j] > 0.f)) d[j].v[e] = 0.f;
    }
    float tg = 0.f, tb = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // (vectors outside the image hold dyb = 0)
      tg = __builtin_fmaf(d[j].v[e], x[j].v[e], tg);
      tb += d[j].v[e];
    }
    sg[e] = tg;
    sb[e] = tb;
  }

  // ---- the group's A = sum dxhat and B = sum dxhat * xhat, from the channel sums
  float ab[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) ab[i] = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    ab[e / CGL] = __builtin_fmaf(ga.v[e], sb[e], ab[e / CGL]);
    ab[NG + e / CGL] = __builtin_fmaf(ga.v[e], sg[e], ab[NG + e / CGL]);
  }
  group_sum<NV>(ab, lds, l, p);

  // ---- dz = is * (dxhat - A / m - xhat * B / m)
  float sz[8];
  unsigned short* dz = a.dz + img + c0;
#pragma unroll
  for (int e = 0; e < 8; ++e) sz[e] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float kA = ab[e / CGL] * p.inv_m, kB = ab[NG + e / CGL] * p.inv_m;
      const float t = __builtin_fmaf(-x[j].v[e], kB, d[j].v[e] * ga.v[e] - kA);
      o[e] = is[e / CGL] * t;
      if (l.ok[j]) sz[e] += o[e];
    }
    if (l.ok[j]) *reinterpret_cast<uint4*>(dz + (size_t)l.pix[j] * C) = pack8(o);
  }

  // ---- per-channel partials [n][3][C]: the lanes of a chunk lane, added in slot order
  float* ws = a.ws + (size_t)l.n * 3 * C + c0;
  const bool writer = l.live && l.slot == 0;
  slot_sum<8>(sg, lds, l, p);
  if (writer)
#pragma unroll
    for (int e = 0; e < 8; ++e) ws[e] = sg[e];
  slot_sum<8>(sb, lds, l, p);
  if (writer)
#pragma unroll
    for (int e = 0; e < 8; ++e) ws[C + e] = sb[e];
  if (a.dbias) {
    slot_sum<8>(sz, lds, l, p);
    if (writer)
#pragma unroll
      for (int e = 0; e < 8; ++e) ws[2 * C + e] = sz[e];
  }
}

// (dgamma, dbeta, dbias)[c] += the partials over n. A block owns 32 of the 3 C elements; eight
// lanes per element each add every eighth image in image order, then one lane adds the eight sums
// in lane order: a fixed order (dwconv.hip's finish).
__global__ __launch_bounds__(256) void gn_finish_kernel(GnArgs a) {
  __shared__ float red[8][32];
  const int el = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + el, total = (a.dbias ? 3 : 2) * a.C;
  float s = 0.f;
  const int q = e < a.C ? 0 : (e < 2 * a.C ? 1 : 2), c = e - q * a.C;
  if (e < total) {
#pragma unroll 4
    for (int n = part; n < a.N; n += 8) s += a.ws[((size_t)n * 3 + q) * a.C + c];
  }
  red[part][el] = s;
  __syncthreads();
  if (part == 0 && e < total) {
    float v = red[0][el];
#pragma unroll
    for (int i = 1; i < 8; ++i) v += red[i][el];
    float* dst = q == 0 ? a.dgamma : (q == 1 ? a.dbeta : a.dbias);
    dst[c] += v;
  }
}

// ------------------------------------------------------------------ host side
static bool served(int N, int P, int Q, int C, int groups, int pool) {
  if (N < 1 || P < 1 || Q < 1 || C < 8 || C % 8 || groups < 1 || C % groups) return false;
  const int Cg = C / groups;
  if (Cg > 64 || (Cg & (Cg - 1))) return false;
  if (pool && ((P | Q) & 1)) return false;
  if ((long long)std::max(8, Cg) * P * Q > kBudget) return false;
  if ((long long)N * P * Q * C >= 0x80000000ll) return false;
  return true;
}

static Plan plan(const GnArgs& a) {
  Plan p{};
  const int Cg = a.C / a.groups, nch = a.C / 8;
  p.lpg = std::max(1, Cg / 8);
  const int units = a.pool ? a.P * a.Q / 4 : a.P * a.Q;
  // the widest slab of whole groups whose tile fits four vectors (one window) per lane; lpg
  // always fits: 256 / lpg * 4 pixels * max(8, Cg) channels = kBudget
  for (int cl = std::min(64, nch); cl >= p.lpg; --cl) {
    if (nch % cl || cl % p.lpg) continue;
    if (units <= 256 / cl * (a.pool ? 1 : 4)) { p.CL = cl; break; }
  }
  p.nslots = 256 / p.CL;
  p.nslab = nch / p.CL;
  p.Wo = std::max(1, a.Q / 2);
  p.inv_m = 1.f / (float)(Cg * a.P * a.Q);
  p.dCL = make_fastdiv(p.CL);
  p.dWo = make_fastdiv(p.Wo);
  p.dSlab = make_fastdiv(p.nslab);
  return p;
}

template <bool BWD, int CGL>
static void launch2(const GnArgs& a, const Plan& p, hipStream_t st) {
  const dim3 grid(a.N * p.nslab);
  if (BWD) {
    if (a.pool) hipLaunchKernelGGL((gn_bwd_kernel<CGL, true>), grid, dim3(256), 0, st, a, p);
    else hipLaunchKernelGGL((gn_bwd_kernel<CGL, false>), grid, dim3(256), 0, st, a, p);
  } else {
    if (a.pool) hipLaunchKernelGGL((gn_fwd_kernel<CGL, true>), grid, dim3(256), 0, st, a, p);
    else hipLaunchKernelGGL((gn_fwd_kernel<CGL, false>), grid, dim3(256), 0, st, a, p);
  }
}

template <bool BWD>
static int launch(const GnArgs& a, hipStream_t st) {
  const Plan p = plan(a);
  switch (std::min(8, a.C / a.groups)) {
    case 1: launch2<BWD, 1>(a, p, st); break;
    case 2: launch2<BWD, 2>(a, p, st); break;
    case 4: launch2<BWD, 4>(a, p, st); break;
    default: launch2<BWD, 8>(a, p, st); break;
  }
  return (int)hipGetLastError();
}

}  // namespace gn
}  // namespace ddp_amd

using namespace ddp_amd;

extern "C" int ddp_gn_ok(int N, int P, int Q, int C, int groups, int pool) {
  return gn::served(N, P, Q, C, groups, pool) ? 1 : 0;
}

extern "C" int ddp_gn_act_fwd(const GnArgs* a, hipStream_t st) {
  if (!a || !gn::served(a->N, a->P, a->Q, a->C, a->groups, a->pool)) return -1;
  if (!a->z || !a->y || !a->gamma || !a->beta || !a->table) return -1;
  return gn::launch<false>(*a, st);
}

extern "C" int ddp_gn_act_bwd(const GnArgs* a, hipStream_t st) {
  if (!a || !gn::served(a->N, a->P, a->Q, a->C, a->groups, a->pool)) return -1;
  if (!a->z || !a->dy || !a->dz || !a->gamma || !a->beta || !a->table || !a->dgamma ||
      !a->dbeta || !a->ws)
    return -1;
  if (a->ws_elems < (size_t)a->N * 3 * a->C) return -2;
  const int rc = gn::launch<true>(*a, st);
  if (rc) return rc;
  const int total = (a->dbias ? 3 : 2) * a->C;
  hipLaunchKernelGGL(gn::gn_finish_kernel, dim3((total + 31) / 32), dim3(256), 0, st, *a);
  return (int)hipGetLastError();
}
