// Ghost BatchNorm + ReLU (+ 2x2 max-pool) for gfx950, forward and backward (bf16 NHWC
// activations, fp32 parameters and arithmetic). Statistics are taken over fixed-size groups of
// images, interleaved as the sharded sampler deals them: with ngroups = ceil(N / ghost), image n
// belongs to group g = n % ngroups; cnt_g images, m_g = cnt_g * P * Q elements per channel.
//   y  = pool2x2?(relu?(gamma_c * (z - mu_{g,c}) * is_{g,c} + beta_c)),  is = rsqrt(var + eps)
//   dz = gamma_c * is * (dyb - S1 / m - xhat * S2 / m),  S1 = sum dyb, S2 = sum dyb * xhat over
//        the group, dyb the gradient routed to the window's first maximum and through the ReLU
//        mask;  dgamma = sum_g S2_g,  dbeta = sum_g S1_g.
// The sets of images that share statistics are the same for every world size that divides
// N / ghost, and so are the bits: a group's plan below never looks at ngroups or N.
//
// No MFMA: there is no matrix product here. No float atomics: two runs give the same bits.
//
// Design: streaming over resident chunks, two launches each way.
//   * A (group, channel slab) does not fit a workgroup's registers as group_norm.hip's one-image
//     tile does (VGG layer 0 at ghost 32: 32 x 32 x 32 pixels x 8 channels = 512 KB), and one
//     block per (group, slab) would leave most of the 256 CUs idle. So a work item is (group,
//     chunk, slab): a chunk is a contiguous range of the group's slots, a slot being one pixel
//     (pooled: one 2x2 window) of one image of the group, images in group order. A chunk is held
//     in registers as group_norm.hip holds its tile: at most 8192 elements per block of 256
//     lanes, a lane owning one 8-channel 16-byte vector of up to four pixels; pooled, the four
//     pixels of ONE window, so the max, the first-maximum position and the gradient routing stay
//     inside a lane. tid = lane slot * CL + chunk lane; unpooled, a lane's slots are
//     lane slot + j * (256 / CL), j = 0..3. Chunks may cross image boundaries.
//   * Slab width CL (chunk lanes of 8 channels), as gn::Plan: the widest divisor of C / 8, at
//     most 64, for which one image fits a chunk. 32x32 (VGG layer 0) gets CL = 1 (xcd_remap puts
//     the slabs of a chunk on one XCD so the 128-byte line's other readers find it in that L2),
//     16x16 CL = 4, 8x8 and below whole lines. The plan of a group depends only on (cnt_g, P, Q,
//     C, pool).
//   * Forward 1, gbn_stats_kernel: a block forms its chunk's mean and centred sum of squares per
//     channel from the resident registers (no E[z^2] - mu^2 form), lanes combined in a fixed
//     order (CL in 1, 2, 4, 8: DPP row rotations, then the 16 rows in LDS in row order;
//     otherwise LDS in slot order, every 16th slot by one lane, then the 16 results), and writes
//     (mean_b, M2_b) partials [item][2][8 CL] with plain vector stores.
//   * Forward 2, gbn_apply_kernel: the prologue merges the group's partials per channel in chunk
//     order with the pairwise (Chan) update, one thread per channel, and leaves (mu, is) in LDS;
//     the block of chunk 0 stores them to the table [ngroups][2][C]. Then every block reads its
//     chunk of z again and writes y. The second read is ASSUMED to come from L2 (same work item
//     -> same XCD in both launches); that has not been measured.
//   * Backward 1, gbn_bwd_reduce_kernel: reads the chunk of z and dy, recomputes xhat and the
//     pre-activation from the table with the forward's own expressions (no masks or indices are
//     saved) and writes per-channel (S2, S1) partials.
//   * Backward 2, gbn_bwd_apply_kernel: the prologue adds the group's partials in chunk order;
//     the block recomputes xhat / dyb and writes dz. The blocks of (group 0, chunk 0) also add
//     dgamma / dbeta onto the gradient arena: group sums (each in chunk order) added in group
//     order. The producing conv's bias gradient is analytically zero (sum dz = 0 per group).
//
// Resource usage: compiler output of -Rpass-analysis=kernel-resource-usage for gfx950 at -O3,
// NOT a measurement; <no pool> / <pool>:
//   gbn_stats_kernel:       55 / 55 VGPRs,   scratch 0, LDS 16 KB, 8 / 8 waves / SIMD
//   gbn_apply_kernel:       65 / 62 VGPRs,   scratch 0, LDS 4 KB,  7 / 8 waves / SIMD
//   gbn_bwd_reduce_kernel:  105 / 79 VGPRs,  scratch 0, LDS 16 KB, 4 / 6 waves / SIMD
//   gbn_bwd_apply_kernel:   103 / 118 VGPRs, scratch 0, LDS 4 KB,  4 / 4 waves / SIMD
// No kernel of this file uses scratch.
//
// Limits (ddp_gbn_ok): C % 8 == 0, N >= 1, ghost >= 1, even P and Q with the pool, tensors below
// 2^31 elements, items * 16 CL floats of partials within the workspace passed in. Out of scope:
// a one-launch variant for groups that fit one block, running statistics.
#include "common.h"
#include "api.h"
#include "norm_tile.h"

#include <algorithm>

namespace ddp_amd {
namespace gbn {

using namespace tile;  // F8, cvt8, pack8, ldf8, xhat_of, pre_of

constexpr int kFold = 16;   // slots added by one lane in the first LDS phase
constexpr int kMaxW = 512;  // channels of the widest slab (CL = 64)

struct Plan {
  int CL, nslots, nslab;  // chunk lanes, lane slots of a block, slabs
  int U, Wo, cap;         // slots per image, pooled width, slots per chunk
  int ngroups, nbig, cnt; // the first nbig groups hold cnt + 1 images, the others cnt
  int nch[2], items[2];   // chunks / work items of a (big, small) group
  int nblocks;
  FastDiv dCL, dU, dWo, dSlab, dItems[2];
};

// This block's work item (uniform over the block).
struct Item {
  int id;          // logical item = index of its partials
  int g, k, slab;  // group, chunk, slab
  int nch, base;   // chunks of the group, its first item
  int S, s0;       // slots of the group, first slot of the chunk
};

__device__ __forceinline__ int group_images(const Plan& p, int g) { return p.cnt + (g < p.nbig); }
__device__ __forceinline__ int group_chunks(const Plan& p, int g) {
  return g < p.nbig ? p.nch[0] : p.nch[1];
}
__device__ __forceinline__ int group_base(const Plan& p, int g) {
  return g < p.nbig ? g * p.items[0] : p.nbig * p.items[0] + (g - p.nbig) * p.items[1];
}

__device__ __forceinline__ Item item_of(const Plan& p) {
  Item it;
  it.id = xcd_remap(blockIdx.x, gridDim.x);
  const int split = p.nbig * p.items[0];
  int rem;
  if (it.id < split) {
    it.g = fast_div(it.id, p.dItems[0]);
    rem = it.id - it.g * p.items[0];
  } else {
    const int gi = fast_div(it.id - split, p.dItems[1]);
    it.g = p.nbig + gi;
    rem = it.id - split - gi * p.items[1];
  }
  it.base = it.id - rem;
  it.nch = group_chunks(p, it.g);
  it.k = fast_div(rem, p.dSlab);
  it.slab = rem - it.k * p.nslab;
  it.S = group_images(p, it.g) * p.U;
  it.s0 = it.k * p.cap;
  return it;
}

// per-channel element count of chunk k of a group with S slots
template <bool POOL>
__device__ __forceinline__ float chunk_count(const Plan& p, int S, int k) {
  return (float)(min(p.cap, S - k * p.cap) * (POOL ? 4 : 1));
}

// This thread's place in the chunk. Idle lanes (past the last whole lane slot, when CL does not
// divide 256) take slot = nslots, chunk lane 0: they add zeros, read live cells, write nothing.
struct Lane {
  int slot, cl;
  bool live;
  bool ok[4];  // its vector j lies in the group
  int pix[4];  // ... at this pixel of the batch ((n * P + p) * Q + q)
  int out;     // pooled: its window in the pooled tensor ((n * Ho + wp) * Wo + wq)
};

template <bool POOL>
__device__ __forceinline__ Lane locate(const GhostBnArgs& a, const Plan& p, const Item& it) {
  Lane l;
  l.slot = fast_div((int)threadIdx.x, p.dCL);
  l.cl = threadIdx.x - l.slot * p.CL;
  l.live = l.slot < p.nslots;
  if (!l.live) { l.slot = p.nslots; l.cl = 0; }
  l.out = 0;
  if (POOL) {
    const int s = it.s0 + l.slot;
    const bool v = l.live && s < it.S;
    const int i = fast_div(s, p.dU), u = s - i * p.U, n = it.g + i * p.ngroups;
    const int wp = fast_div(u, p.dWo), wq = u - wp * p.Wo;
    l.out = v ? n * p.U + u : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      l.ok[j] = v;
      l.pix[j] = v ? (n * a.P + 2 * wp + (j >> 1)) * a.Q + 2 * wq + (j & 1) : 0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = it.s0 + l.slot + j * p.nslots;
      l.ok[j] = l.live && s < it.S;
      const int i = fast_div(s, p.dU), u = s - i * p.U, n = it.g + i * p.ngroups;
      l.pix[j] = l.ok[j] ? n * p.U + u : 0;
    }
  }
  return l;
}

// v[i] <- the sum of v[i] over the ``nslots`` lanes cl, stride + cl, 2 stride + cl, ... of the
// block, in a fixed order, delivered to each of them. lds: 2 * NV * 256 floats, [value][lane].
template <int NV>
__device__ __forceinline__ void slot_sum(float (&v)[NV], float* lds, int slot, int cl, int nslots,
                                         int stride) {
  float* A = lds;
  float* B = lds + NV * 256;
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < NV; ++i) A[i * 256 + tid] = v[i];
  __syncthreads();
  const float* src = A;
  const int rows = min(kFold, nslots);
  if (nslots > kFold) {
    if (slot < rows) {  // (an idle lane's slot is nslots >= rows)
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        float t = A[i * 256 + tid];
        for (int s = slot + kFold; s < nslots; s += kFold) t += A[i * 256 + s * stride + cl];
        B[i * 256 + tid] = t;
      }
    }
    __syncthreads();
    src = B;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    float t = src[i * 256 + cl];
    for (int s = 1; s < rows; ++s) t += src[i * 256 + s * stride + cl];
    v[i] = t;
  }
  __syncthreads();  // the next call writes A (and B) again
}

// The block's sum per chunk lane. CL in {1, 2, 4, 8} (it divides a DPP row of 16 lanes, no idle
// lanes): the row's lanes of one chunk lane are added by row rotations (every lane of the class
// ends with the same bits: a + b is commutative and the operands of each step are shared), then
// the 16 rows in LDS in row order. Otherwise LDS alone, in slot order. All 256 threads call it.
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* lds, const Lane& l, const Plan& p) {
  const int CL = p.CL;
  if (CL <= 8 && (CL & (CL - 1)) == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      v[i] += dpp_f<0x128>(v[i]);               // row_ror:8
      if (CL <= 4) v[i] += dpp_f<0x124>(v[i]);  // row_ror:4
      if (CL <= 2) v[i] += dpp_f<0x122>(v[i]);  // row_ror:2
      if (CL <= 1) v[i] += dpp_f<0x121>(v[i]);  // row_ror:1
    }
    slot_sum<NV>(v, lds, threadIdx.x >> 4, threadIdx.x & 15, 16, 16);
  } else {
    slot_sum<NV>(v, lds, l.slot, l.cl, p.nslots, CL);
  }
}

// the chunk's vectors as fp32 (zeros outside the group)
__device__ __forceinline__ void load_tile(const unsigned short* base, const Lane& l, int C,
                                          F8 (&t)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint4 u = {0u, 0u, 0u, 0u};
    if (l.ok[j]) u = *reinterpret_cast<const uint4*>(base + (size_t)l.pix[j] * C);
    t[j] = cvt8(u);
  }
}

// dy of the chunk: pooled, the window's one vector in d[0]
template <bool POOL>
__device__ __forceinline__ void load_dy(const unsigned short* base, const Lane& l, int C,
                                        F8 (&d)[4]) {
  if (POOL) {
    uint4 u = {0u, 0u, 0u, 0u};
    if (l.ok[0]) u = *reinterpret_cast<const uint4*>(base + (size_t)l.out * C);
    d[0] = cvt8(u);
  } else {
    load_tile(base, l, C, d);
  }
}

// x: z -> xhat; d: dy -> dyb, the gradient at the pre-activation (routed to the window's first
// maximum in row-major order, strict >, and through the ReLU mask). Vectors outside the group
// end with dyb = 0. Both backward kernels call this, so they see the same dyb.
template <bool POOL>
__device__ __forceinline__ void route(F8 (&x)[4], F8 (&d)[4], const F8& mu, const F8& is,
                                      const F8& ga, const F8& be, int relu) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float pre[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j].v[e] = xhat_of(x[j].v[e], mu.v[e], is.v[e]);
      pre[j] = pre_of(x[j].v[e], ga.v[e], be.v[e]);
    }
    if (POOL) {
      const float g0 = d[0].v[e];
      int arg = 0;
      float best = relu ? fmaxf(pre[0], 0.f) : pre[0];
#pragma unroll
      for (int j = 1; j < 4; ++j) {
        const float v = relu ? fmaxf(pre[j], 0.f) : pre[j];
        if (v > best) { best = v; arg = j; }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j].v[e] = (j == arg && (!relu || pre[j] > 0.f)) ? g0 : 0.f;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (relu && !(pre[j] > 0.f)) d[j].v[e] = 0.f;
    }
  }
}

// ------------------------------------------------------------------ forward
template <bool POOL>
__global__ __launch_bounds__(256) void gbn_stats_kernel(GhostBnArgs a, Plan p) {
  __shared__ float lds[2 * 8 * 256];
  const Item it = item_of(p);
  const Lane l = locate<POOL>(a, p, it);
  const int c0 = (it.slab * p.CL + l.cl) * 8;
  F8 z[4];
  load_tile(a.z + c0, l, a.C, z);
  const float nb = chunk_count<POOL>(p, it.S, it.k);

  float mean[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) mean[e] = (z[0].v[e] + z[1].v[e]) + (z[2].v[e] + z[3].v[e]);
  block_sum<8>(mean, lds, l, p);
#pragma unroll
  for (int e = 0; e < 8; ++e) mean[e] = mean[e] / nb;

  float m2[8];  // centred, from the resident chunk
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = l.ok[j] ? z[j].v[e] - mean[e] : 0.f;
      t = __builtin_fmaf(d, d, t);
    }
    m2[e] = t;
  }
  block_sum<8>(m2, lds, l, p);

  if (l.live && l.slot == 0) {
    const int W = p.CL * 8;
    float* ws = a.ws + (size_t)it.id * 2 * W + l.cl * 8;
    *reinterpret_cast<float4*>(ws) = make_float4(mean[0], mean[1], mean[2], mean[3]);
    *reinterpret_cast<float4*>(ws + 4) = make_float4(mean[4], mean[5], mean[6], mean[7]);
    *reinterpret_cast<float4*>(ws + W) = make_float4(m2[0], m2[1], m2[2], m2[3]);
    *reinterpret_cast<float4*>(ws + W + 4) = make_float4(m2[4], m2[5], m2[6], m2[7]);
  }
}

template <bool POOL>
__global__ __launch_bounds__(256) void gbn_apply_kernel(GhostBnArgs a, Plan p) {
  __shared__ float tab[2 * kMaxW];  // (mu, is) of the slab's channels
  const Item it = item_of(p);
  const Lane l = locate<POOL>(a, p, it);
  const int C = a.C, W = p.CL * 8;

  // ---- the group's partials in chunk order, Chan's pairwise update; one thread per channel
  const float* ws = a.ws + ((size_t)it.base + it.slab) * 2 * W;
  const size_t step = (size_t)p.nslab * 2 * W;
  for (int c = threadIdx.x; c < W; c += 256) {
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int k = 0; k < it.nch; ++k) {
      const float nb = chunk_count<POOL>(p, it.S, k);
      const float pm = ws[k * step + c], pq = ws[k * step + W + c];
      const float nt = n + nb, delta = pm - mean;
      mean = __builtin_fmaf(delta, nb / nt, mean);
      m2 = (m2 + pq) + (delta * delta) * (n * nb / nt);
      n = nt;
    }
    const float is = rsqrtf(m2 / n + a.eps);
    tab[c] = mean;
    tab[kMaxW + c] = is;
    if (it.k == 0) {
      float* t = a.table + (size_t)it.g * 2 * C + it.slab * W + c;
      t[0] = mean;
      t[C] = is;
    }
  }
  __syncthreads();

  // ---- normalise, ReLU, pool
  const int c0 = (it.slab * p.CL + l.cl) * 8;
  const F8 mu = ldf8(tab + l.cl * 8), is = ldf8(tab + kMaxW + l.cl * 8);
  const F8 ga = ldf8(a.gamma + c0), be = ldf8(a.beta + c0);
  F8 z[4];
  load_tile(a.z + c0, l, C, z);
  float o[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = pre_of(xhat_of(z[j].v[e], mu.v[e], is.v[e]), ga.v[e], be.v[e]);
      o[j][e] = a.relu ? fmaxf(v, 0.f) : v;
    }
  unsigned short* y = a.y + c0;
  if (POOL) {
    if (!l.ok[0]) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[0][e] = fmaxf(fmaxf(o[0][e], o[1][e]), fmaxf(o[2][e], o[3][e]));
    *reinterpret_cast<uint4*>(y + (size_t)l.out * C) = pack8(o[0]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (l.ok[j]) *reinterpret_cast<uint4*>(y + (size_t)l.pix[j] * C) = pack8(o[j]);
  }
}

// ------------------------------------------------------------------ backward
template <bool POOL>
__global__ __launch_bounds__(256) void gbn_bwd_reduce_kernel(GhostBnArgs a, Plan p) {
  __shared__ float lds[2 * 8 * 256];
  const Item it = item_of(p);
  const Lane l = locate<POOL>(a, p, it);
  const int C = a.C, c0 = (it.slab * p.CL + l.cl) * 8;
  F8 x[4], d[4];
  load_tile(a.z + c0, l, C, x);
  load_dy<POOL>(a.dy + c0, l, C, d);
  const float* t = a.table + (size_t)it.g * 2 * C + c0;
  route<POOL>(x, d, ldf8(t), ldf8(t + C), ldf8(a.gamma + c0), ldf8(a.beta + c0), a.relu);

  float s2[8], s1[8];  // sum dyb * xhat, sum dyb
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float tg = 0.f, tb = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tg = __builtin_fmaf(d[j].v[e], x[j].v[e], tg);
      tb += d[j].v[e];
    }
    s2[e] = tg;
    s1[e] = tb;
  }
  block_sum<8>(s2, lds, l, p);
  block_sum<8>(s1, lds, l, p);
  if (l.live && l.slot == 0) {
    const int W = p.CL * 8;
    float* ws = a.ws + (size_t)it.id * 2 * W + l.cl * 8;
    *reinterpret_cast<float4*>(ws) = make_float4(s2[0], s2[1], s2[2], s2[3]);
    *reinterpret_cast<float4*>(ws + 4) = make_float4(s2[4], s2[5], s2[6], s2[7]);
    *reinterpret_cast<float4*>(ws + W) = make_float4(s1[0], s1[1], s1[2], s1[3]);
    *reinterpret_cast<float4*>(ws + W + 4) = make_float4(s1[4], s1[5], s1[6], s1[7]);
  }
}

// (S2, S1)[c] of group g's slab: its partials added in chunk order
__device__ __forceinline__ void group_sums(const GhostBnArgs& a, const Plan& p, int g, int slab,
                                           int c, float& s2, float& s1) {
  const int W = p.CL * 8, nch = group_chunks(p, g);
  const float* ws = a.ws + ((size_t)group_base(p, g) + slab) * 2 * W;
  const size_t step = (size_t)p.nslab * 2 * W;
  s2 = 0.f;
  s1 = 0.f;
  for (int k = 0; k < nch; ++k) {
    s2 += ws[k * step + c];
    s1 += ws[k * step + W + c];
  }
}

template <bool POOL>
__global__ __launch_bounds__(256) void gbn_bwd_apply_kernel(GhostBnArgs a, Plan p) {
  __shared__ float tab[2 * kMaxW];  // (S2 / m, S1 / m) of the slab's channels
  const Item it = item_of(p);
  const Lane l = locate<POOL>(a, p, it);
  const int C = a.C, W = p.CL * 8;
  const float inv_m = 1.f / (float)(group_images(p, it.g) * a.P * a.Q);
  for (int c = threadIdx.x; c < W; c += 256) {
    float s2, s1;
    group_sums(a, p, it.g, it.slab, c, s2, s1);
    tab[c] = s2 * inv_m;
    tab[kMaxW + c] = s1 * inv_m;
    if (it.g == 0 && it.k == 0) {
      // dgamma / dbeta: the groups' sums in group order, onto what the arena holds
      for (int g = 1; g < p.ngroups; ++g) {
        float t2, t1;
        group_sums(a, p, g, it.slab, c, t2, t1);
        s2 += t2;
        s1 += t1;
      }
      a.dgamma[it.slab * W + c] += s2;
      a.dbeta[it.slab * W + c] += s1;
    }
  }
  __syncthreads();

  const int c0 = (it.slab * p.CL + l.cl) * 8;
  F8 x[4], d[4];
  load_tile(a.z + c0, l, C, x);
  load_dy<POOL>(a.dy + c0, l, C, d);
  const float* t = a.table + (size_t)it.g * 2 * C + c0;
  const F8 is = ldf8(t + C), ga = ldf8(a.gamma + c0);
  route<POOL>(x, d, ldf8(t), is, ga, ldf8(a.beta + c0), a.relu);
  const F8 k2 = ldf8(tab + l.cl * 8), k1 = ldf8(tab + kMaxW + l.cl * 8);

  // ---- dz = gamma * is * (dyb - S1 / m - xhat * S2 / m)
  unsigned short* dz = a.dz + c0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o[e] = (ga.v[e] * is.v[e]) * __builtin_fmaf(-x[j].v[e], k2.v[e], d[j].v[e] - k1.v[e]);
    if (l.ok[j]) *reinterpret_cast<uint4*>(dz + (size_t)l.pix[j] * C) = pack8(o);
  }
}

// ------------------------------------------------------------------ host side
static bool shape_ok(int N, int P, int Q, int C, int ghost, int pool) {
  if (N < 1 || P < 1 || Q < 1 || C < 8 || C % 8 || ghost < 1) return false;
  if (pool && ((P | Q) & 1)) return false;
  if ((long long)N * P * Q * C >= 0x80000000ll) return false;
  return true;
}

static Plan plan(int N, int P, int Q, int C, int ghost, int pool) {
  Plan p{};
  const int nvec = C / 8;
  p.U = pool ? P * Q / 4 : P * Q;
  p.Wo = std::max(1, Q / 2);
  // the widest slab for which one image fits a chunk (four vectors, or one window, per lane);
  // larger images stream at CL = 1
  p.CL = 1;
  for (int cl = std::min(64, nvec); cl > 1; --cl) {
    if (nvec % cl) continue;
    if (p.U <= 256 / cl * (pool ? 1 : 4)) { p.CL = cl; break; }
  }
  p.nslots = 256 / p.CL;
  p.nslab = nvec / p.CL;
  p.cap = p.nslots * (pool ? 1 : 4);
  p.ngroups = (int)(((long long)N + ghost - 1) / ghost);
  p.nbig = N % p.ngroups;
  p.cnt = N / p.ngroups;
  for (int i = 0; i < 2; ++i) {
    const long long S = (long long)(p.cnt + 1 - i) * p.U;
    p.nch[i] = (int)((S + p.cap - 1) / p.cap);
    p.items[i] = p.nch[i] * p.nslab;
    p.dItems[i] = make_fastdiv(p.items[i]);
  }
  p.nblocks = p.nbig * p.items[0] + (p.ngroups - p.nbig) * p.items[1];
  p.dCL = make_fastdiv(p.CL);
  p.dU = make_fastdiv(p.U);
  p.dWo = make_fastdiv(p.Wo);
  p.dSlab = make_fastdiv(p.nslab);
  return p;
}

static size_t ws_need(const Plan& p) { return (size_t)p.nblocks * 16 * p.CL; }

#define GBN_LAUNCH(kernel)                                                                  \
  do {                                                                                      \
    if (a.pool) hipLaunchKernelGGL((kernel<true>), dim3(p.nblocks), dim3(256), 0, st, a, p); \
    else hipLaunchKernelGGL((kernel<false>), dim3(p.nblocks), dim3(256), 0, st, a, p);       \
  } while (0)

}  // namespace gbn
}  // namespace ddp_amd

using namespace ddp_amd;

extern "C" size_t ddp_gbn_ws_elems(int N, int P, int Q, int C, int ghost, int pool) {
  if (!gbn::shape_ok(N, P, Q, C, ghost, pool)) return 0;
  return gbn::ws_need(gbn::plan(N, P, Q, C, ghost, pool));
}

extern "C" int ddp_gbn_ok(int N, int P, int Q, int C, int ghost, int pool, size_t ws_elems) {
  if (!gbn::shape_ok(N, P, Q, C, ghost, pool)) return 0;
  return gbn::ws_need(gbn::plan(N, P, Q, C, ghost, pool)) <= ws_elems ? 1 : 0;
}

extern "C" int ddp_gbn_act_fwd(const GhostBnArgs* ap, hipStream_t st) {
  if (!ap || !ddp_gbn_ok(ap->N, ap->P, ap->Q, ap->C, ap->ghost, ap->pool, ap->ws_elems)) return -1;
  const GhostBnArgs& a = *ap;
  if (!a.z || !a.y || !a.gamma || !a.beta || !a.table || !a.ws) return -1;
  const gbn::Plan p = gbn::plan(a.N, a.P, a.Q, a.C, a.ghost, a.pool);
  GBN_LAUNCH(gbn::gbn_stats_kernel);
  GBN_LAUNCH(gbn::gbn_apply_kernel);
  return (int)hipGetLastError();
}

extern "C" int ddp_gbn_act_bwd(const GhostBnArgs* ap, hipStream_t st) {
  if (!ap || !ddp_gbn_ok(ap->N, ap->P, ap->Q, ap->C, ap->ghost, ap->pool, ap->ws_elems)) return -1;
  const GhostBnArgs& a = *ap;
  if (!a.z || !a.dy || !a.dz || !a.gamma || !a.beta || !a.table || !a.dgamma || !a.dbeta || !a.ws)
    return -1;
  const gbn::Plan p = gbn::plan(a.N, a.P, a.Q, a.C, a.ghost, a.pool);
  GBN_LAUNCH(gbn::gbn_bwd_reduce_kernel);
  GBN_LAUNCH(gbn::gbn_bwd_apply_kernel);
  return (int)hipGetLastError();
}
