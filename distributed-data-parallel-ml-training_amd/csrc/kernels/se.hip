// Squeeze-and-Excitation tail of a bottleneck for gfx950, forward and backward (bf16 NHWC
// activations, fp32 parameters, tables and arithmetic):
//   u = a_c z + b_c                       bn3 as its coefficient table (a = gamma * invstd)
//   m[n,c] = mean_hw(u) = a_c S[n,c] / HW + b_c,   S[n,c] = sum_hw z
//   h = relu(W1 m + b1),  s = sigmoid(W2 h + b2)
//   y = relu(u * s[n,c] + res)
// The gate rides inside the block's BatchNorm passes. Because bn3 is affine per channel the
// squeeze reads z, not u, and the backward needs ONE reduce pass: with g = dy * [y > 0],
// G1 = sum_hw g, G2 = sum_hw g z,
//   ds[n,c] = a_c G2 + b_c G1,   du = g s + dm / HW   (dm = the gradient at m)
//   sum du = sum_n (s G1 + dm),  sum du z = sum_n (s G2 + dm S / HW)
// so everything between the two activation-sized passes works on [N][C] tables.
//
// Launches (ddp_se_fwd: 4, ddp_se_bwd: 4):
//   finalize    one thread per channel: statistics replicas -> coefficient table (bn_act.hip's
//               finalize_fwd_ch, the same expressions in the same order), running statistics
//   squeeze     S. A workgroup owns one image x a 64-channel slab (one 128-byte line per pixel:
//               8 chunk lanes of 16 bytes x 32 pixel slots), or a fixed pixel range of it when
//               N * C / 64 workgroups would not fill the machine. Lanes add their pixels in
//               pixel order, the 32 slots meet in LDS and are added in slot order; split pixel
//               ranges go as fp32 partials [split][N][C] into the workspace and their consumer
//               (excite) adds them in split order and writes S. No float atomics.
//   excite      one workgroup = 16 images (the M of v_mfma_f32_16x16x32_bf16) x a 256-channel
//               chunk of the gate. GEMM1 [16 x C] . [C x Cr]: the four waves take every fourth
//               32-wide k-step over all Cr / 16 column tiles and meet in LDS (wave order); the
//               A fragment is formed in registers from S and the table, the B fragment is read
//               as fp32 from W1 [Cr][C] and rounded in registers: no packed copy, no LDS staging
//               (each operand element is used by one lane once). h stays in LDS; GEMM2
//               [16 x Cr] . [Cr x 256] gives each wave four column tiles. GEMM1 is recomputed by
//               every chunk (at most 8 x a tiny GEMM) for a grid of ceil(N / 16) * ceil(C / 256)
//               without a second launch.
//   apply       y and the ReLU mask bits (BnArgs::mask format), one thread = 8 channels of
//               4 pixels, tables read from L2.
//   reduce      G1, G2 from dy, the mask bits and z: squeeze's ownership and order.
//   excite_bwd  one workgroup per 16 images: ds, dt2 = ds s (1 - s), dh = (dt2 W2) [h > 0],
//               dm = dh W1 on MFMA, B fragments gathered with stride (k-major weights are read
//               as they lie; 64-byte runs per k).
//   param_bwd   owned by outputs, looping over the images in order (reduction length N, no
//               partials): 64 x 16 tiles of dW2 and dW1 on fp32 FMAs (operands NOT rounded to
//               bf16), db2, db1, the two BatchNorm sums, dgamma, dbeta, k1, k2.
//   apply_bwd   dz = a (du - k1 - xhat k2), dres = g.
//
// Store points (everything else is fp32 and never rounded):
//   GEMM1 operands  bf16(m) with m = fma(a, S * (1 / HW), b);  bf16(W1)
//   GEMM2 operands  bf16(h) with h = max(acc + b1, 0) (the fp32 h is what is stored);  bf16(W2)
//   s               fp32: 1 / (1 + expf(-(acc + b2)))
//   y               bf16(max(fma(fma(a, z, b), s, res), 0)); mask bit = that fma > 0
//   dh GEMM         bf16(dt2), bf16(W2);  dm GEMM: bf16(dh), bf16(W1)
//   dz              bf16(a * fma(-xhat, k2, fma(g, s, dm * (1 / HW)) - k1)), xhat = (z - mu) * is
//   dgamma          is * fma(-mu, T1, T2) with T1 = sum du, T2 = sum du z
//
// Where this leaves the usual design: no LDS staging of MFMA operands and no double buffering
// (the GEMMs are 16 rows tall and every operand element has one reader), fp32 weights read in
// place instead of packed bf16 copies (no work in the update launch; the table kernels are
// latency-, not bandwidth-bound), and the weight gradients on VALU FMAs (67 MFLOP at the widest
// layer; keeps them free of operand rounding).
//
// Resource usage: compiler output of -Rpass-analysis=kernel-resource-usage for gfx950 at -O3,
// NOT a measurement (VGPRs, AGPRs, scratch bytes, LDS bytes):
//   se_finalize_kernel          48,  0, 0,     0    8 waves / SIMD
//   se_sum_kernel<false>        40,  0, 0,  8192    8   (squeeze)
//   se_sum_kernel<true>         94,  0, 0, 16384    5   (reduce)
//   se_excite_kernel            90, 32, 0, 40960    4
//   se_apply_kernel<false>      68,  0, 0,     0    7
//   se_excite_bwd_kernel        98, 32, 0, 40960    3
//   se_param_bwd_kernel         66,  0, 0,     0    7
//   se_apply_kernel<true>       98,  0, 0,     0    4   (apply_bwd)
// No kernel of this file uses scratch.
//
// Limits (ddp_se_ok): C % 64 == 0, 64 <= C <= 2048, C % reduction == 0, Cr = C / reduction a
// multiple of 16 in 16..128, any N, P, Q >= 1 with P * Q * C and N * C below 2^31.
#include "common.h"
#include "api.h"

#include <algorithm>

namespace ddp_amd {
namespace se {

enum { kSc = 0, kSh = 1, kMu = 2, kIs = 3, kK1 = 4, kK2 = 5 };  // coef table rows (bn_act.hip)
constexpr int kTile = 16;     // images of one excite workgroup
constexpr int kChunk = 256;   // gate channels of one excite workgroup
constexpr int kMaxCr = 128;
constexpr int kIpt = 4;       // items per thread of the apply passes

struct Plan {
  int HW, G, Cr, nslab, nsplit, pps, nchunk, bpi, nrt, nbw, nbc;
  float inv_hw, inv_m;
  FastDiv dG, dSlab, dSS, dChunk, dBpi, dCr, dRt;
};

struct F8 { float v[8]; };

__device__ __forceinline__ F8 ldf8(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  return F8{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ void stf8(float* p, const F8& f) {
  *reinterpret_cast<float4*>(p) = make_float4(f.v[0], f.v[1], f.v[2], f.v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(f.v[4], f.v[5], f.v[6], f.v[7]);
}
__device__ __forceinline__ bf16x8 to_frag(const F8& f) {
  u16x8 u;
#pragma unroll
  for (int e = 0; e < 8; ++e) u[e] = f2bf(f.v[e]);
  return __builtin_bit_cast(bf16x8, u);
}
__device__ __forceinline__ bf16x8 zero_frag() {
  const u16x8 u = {0, 0, 0, 0, 0, 0, 0, 0};
  return __builtin_bit_cast(bf16x8, u);
}
// table[n][c0 .. c0 + 7] of a [parts][NV][N][C] partial set, parts added in part order
__device__ __forceinline__ F8 ld_parts(const float* part, int nparts, size_t part_stride,
                                       size_t off) {
  F8 r = ldf8(part + off);
  for (int sp = 1; sp < nparts; ++sp) {
    const F8 t = ldf8(part + sp * part_stride + off);
#pragma unroll
    for (int e = 0; e < 8; ++e) r.v[e] += t.v[e];
  }
  return r;
}

// ------------------------------------------------------------------ finalize
__global__ __launch_bounds__(256) void se_finalize_kernel(SeArgs a) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.C) return;
  float mu, is;
  if (a.use_running) {
    mu = a.running_mean[c];
    is = rsqrtf(a.running_var[c] + a.eps);
  } else {
    const float M = (float)a.N * a.P * a.Q;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int r = 0; r < kStatRep; ++r) {
      s1 += a.stats[r * 2 * a.C + c];
      s2 += a.stats[r * 2 * a.C + a.C + c];
    }
    mu = s1 / M;
    const float var = fmaxf(s2 / M - mu * mu, 0.f);
    is = rsqrtf(var + a.eps);
    if (a.running_mean) {
      const float unbiased = M > 1.f ? var * M / (M - 1.f) : var;
      a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * mu;
      a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * unbiased;
    }
  }
  const float sc = a.gamma[c] * is;
  a.coef[kSc * a.C + c] = sc;
  a.coef[kSh * a.C + c] = a.beta[c] - mu * sc;
  a.coef[kMu * a.C + c] = mu;
  a.coef[kIs * a.C + c] = is;
}

// ------------------------------------------------------------------ squeeze / reduce
// BWD = false: S = sum z into ``dst`` [split][1][N][C]; true: (G1, G2) into [split][2][N][C].
template <bool BWD>
__global__ __launch_bounds__(256) void se_sum_kernel(SeArgs a, Plan p, float* dst) {
  constexpr int NV = BWD ? 2 : 1;
  __shared__ __attribute__((aligned(16))) float lds[NV * 32 * 64];
  const int blk = blockIdx.x;
  const int n = fast_div(blk, p.dSS);
  const int rem = blk - n * (p.nslab * p.nsplit);
  const int split = fast_div(rem, p.dSlab), slab = rem - split * p.nslab;
  const int cl = threadIdx.x & 7, slot = threadIdx.x >> 3;
  const int chunk = slab * 8 + cl;
  const int p0 = split * p.pps, p1 = min(p.HW, p0 + p.pps);
  const size_t img = (size_t)n * p.HW;
  const unsigned short* z = a.z + img * a.C + chunk * 8;
  const unsigned short* dy = BWD ? a.dy + img * a.C + chunk * 8 : nullptr;
  const unsigned char* mk = BWD ? a.mask + img * p.G + chunk : nullptr;
  float s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s1[e] = s2[e] = 0.f;
#pragma unroll 4
  for (int px = p0 + slot; px < p1; px += 32) {
    const u16x8 zv = ld8(z + (size_t)px * a.C);
    if (BWD) {
      const u16x8 dv = ld8(dy + (size_t)px * a.C);
      const unsigned mb = mk[(size_t)px * p.G];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = ((mb >> e) & 1u) ? bf2f(dv[e]) : 0.f;
        s1[e] += g;
        s2[e] = __builtin_fmaf(g, bf2f(zv[e]), s2[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) s1[e] += bf2f(zv[e]);
    }
  }
  float* row = lds + slot * 64 + cl * 8;
  *reinterpret_cast<float4*>(row) = make_float4(s1[0], s1[1], s1[2], s1[3]);
  *reinterpret_cast<float4*>(row + 4) = make_float4(s1[4], s1[5], s1[6], s1[7]);
  if (BWD) {
    *reinterpret_cast<float4*>(row + 2048) = make_float4(s2[0], s2[1], s2[2], s2[3]);
    *reinterpret_cast<float4*>(row + 2052) = make_float4(s2[4], s2[5], s2[6], s2[7]);
  }
  __syncthreads();
  if (threadIdx.x < 64 * NV) {
    const int v = threadIdx.x >> 6, ch = threadIdx.x & 63;
    const float* col = lds + v * 2048 + ch;
    float t = col[0];
#pragma unroll
    for (int s = 1; s < 32; ++s) t += col[s * 64];
    dst[((size_t)(split * NV + v) * a.N + n) * a.C + slab * 64 + ch] = t;
  }
}

// sum of the four waves' partial tiles in wave order
__device__ __forceinline__ float wave_tiles(const float* red, int row, int j) {
  const float* q = red + row * kMaxCr + j;
  return ((q[0] + q[kTile * kMaxCr]) + q[2 * kTile * kMaxCr]) + q[3 * kTile * kMaxCr];
}

// ------------------------------------------------------------------ excite (forward)
__global__ __launch_bounds__(256) void se_excite_kernel(SeArgs a, Plan p, const float* Spart) {
  __shared__ __attribute__((aligned(16))) float red[4 * kTile * kMaxCr];  // [wave][row][Cr]
  __shared__ __attribute__((aligned(16))) float hl[kTile * kMaxCr];       // [row][Cr]
  const int C = a.C, Cr = p.Cr, NT1 = Cr >> 4;
  const int tile = fast_div((int)blockIdx.x, p.dChunk), chunk = blockIdx.x - tile * p.nchunk;
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int row = tile * kTile + fr;
  const bool rowok = row < a.N;
  const size_t pstride = (size_t)a.N * C;

  // ---- GEMM1: this wave's k-steps over every column tile
  f32x4 acc[kMaxCr / 16];
#pragma unroll
  for (int nt = 0; nt < kMaxCr / 16; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ks = wid; ks < (C >> 5); ks += 4) {
    const int k0 = ks * 32 + fq * 8;
    bf16x8 fa = zero_frag();
    if (rowok) {
      const F8 sv = ld_parts(Spart, p.nsplit, pstride, (size_t)row * C + k0);
      if (p.nsplit > 1 && chunk == 0) stf8(a.S + (size_t)row * C + k0, sv);
      const F8 sc = ldf8(a.coef + kSc * C + k0), sh = ldf8(a.coef + kSh * C + k0);
      F8 m;
#pragma unroll
      for (int e = 0; e < 8; ++e) m.v[e] = __builtin_fmaf(sc.v[e], sv.v[e] * p.inv_hw, sh.v[e]);
      fa = to_frag(m);
    }
#pragma unroll
    for (int nt = 0; nt < kMaxCr / 16; ++nt)
      if (nt < NT1) {
        const bf16x8 fb = to_frag(ldf8(a.w1 + (size_t)(nt * 16 + fr) * C + k0));
        // operands swapped as in conv_igemm.hip: the lane owns row fr, columns 4 fq .. + 3
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, fa, acc[nt], 0, 0, 0);
      }
  }
#pragma unroll
  for (int nt = 0; nt < kMaxCr / 16; ++nt)
    if (nt < NT1)
      *reinterpret_cast<float4*>(red + (wid * kTile + fr) * kMaxCr + nt * 16 + 4 * fq) =
          make_float4(acc[nt][0], acc[nt][1], acc[nt][2], acc[nt][3]);
  __syncthreads();
  for (int i = threadIdx.x; i < kTile * Cr; i += 256) {
    const int r = fast_div(i, p.dCr), j = i - r * Cr;
    const float hv = fmaxf(wave_tiles(red, r, j) + a.b1[j], 0.f);
    hl[r * kMaxCr + j] = hv;
    if (chunk == 0 && tile * kTile + r < a.N) a.h[(size_t)(tile * kTile + r) * Cr + j] = hv;
  }
  __syncthreads();

  // ---- GEMM2: column tiles wid, wid + 4, .. of this chunk
  const int cbase = chunk * kChunk, ncols = min(kChunk, C - cbase);
  f32x4 acc2[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = fq * 8; k0 < ((Cr + 31) & ~31); k0 += 32) {
    const bool kok = k0 < Cr;  // Cr % 32 == 16: the last k-step's upper half is zero
    const bf16x8 fa = kok ? to_frag(ldf8(hl + fr * kMaxCr + k0)) : zero_frag();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int ct = wid + 4 * t;
      if (ct * 16 < ncols) {
        const bf16x8 fb =
            kok ? to_frag(ldf8(a.w2 + (size_t)(cbase + ct * 16 + fr) * Cr + k0)) : zero_frag();
        acc2[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, fa, acc2[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ct = wid + 4 * t;
    if (ct * 16 < ncols && rowok) {
      const int c = cbase + ct * 16 + 4 * fq;
      const float4 b = *reinterpret_cast<const float4*>(a.b2 + c);
      float4 o;
      o.x = 1.f / (1.f + expf(-(acc2[t][0] + b.x)));
      o.y = 1.f / (1.f + expf(-(acc2[t][1] + b.y)));
      o.z = 1.f / (1.f + expf(-(acc2[t][2] + b.z)));
      o.w = 1.f / (1.f + expf(-(acc2[t][3] + b.w)));
      *reinterpret_cast<float4*>(a.s + (size_t)row * C + c) = o;
    }
  }
}

// ------------------------------------------------------------------ excite (backward)
__global__ __launch_bounds__(256) void se_excite_bwd_kernel(SeArgs a, Plan p, const float* Gpart) {
  __shared__ __attribute__((aligned(16))) float red[4 * kTile * kMaxCr];
  __shared__ __attribute__((aligned(16))) float dhl[kTile * kMaxCr];
  const int C = a.C, Cr = p.Cr, NT1 = Cr >> 4;
  const int tile = blockIdx.x;
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int row = tile * kTile + fr;
  const bool rowok = row < a.N;
  const size_t NC = (size_t)a.N * C;

  // ---- dt2 (stored) and dh = dt2 . W2, k = the channel
  f32x4 acc[kMaxCr / 16];
#pragma unroll
  for (int nt = 0; nt < kMaxCr / 16; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ks = wid; ks < (C >> 5); ks += 4) {
    const int k0 = ks * 32 + fq * 8;
    bf16x8 fa = zero_frag();
    if (rowok) {
      const size_t off = (size_t)row * C + k0;
      const F8 g1 = ld_parts(Gpart, p.nsplit, 2 * NC, off);
      const F8 g2 = ld_parts(Gpart + NC, p.nsplit, 2 * NC, off);
      if (p.nsplit > 1) {
        stf8(a.G + off, g1);
        stf8(a.G + NC + off, g2);
      }
      const F8 sc = ldf8(a.coef + kSc * C + k0), sh = ldf8(a.coef + kSh * C + k0);
      const F8 sv = ldf8(a.s + off);
      F8 d;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float ds = __builtin_fmaf(sc.v[e], g2.v[e], sh.v[e] * g1.v[e]);
        d.v[e] = ds * (sv.v[e] * (1.f - sv.v[e]));
      }
      stf8(a.dt2 + off, d);
      fa = to_frag(d);
    }
#pragma unroll
    for (int nt = 0; nt < kMaxCr / 16; ++nt)
      if (nt < NT1) {
        const float* w = a.w2 + (size_t)k0 * Cr + nt * 16 + fr;  // W2[k0 + e][j]
        F8 f;
#pragma unroll
        for (int e = 0; e < 8; ++e) f.v[e] = w[(size_t)e * Cr];
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(to_frag(f), fa, acc[nt], 0, 0, 0);
      }
  }
#pragma unroll
  for (int nt = 0; nt < kMaxCr / 16; ++nt)
    if (nt < NT1)
      *reinterpret_cast<float4*>(red + (wid * kTile + fr) * kMaxCr + nt * 16 + 4 * fq) =
          make_float4(acc[nt][0], acc[nt][1], acc[nt][2], acc[nt][3]);
  __syncthreads();
  for (int i = threadIdx.x; i < kTile * Cr; i += 256) {
    const int r = fast_div(i, p.dCr), j = i - r * Cr;
    const int n = tile * kTile + r;
    float v = 0.f;
    if (n < a.N) {
      v = a.h[(size_t)n * Cr + j] > 0.f ? wave_tiles(red, r, j) : 0.f;
      a.dh[(size_t)n * Cr + j] = v;
    }
    dhl[r * kMaxCr + j] = v;
  }
  __syncthreads();

  // ---- dm = dh . W1, k = the reduced channel; column tiles wid, wid + 4, ..
  bf16x8 fa[kMaxCr / 32];
#pragma unroll
  for (int ks = 0; ks < kMaxCr / 32; ++ks) {
    const int k0 = ks * 32 + fq * 8;
    fa[ks] = k0 < Cr ? to_frag(ldf8(dhl + fr * kMaxCr + k0)) : zero_frag();
  }
  for (int ct = wid; ct < (C >> 4); ct += 4) {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < kMaxCr / 32; ++ks) {
      const int k0 = ks * 32 + fq * 8;
      if (ks * 32 < Cr) {
        F8 f;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          f.v[e] = k0 < Cr ? a.w1[(size_t)(k0 + e) * C + ct * 16 + fr] : 0.f;  // W1[k0 + e][c]
        o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(to_frag(f), fa[ks], o, 0, 0, 0);
      }
    }
    if (rowok)
      *reinterpret_cast<float4*>(a.dm + (size_t)row * C + ct * 16 + 4 * fq) =
          make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ------------------------------------------------------------------ parameter gradients
// blocks [0, nbw): 64 x 16 tiles of dW2; [nbw, 2 nbw): of dW1; then nbc blocks of 256 channels
// (db2, the BatchNorm sums, dgamma, dbeta, k1, k2); the last block: db1
__global__ __launch_bounds__(256) void se_param_bwd_kernel(SeArgs a, Plan p) {
  const int C = a.C, Cr = p.Cr, N = a.N;
  int b = blockIdx.x;
  if (b < 2 * p.nbw) {
    const bool first = b >= p.nbw;  // dW1
    if (first) b -= p.nbw;
    const int ct = fast_div(b, p.dRt), rt = b - ct * p.nrt;
    const int r = rt * 16 + (threadIdx.x & 15), c = ct * 64 + (threadIdx.x >> 4) * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (first) {
      const float4 sc = *reinterpret_cast<const float4*>(a.coef + kSc * C + c);
      const float4 sh = *reinterpret_cast<const float4*>(a.coef + kSh * C + c);
#pragma unroll 4
      for (int n = 0; n < N; ++n) {
        const float d = a.dh[(size_t)n * Cr + r];
        const float4 S = *reinterpret_cast<const float4*>(a.S + (size_t)n * C + c);
        acc[0] = __builtin_fmaf(d, __builtin_fmaf(sc.x, S.x * p.inv_hw, sh.x), acc[0]);
        acc[1] = __builtin_fmaf(d, __builtin_fmaf(sc.y, S.y * p.inv_hw, sh.y), acc[1]);
        acc[2] = __builtin_fmaf(d, __builtin_fmaf(sc.z, S.z * p.inv_hw, sh.z), acc[2]);
        acc[3] = __builtin_fmaf(d, __builtin_fmaf(sc.w, S.w * p.inv_hw, sh.w), acc[3]);
      }
      float4* dst = reinterpret_cast<float4*>(a.dw1 + (size_t)r * C + c);
      float4 o = *dst;
      o.x += acc[0]; o.y += acc[1]; o.z += acc[2]; o.w += acc[3];
      *dst = o;
    } else {
#pragma unroll 4
      for (int n = 0; n < N; ++n) {
        const float hv = a.h[(size_t)n * Cr + r];
        const float4 d = *reinterpret_cast<const float4*>(a.dt2 + (size_t)n * C + c);
        acc[0] = __builtin_fmaf(d.x, hv, acc[0]);
        acc[1] = __builtin_fmaf(d.y, hv, acc[1]);
        acc[2] = __builtin_fmaf(d.z, hv, acc[2]);
        acc[3] = __builtin_fmaf(d.w, hv, acc[3]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) a.dw2[(size_t)(c + i) * Cr + r] += acc[i];
    }
    return;
  }
  b -= 2 * p.nbw;
  if (b < p.nbc) {
    const int c = b * 256 + threadIdx.x;
    if (c >= C) return;
    const size_t NC = (size_t)N * C;
    float t1 = 0.f, t2 = 0.f, tb = 0.f;
#pragma unroll 2
    for (int n = 0; n < N; ++n) {
      const size_t o = (size_t)n * C + c;
      const float sv = a.s[o], dmv = a.dm[o];
      t1 += __builtin_fmaf(sv, a.G[o], dmv);
      t2 += __builtin_fmaf(sv, a.G[NC + o], dmv * (a.S[o] * p.inv_hw));
      tb += a.dt2[o];
    }
    const float sxh = a.coef[kIs * C + c] * __builtin_fmaf(-a.coef[kMu * C + c], t1, t2);
    a.coef[kK1 * C + c] = t1 * p.inv_m;
    a.coef[kK2 * C + c] = sxh * p.inv_m;
    a.dgamma[c] += sxh;
    a.dbeta[c] += t1;
    a.db2[c] += tb;
    return;
  }
  if ((int)threadIdx.x < Cr) {
    float t = 0.f;
    for (int n = 0; n < N; ++n) t += a.dh[(size_t)n * Cr + threadIdx.x];
    a.db1[threadIdx.x] += t;
  }
}

// ------------------------------------------------------------------ the two apply passes
// grid = N * bpi: a block owns 256 * kIpt items (one pixel x 8 channels each) of one image
template <bool BWD>
__global__ __launch_bounds__(256) void se_apply_kernel(SeArgs a, Plan p) {
  const int C = a.C;
  const int n = fast_div((int)blockIdx.x, p.dBpi);
  const int i0 = (blockIdx.x - n * p.bpi) * (256 * kIpt) + threadIdx.x;
  const int items = p.HW * p.G;
  const size_t img = (size_t)n * p.HW * C;
  const size_t mimg = (size_t)n * p.HW * p.G;
  const float* srow = a.s + (size_t)n * C;
  const float* dmrow = BWD ? a.dm + (size_t)n * C : nullptr;
  u16x8 zv[kIpt], rv[kIpt];
  unsigned mb[kIpt];
#pragma unroll
  for (int it = 0; it < kIpt; ++it) {
    const int i = i0 + it * 256;
    const int ii = i < items ? i : 0;
    zv[it] = ld8(a.z + img + (size_t)ii * 8);
    rv[it] = ld8((BWD ? a.dy : a.res) + img + (size_t)ii * 8);
    mb[it] = BWD ? a.mask[mimg + ii] : 0u;
  }
#pragma unroll
  for (int it = 0; it < kIpt; ++it) {
    const int i = i0 + it * 256;
    if (i >= items) break;
    const int c0 = (i - fast_div(i, p.dG) * p.G) * 8;
    const F8 sc = ldf8(a.coef + kSc * C + c0), sv = ldf8(srow + c0);
    u16x8 o;
    if (!BWD) {
      const F8 sh = ldf8(a.coef + kSh * C + c0);
      unsigned m = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float u = __builtin_fmaf(sc.v[e], bf2f(zv[it][e]), sh.v[e]);
        const float v = __builtin_fmaf(u, sv.v[e], bf2f(rv[it][e]));
        m |= (v > 0.f ? 1u : 0u) << e;
        o[e] = f2bf(fmaxf(v, 0.f));
      }
      st8(a.y + img + (size_t)i * 8, o);
      a.mask[mimg + i] = (unsigned char)m;
    } else {
      const F8 mu = ldf8(a.coef + kMu * C + c0), is = ldf8(a.coef + kIs * C + c0);
      const F8 k1 = ldf8(a.coef + kK1 * C + c0), k2 = ldf8(a.coef + kK2 * C + c0);
      const F8 dm = ldf8(dmrow + c0);
      u16x8 r;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool pos = (mb[it] >> e) & 1u;
        const float g = pos ? bf2f(rv[it][e]) : 0.f;
        r[e] = pos ? rv[it][e] : (unsigned short)0;
        const float du = __builtin_fmaf(g, sv.v[e], dm.v[e] * p.inv_hw);
        const float xh = (bf2f(zv[it][e]) - mu.v[e]) * is.v[e];
        o[e] = f2bf(sc.v[e] * __builtin_fmaf(-xh, k2.v[e], du - k1.v[e]));
      }
      st8(a.dz + img + (size_t)i * 8, o);
      if (a.dres) st8(a.dres + img + (size_t)i * 8, r);
    }
  }
}

// ------------------------------------------------------------------ host side
static bool served(int N, int P, int Q, int C, int reduction) {
  if (N < 1 || P < 1 || Q < 1 || C < 64 || C > 2048 || C % 64 || reduction < 1 || C % reduction)
    return false;
  const int Cr = C / reduction;
  if (Cr < 16 || Cr > kMaxCr || Cr % 16) return false;
  if ((long long)P * Q * C >= 0x80000000ll || (long long)N * C >= 0x80000000ll) return false;
  if ((long long)P * Q > 0x7fffffffll / 8) return false;
  return true;
}

static Plan plan(const SeArgs& a) {
  Plan p{};
  p.HW = a.P * a.Q;
  p.G = a.C / 8;
  p.Cr = a.C / a.reduction;
  p.nslab = a.C / 64;
  // pixel ranges only where whole images would leave most of the 256 CUs idle; a range is a
  // multiple of the 32 pixel slots and at least 64 pixels
  const long long base = (long long)a.N * p.nslab;
  int want = 1;
  if (base < 512 && p.HW >= 128)
    want = (int)std::min<long long>((1024 + base - 1) / base, p.HW / 64);
  p.pps = ((p.HW + want - 1) / want + 31) / 32 * 32;
  p.nsplit = (p.HW + p.pps - 1) / p.pps;
  p.nchunk = (a.C + kChunk - 1) / kChunk;
  p.bpi = (p.HW * p.G + 256 * kIpt - 1) / (256 * kIpt);
  p.nrt = p.Cr / 16;
  p.nbw = p.nslab * p.nrt;
  p.nbc = (a.C + 255) / 256;
  p.inv_hw = 1.f / (float)p.HW;
  p.inv_m = 1.f / ((float)a.N * a.P * a.Q);
  p.dG = make_fastdiv(p.G);
  p.dSlab = make_fastdiv(p.nslab);
  p.dSS = make_fastdiv(p.nslab * p.nsplit);
  p.dChunk = make_fastdiv(p.nchunk);
  p.dBpi = make_fastdiv(p.bpi);
  p.dCr = make_fastdiv(p.Cr);
  p.dRt = make_fastdiv(p.nrt);
  return p;
}

}  // namespace se
}  // namespace ddp_amd

using namespace ddp_amd;

extern "C" int ddp_se_ok(int N, int P, int Q, int C, int reduction) {
  return se::served(N, P, Q, C, reduction) ? 1 : 0;
}

extern "C" int ddp_se_fwd(const SeArgs* a, hipStream_t st) {
  if (!a || !se::served(a->N, a->P, a->Q, a->C, a->reduction)) return -1;
  if (!a->z || !a->res || !a->gamma || !a->beta || !a->coef || !a->w1 || !a->b1 || !a->w2 ||
      !a->b2 || !a->S || !a->s || !a->h || !a->y || !a->mask)
    return -1;
  if (a->use_running ? (!a->running_mean || !a->running_var) : !a->stats) return -1;
  const se::Plan p = se::plan(*a);
  if ((long long)a->N * p.bpi >= 0x80000000ll) return -1;
  float* Spart = a->S;
  if (p.nsplit > 1) {
    if (!a->ws || a->ws_elems < (size_t)p.nsplit * a->N * a->C) return -2;
    Spart = a->ws;
  }
  const int tiles = (a->N + se::kTile - 1) / se::kTile;
  hipLaunchKernelGGL(se::se_finalize_kernel, dim3((a->C + 255) / 256), dim3(256), 0, st, *a);
  hipLaunchKernelGGL(se::se_sum_kernel<false>, dim3(a->N * p.nslab * p.nsplit), dim3(256), 0, st,
                     *a, p, Spart);
  hipLaunchKernelGGL(se::se_excite_kernel, dim3(tiles * p.nchunk), dim3(256), 0, st, *a, p,
                     (const float*)Spart);
  hipLaunchKernelGGL(se::se_apply_kernel<false>, dim3(a->N * p.bpi), dim3(256), 0, st, *a, p);
  return (int)hipGetLastError();
}

extern "C" int ddp_se_bwd(const SeArgs* a, hipStream_t st) {
  if (!a || !se::served(a->N, a->P, a->Q, a->C, a->reduction)) return -1;
  if (!a->z || !a->dy || !a->mask || !a->coef || !a->w1 || !a->w2 || !a->S || !a->s || !a->h ||
      !a->G || !a->dt2 || !a->dh || !a->dm || !a->dw1 || !a->db1 || !a->dw2 || !a->db2 ||
      !a->dgamma || !a->dbeta || !a->dz || a->use_running)
    return -1;
  const se::Plan p = se::plan(*a);
  if ((long long)a->N * p.bpi >= 0x80000000ll) return -1;
  float* Gpart = a->G;
  if (p.nsplit > 1) {
    if (!a->ws || a->ws_elems < (size_t)p.nsplit * 2 * a->N * a->C) return -2;
    Gpart = a->ws;
  }
  const int tiles = (a->N + se::kTile - 1) / se::kTile;
  hipLaunchKernelGGL(se::se_sum_kernel<true>, dim3(a->N * p.nslab * p.nsplit), dim3(256), 0, st,
                     *a, p, Gpart);
  hipLaunchKernelGGL(se::se_excite_bwd_kernel, dim3(tiles), dim3(256), 0, st, *a, p,
                     (const float*)Gpart);
  hipLaunchKernelGGL(se::se_param_bwd_kernel, dim3(2 * p.nbw + p.nbc + 1), dim3(256), 0, st, *a, p);
  hipLaunchKernelGGL(se::se_apply_kernel<true>, dim3(a->N * p.bpi), dim3(256), 0, st, *a, p);
  return (int)hipGetLastError();
}
