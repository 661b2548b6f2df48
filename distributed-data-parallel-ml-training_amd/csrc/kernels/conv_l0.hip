// VGG input block for gfx950: conv 3x3 / s1 / p1 (3 image channels zero-padded to 8 -> 64) +
// training-mode BatchNorm + ReLU + 2x2/s2 max-pool, with the pre-BatchNorm activation z
// RECOMPUTED wherever it is needed instead of stored.
//
// Reference parity: the first block of part1/model.py:18-25 (Conv2d(3, 64, 3, padding=1) ->
// BatchNorm2d(64) -> ReLU -> MaxPool2d(2, 2)); SURVEY.md §2.D row 0.
//
// Why: the layer's convolution is 0.9 GFLOP at batch 256 (27 MACs per output), but its output z
// is the largest activation of the network (N x 32 x 32 x 64 bf16 = 33.5 MB at b256). The
// unfused chain streams it five times — conv store, BN+pool read, BN-backward reduce read, apply
// read — for ~66 us of a 0.85 ms step (profiles/r4f_vgg11_b256.md). Recomputing z from the
// 4.2 MB input costs a few microseconds of MFMA per pass, so here:
//   l0_stats_kernel  conv -> per-channel sum / sum of squares of the bf16-rounded z (no store)
//   l0_fwd_kernel    conv -> BN (coefficients folded from the statistics in every block; block 0
//                    writes the [6][64] table) -> ReLU -> 2x2 max-pool -> pooled y (8.4 MB) and,
//                    per pooled value, the window position its gradient goes to (1 B, 4.2 MB)
//   l0_sums_kernel   BN-backward sums S1 / S2 of the routed gradient from dy, code and the
//                    recorded winner z (no conv; or taken by the next block's dgrad finish)
//   l0_bwd_kernel<2> conv -> dz = scale * (dy_bn - k1 - xhat * k2) rounded to bf16 (k1 / k2
//                    folded from S1 / S2; block 0 adds dgamma / dbeta) -> weight gradient
//                    dW[k][tap][c] += sum over the tile's pixels of dz * x, MFMA into fp32
//                    accumulators that live across the wave's tiles -> one compact [64][28]
//                    fp32 partial per block. dz, the layer's last full-resolution tensor
//                    (33.5 MB at b256), is never stored: its only consumer was the weight
//                    gradient GEMM, which read it back and left 512 slabs to a finish launch
//   l0_wgrad_finish_kernel  fixed-order sum of the block partials, added into the gradient or
//                    (registered SGD step, api.h SgdFuse) applied to the master weights
//   l0_bwd_kernel<1> the dz pass that stores dz for the weight gradient GEMM (ops/layers.py
//                    L0_WGRAD_FUSE = False; the fused variant's reference), l0_bwd_kernel<0> the
//                    BN-backward sums through the recomputed z
// Every pass runs the same conv code on the same inputs, so z is bit-identical to the forward's;
// the arithmetic of each step is the one of conv_smallk.hip (conv) and bn_act.hip (finalize,
// apply, first-maximum pool rule).
//
// Tiling: a wave owns 16 output pixels = 2 image rows x 8 columns (four whole 2x2 pool windows)
// x 64 channels: the conv is conv_smallk.hip's direct MFMA (lane = one pixel x 4 channels per
// 16-channel tile, weights read from an LDS image staged once per block), and a pool window's
// four values sit in lanes {l, l^1, l^8, l^9} of the same 16-lane row — max and argmax are
// exchanged with DPP (quad_perm, row_ror:8), no LDS.
// Measured (profiles/r4k_vgg11_b256_l0v5.md): 12.0 + 19.1 us forward, 15.3 + 17.3 us backward
// at b256 against ~66 us of conv + BN passes unfused; step 0.835-0.846 vs 0.855 ms same box.
//
// Fused weight gradient (l0_bwd_kernel<2>): the conv contracts over (tap, channel) with lane =
// pixel, the weight gradient contracts over the tile's 16 pixels, so both operands are
// transposed through a per-wave LDS stage: the bf16 dz tile [16 px][64 ch] is written as the
// lanes hold it and read back with ds_read_b64_tr_b16 as the A operand (row = channel, k =
// pixel) of v_mfma_f32_16x16x16_bf16; the tile's 4 x 10 input halo patch (4 of the 8 padded
// channels) is written from the conv's own fragments and read per lane as the B operand
// (k = pixel, column = tap * 3 + c: 27 real columns in two 16-column tiles, the five spare
// columns read the zero pad channel 3). 4 x 2 MFMAs per tile, 32 accumulator registers.
// Measured (profiles/l0_wgrad_fused.md): 16.5 us + 6.2 us finish at b256 against 18.2 us dz
// pass + 14.6 us WGRAD GEMM + 5.5 us finish; step 0.7017 vs 0.7389 ms, every trial of the A/B.
#include "common.h"
#include "api.h"

#include <algorithm>

namespace ddp_amd {
namespace l0 {

constexpr int kK = 64;    // output channels
constexpr int kNT = 4;    // 16-channel MFMA column tiles
constexpr int kNKS = 3;   // k-steps of 4 taps (9 taps padded to 12)

struct Args {
  const unsigned short* x;   // [N][H][W][8] bf16 (channels 3..7 zero)
  const unsigned short* wc;  // [64][3][3][8] bf16
  const float* bias;         // [64] or null
  int N, H, W, tiles;        // tiles = N * (H / 2) * (W / 8)
  float eps;
  int relu;
  float* stats;              // [kStatRep][2][64] forward sums (zeroed per step)
  const float* gamma;
  const float* beta;
  float* coef;               // [6][64]: scale, shift, mean, invstd, k1, k2
  unsigned short* y;         // [N][H/2][W/2][64] pooled output
  const unsigned short* dy;  // [N][H/2][W/2][64] gradient at the pooled output
  float* sums;               // [kStatRep][2][64] BN-backward sums (zeroed per step)
  unsigned short* dz;        // [N][H][W][64] gradient at z
  unsigned* code;            // per pool window and channel: the position (0..3) that takes the
                             // gradient, 4 = none (ReLU cut), 0xFF = NaN window; lane-major
                             // [window][g][j][v] bytes, written by the forward, read by both
                             // backward passes
  unsigned short* zw;        // [N][H/2][W/2][64] bf16: z of the pixel code points to (forward;
                             // the backward sums need nothing else of the window)
  float* dgamma;             // accumulated (arena)
  float* dbeta;
  float* wg;                 // fused weight gradient: [blocks][64][kWgN] fp32 partials
};

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 as_bf(const uint4& v) { return __builtin_bit_cast(bf16x8, v); }

// lane l of each 16-lane row <- lane l ^ 1 / l ^ 8
__device__ __forceinline__ float xor1(float v) { return dpp_f<0xB1>(v); }
__device__ __forceinline__ float xor8(float v) { return dpp_f<0x128>(v); }  // row_ror:8

struct Tile {
  int n, h, w;  // this lane's pixel
  int hp, wo;   // its pool window (pooled row / column)
  int d;        // its position in the window (bn_act.hip order: 0 (0,0), 1 (0,1), 2 (1,0), 3 (1,1))
};

__device__ __forceinline__ Tile tile_pixel(const Args& a, int t, int rl) {
  const int wb = a.W / 8, per_img = (a.H / 2) * wb;
  Tile p;
  p.n = t / per_img;
  const int rem = t - p.n * per_img;
  p.hp = rem / wb;
  const int cb = rem - p.hp * wb;
  const int r = rl >> 3, c = rl & 7;
  p.h = 2 * p.hp + r;
  p.w = 8 * cb + c;
  p.wo = 4 * cb + (c >> 1);
  p.d = 2 * r + (c & 1);
  return p;
}

// LDS weight image [64 rows][13 taps][8 ch] (12 used taps + 1 pad tap per row spreads the 16
// rows a ds_read_b128 lane group reads over the banks, conv_smallk.hip's stem layout), staged
// once per block: the per-wave register copy of round-4's first version cost 48 VGPRs and
// capped the kernel at 2 waves per SIMD
constexpr int kRow = 13;
struct Smem {
  uint4 w[kK * kRow];
  float cf[7][kK];  // 0 scale, 1 shift, 2 mean, 3 inv-std, 4 / 5 backward sums, 6 bias
  float red[4][2][kK];
};

__device__ __forceinline__ void stage_weights(const Args& a, Smem& sm) {
  for (int i = threadIdx.x; i < kK * 12; i += 256) {
    const int k = i / 12, tap = i - k * 12;
    sm.w[k * kRow + tap] = tap < 9 ? *reinterpret_cast<const uint4*>(a.wc + ((size_t)k * 9 + tap) * 8)
                                   : make_uint4(0, 0, 0, 0);
  }
}

// activation fragments of one tile: lane l loads tap 4t + (l >> 4) of its pixel (16 B)
__device__ __forceinline__ void load_x(const Args& a, const Tile& p, int g, uint4 (&xf)[kNKS]) {
#pragma unroll
  for (int t = 0; t < kNKS; ++t) {
    const int tap = 4 * t + g;
    const int r = tap / 3, s = tap - r * 3;
    const int h = p.h + r - 1, w = p.w + s - 1;
    xf[t] = (tap < 9 && (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W)
                ? *reinterpret_cast<const uint4*>(a.x + (((size_t)p.n * a.H + h) * a.W + w) * 8)
                : make_uint4(0, 0, 0, 0);
  }
}

// z of this lane's pixel for channels j*16 + 4g + v (bf16-rounded, + bias): conv_smallk.hip math
__device__ __forceinline__ void conv_z(const Smem& sm, const uint4 (&xf)[kNKS], int g, int rl,
                                       float (&z)[kNT][4]) {
  f32x4 acc[kNT];
#pragma unroll
  for (int j = 0; j < kNT; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < kNKS; ++t)
#pragma unroll
    for (int j = 0; j < kNT; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(sm.w[(j * 16 + rl) * kRow + 4 * t + g]),
                                                      as_bf(xf[t]), acc[j], 0, 0, 0);
#pragma unroll
  for (int j = 0; j < kNT; ++j)
#pragma unroll
    for (int v = 0; v < 4; ++v) z[j][v] = bf2f(f2bf(acc[j][v] + sm.cf[6][j * 16 + 4 * g + v]));
}

__device__ __forceinline__ void stage_bias(const Args& a, Smem& sm) {
  if (threadIdx.x < kK) sm.cf[6][threadIdx.x] = a.bias ? a.bias[threadIdx.x] : 0.f;
}

__device__ __forceinline__ int xor1i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false); }
__device__ __forceinline__ int xor8i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false); }

// max over the pool window (lanes l, l^1, l^8, l^9), NaN-propagating like bn_act.hip's pool
__device__ __forceinline__ float window_max(float v) {
  v = __builtin_elementwise_maximum(v, xor1(v));
  return __builtin_elementwise_maximum(v, xor8(v));
}

// block reduction of per-lane channel sums (lane: channels j*16 + 4g + v) -> one atomic per
// channel per block into replica blockIdx.x % kStatRep (conv_smallk.hip scheme)
__device__ __forceinline__ void block_sums(float (&s1)[kNT][4], float (&s2)[kNT][4], float* rep,
                                           int rl, int g, Smem& sm) {
#pragma unroll
  for (int j = 0; j < kNT; ++j)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      s1[j][v] = dpp_sum16(s1[j][v]);
      s2[j][v] = dpp_sum16(s2[j][v]);
    }
  const int wib = threadIdx.x >> 6;
  if (rl == 0) {
#pragma unroll
    for (int j = 0; j < kNT; ++j)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        sm.red[wib][0][j * 16 + 4 * g + v] = s1[j][v];
        sm.red[wib][1][j * 16 + 4 * g + v] = s2[j][v];
      }
  }
  __syncthreads();
  if (threadIdx.x < 2 * kK) {
    const int k = threadIdx.x / kK, c = threadIdx.x - k * kK;
    atomicAdd(rep + k * kK + c,
              stat_val(sm.red[0][k][c] + sm.red[1][k][c] + sm.red[2][k][c] + sm.red[3][k][c],
                       blockIdx.x));
  }
}

// one tile's global operands: the input fragments and (backward) the pooled gradient of the
// lane's window (the four lanes of a window load the same 8 B)
struct Ops {
  uint4 x[kNKS];
  u16x4 dy[kNT];
  uint4 code;
};

__device__ __forceinline__ size_t window_of(const Args& a, const Tile& p) {
  return ((size_t)p.n * (a.H / 2) + p.hp) * (a.W / 2) + p.wo;
}

template <bool DY>
__device__ __forceinline__ void load_ops(const Args& a, const Tile& p, int g, Ops& o) {
  load_x(a, p, g, o.x);
  if (DY) {
    const size_t win = window_of(a, p);
    const unsigned short* src = a.dy + win * kK + 4 * g;
#pragma unroll
    for (int j = 0; j < kNT; ++j) o.dy[j] = *reinterpret_cast<const u16x4*>(src + j * 16);
    o.code = *reinterpret_cast<const uint4*>(a.code + win * (kK / 4) + g * 4);
  }
}

// Work split: a block = 4 waves, a wave walks tiles wave, wave + nw, ... (at most 1024 blocks:
// every block ends with one atomic per channel into a statistics replica). Latency is hidden by
// occupancy (waves per SIMD): prefetching the next tile's operands into registers measured
// slower (r4i: bwd 31 vs 28 us at b256, 176 VGPRs -> 2 waves per SIMD).
template <bool DY, class Setup, class Body>
__device__ __forceinline__ void tile_loop(const Args& a, int g, int rl, Setup setup, Body body) {
  const int nw = gridDim.x * 4;
  setup();
  __syncthreads();
  for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < a.tiles; t += nw) {
    // keeps the LDS weight reads inside the loop (hoisted, they are 48 VGPRs)
    asm volatile("" ::: "memory");
    const Tile cur = tile_pixel(a, t, rl);
    Ops op;
    load_ops<DY>(a, cur, g, op);
    body(cur, op);
  }
}

// forward statistics of z (no store)
__global__ __launch_bounds__(256) void l0_stats_kernel(Args a) {
  __shared__ Smem sm;
  const int lane = threadIdx.x & 63, g = lane >> 4, rl = lane & 15;
  float s1[kNT][4] = {}, s2[kNT][4] = {};
  tile_loop<false>(
      a, g, rl,
      [&] {
        stage_weights(a, sm);
        stage_bias(a, sm);
      },
      [&](const Tile&, const Ops& op) {
        float z[kNT][4];
        conv_z(sm, op.x, g, rl, z);
#pragma unroll
        for (int j = 0; j < kNT; ++j)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            s1[j][v] += z[j][v];
            s2[j][v] += z[j][v] * z[j][v];
          }
      });
  block_sums(s1, s2, a.stats + stat_rep(blockIdx.x) * 2 * kK, rl, g, sm);
}

__global__ __launch_bounds__(256) void l0_fwd_kernel(Args a) {
  __shared__ Smem sm;
  const int lane = threadIdx.x & 63, g = lane >> 4, rl = lane & 15;
  const int Ho = a.H / 2, Wo = a.W / 2;
  tile_loop<false>(
      a, g, rl,
      [&] {
        stage_weights(a, sm);
        stage_bias(a, sm);
        if (threadIdx.x < kK) {  // (scale, shift) from the statistics replicas (bn_act.hip finalize)
          const int c = threadIdx.x;
          const float M = (float)a.N * a.H * a.W;
          float s1 = 0.f, s2 = 0.f;
#pragma unroll
          for (int r = 0; r < kStatRep; ++r) {
            s1 += a.stats[r * 2 * kK + c];
            s2 += a.stats[r * 2 * kK + kK + c];
          }
          const float mu = s1 / M;
          const float var = fmaxf(s2 / M - mu * mu, 0.f);
          const float is = rsqrtf(var + a.eps);
          const float sc = a.gamma[c] * is, sh = a.beta[c] - mu * sc;
          sm.cf[0][c] = sc;
          sm.cf[1][c] = sh;
          if (blockIdx.x == 0) {  // the table the backward reads
            a.coef[0 * kK + c] = sc;
            a.coef[1 * kK + c] = sh;
            a.coef[2 * kK + c] = mu;
            a.coef[3 * kK + c] = is;
          }
        }
      },
      [&](const Tile& cur, const Ops& op) {
        float z[kNT][4];
        conv_z(sm, op.x, g, rl, z);
        const int bit = 1 << cur.d, upto = (2 << cur.d) - 1;
        u16x4 o[kNT], ow[kNT];
        unsigned cw[kNT];
#pragma unroll
        for (int j = 0; j < kNT; ++j) {
          cw[j] = 0;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int c = j * 16 + 4 * g + v;
            float y = z[j][v] * sm.cf[0][c] + sm.cf[1][c];  // (bn_act.hip apply expression)
            if (a.relu) y = fmaxf(y, 0.f);
            const float m = window_max(y);
            o[j][v] = f2bf(m);
            // the gradient's destination: the window's first maximum (bn_act.hip's tie rule:
            // every lane sets bit d when it holds the max, the lowest bit of the OR wins),
            // none when ReLU zeroed the whole window (its winner had y <= 0)
            int b = y == m ? bit : 0;
            b |= xor1i(b);
            b |= xor8i(b);
            const unsigned cd = b == 0 ? 0xFFu : (a.relu && !(m > 0.f)) ? 4u : (unsigned)__builtin_ctz(b);
            cw[j] |= cd << (8 * v);
            // the winner's z to every lane of the window (the others add exact zeros)
            float zs = (b & upto) == bit ? z[j][v] : 0.f;
            zs += xor1(zs);
            zs += xor8(zs);
            ow[j][v] = f2bf(zs);  // (exact: z is bf16-valued)
          }
        }
        if (cur.d == 0) {
          const size_t win = window_of(a, cur);
          unsigned short* dst = a.y + win * kK + 4 * g;
#pragma unroll
          for (int j = 0; j < kNT; ++j) *reinterpret_cast<u16x4*>(dst + j * 16) = o[j];
          unsigned short* dzw = a.zw + win * kK + 4 * g;
#pragma unroll
          for (int j = 0; j < kNT; ++j) *reinterpret_cast<u16x4*>(dzw + j * 16) = ow[j];
          *reinterpret_cast<uint4*>(a.code + win * (kK / 4) + g * 4) =
              make_uint4(cw[0], cw[1], cw[2], cw[3]);
        }
      });
}

// BatchNorm-backward sums S1 = sum dy_bn, S2 = sum dy_bn * xhat without the conv: dy_bn is the
// pooled gradient at the pixel the forward's code names (zero elsewhere), and that pixel's z is
// the recorded zw, so each pooled value contributes dy * [pass] and dy * (zw - mean) * invstd
// once. A thread owns one window x the 16 channels j*16 + 4g + v of its lane group g (the code
// bytes' order), walking windows with a grid stride; block reduction through LDS, one atomic
// per channel per block into replica blockIdx.x % kStatRep.
__global__ __launch_bounds__(256) void l0_sums_kernel(Args a, int windows) {
  __shared__ float red[256][33];
  const int tid = threadIdx.x, g = tid & 3;
  float mu[kNT][4], is[kNT][4], s1[kNT][4] = {}, s2[kNT][4] = {};
#pragma unroll
  for (int j = 0; j < kNT; ++j)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int c = j * 16 + 4 * g + v;
      mu[j][v] = a.coef[2 * kK + c];
      is[j][v] = a.coef[3 * kK + c];
    }
  for (int w = blockIdx.x * 64 + (tid >> 2); w < windows; w += gridDim.x * 64) {
    const uint4 cq = *reinterpret_cast<const uint4*>(a.code + (size_t)w * (kK / 4) + g * 4);
    const unsigned cw[kNT] = {cq.x, cq.y, cq.z, cq.w};
    u16x4 dv[kNT], zv[kNT];
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      dv[j] = *reinterpret_cast<const u16x4*>(a.dy + (size_t)w * kK + j * 16 + 4 * g);
      zv[j] = *reinterpret_cast<const u16x4*>(a.zw + (size_t)w * kK + j * 16 + 4 * g);
    }
#pragma unroll
    for (int j = 0; j < kNT; ++j)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float d = ((cw[j] >> (8 * v)) & 0xFFu) < 4u ? bf2f(dv[j][v]) : 0.f;
        s1[j][v] += d;
        s2[j][v] += d * ((bf2f(zv[j][v]) - mu[j][v]) * is[j][v]);
      }
  }
#pragma unroll
  for (int j = 0; j < kNT; ++j)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      red[tid][j * 4 + v] = s1[j][v];
      red[tid][16 + j * 4 + v] = s2[j][v];
    }
  __syncthreads();
  if (tid < 2 * kK) {
    const int k = tid / kK, c = tid - k * kK;
    const int gg = (c & 15) >> 2, e = k * 16 + (c >> 4) * 4 + (c & 3);
    float t = 0.f;
    for (int i = 0; i < 64; ++i) t += red[4 * i + gg][e];
    atomicAdd(a.sums + stat_rep(blockIdx.x) * 2 * kK + k * kK + c, stat_val(t, blockIdx.x));
  }
}

// ---- weight gradient fused into the dz pass (APPLY = 2)
typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;
constexpr int kWgN = 28;            // partial's columns: n = tap * 3 + c < 27, + 1 (16-B rows)
constexpr int kWgSlab = kK * kWgN;  // fp32 per block partial (7 KB)
// dz tile row: 64 channels + 4 pad = 34 dwords, so the 16 lanes of a ds_write_b64 group (one
// pixel row each) land on 16 distinct bank pairs
constexpr int kDzRow = 68;
struct alignas(16) WgStage {        // per wave
  unsigned short dz[16][kDzRow];    // this tile's bf16 dz [pixel][channel]
  unsigned short xp[4 * 10][4];     // its input halo patch [row][column][channels 0..3]
};
template <bool ON> struct WgLds { WgStage w[4]; };
template <> struct WgLds<false> {};

// BN backward through the recomputed z. APPLY = 0: S1 / S2 sums; 1: dz (+ dgamma / dbeta);
// 2: dz kept on chip and contracted with the input patch into the weight gradient partial
template <int APPLY>
__device__ __forceinline__ void l0_bwd_body(const Args& a) {
  constexpr bool WG = APPLY == 2;
  __shared__ Smem sm;
  __shared__ WgLds<WG> wl;
  const int lane = threadIdx.x & 63, g = lane >> 4, rl = lane & 15, wib = threadIdx.x >> 6;
  float s1[kNT][4] = {}, s2[kNT][4] = {};
  // WG: dW[channel jt*16 + 4g + v][column nt*16 + rl] of this wave's tiles
  f32x4 dwacc[kNT][2];
  // ... and this lane's B-operand source in the patch: column n = nt*16 + rl = tap * 3 + c at
  // the tile pixels 4g .. 4g+3 (tile row g >> 1, columns 4 (g & 1) + j; + 4 u16 per pixel);
  // n >= 27 reads the zero pad channel 3
  int xoff[2] = {0, 0};
  if (WG) {
#pragma unroll
    for (int jt = 0; jt < kNT; ++jt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) dwacc[jt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int n = nt * 16 + rl;
      const int tap = n < 27 ? n / 3 : 0, c = n < 27 ? n - tap * 3 : 3;
      const int tr = tap / 3, ts = tap - tr * 3;
      xoff[nt] = (((g >> 1) + tr) * 10 + 4 * (g & 1) + ts) * 4 + c;
    }
  }
  tile_loop<true>(
      a, g, rl,
      [&] {
        stage_weights(a, sm);
        stage_bias(a, sm);
        if (threadIdx.x < kK) {
          const int c = threadIdx.x;
          // LDS rows: 0 scale, 2 invstd, 3 -mean * invstd (xhat = z * [2] + [3]); APPLY:
          // 4 / 5 with dz = scale * dy_bn + z * [4] + [5], the bn_act.hip apply expression
          // scale * (dy_bn - k1 - xhat * k2) expanded in z
          const float sc = a.coef[c], mu = a.coef[2 * kK + c], is = a.coef[3 * kK + c];
          sm.cf[0][c] = sc;
          sm.cf[2][c] = is;
          sm.cf[3][c] = -mu * is;
          if (APPLY) {  // finalize of the backward sums (bn_act.hip bn_finalize_bwd_kernel)
            const float inv_m = 1.f / ((float)a.N * a.H * a.W);
            float t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int r = 0; r < kStatRep; ++r) {
              t1 += a.sums[r * 2 * kK + c];
              t2 += a.sums[r * 2 * kK + kK + c];
            }
            const float k1 = t1 * inv_m, k2 = t2 * inv_m;
            sm.cf[4][c] = -sc * k2 * is;
            sm.cf[5][c] = sc * (k2 * is * mu - k1);
            if (blockIdx.x == 0) {
              a.coef[4 * kK + c] = k1;
              a.coef[5 * kK + c] = k2;
              if (a.dgamma) a.dgamma[c] += t2;  // one writer per channel
              if (a.dbeta) a.dbeta[c] += t1;
            }
          }
        }
      },
      [&](const Tile& cur, const Ops& op) {
        if constexpr (WG) {
          // the halo patch from the conv's fragments: tap (tr, ts) of pixel (r, c) is patch
          // position (r + tr, c + ts); positions shared by several lanes get the same value
          WgStage& st = wl.w[wib];
#pragma unroll
          for (int t = 0; t < kNKS; ++t) {
            const int tap = 4 * t + g;
            const int tr = tap / 3, ts = tap - tr * 3;
            if (tap < 9)
              *reinterpret_cast<uint2*>(st.xp[((rl >> 3) + tr) * 10 + (rl & 7) + ts]) =
                  make_uint2(op.x[t].x, op.x[t].y);
          }
        }
        float z[kNT][4];
        conv_z(sm, op.x, g, rl, z);
        const unsigned cw[kNT] = {op.code.x, op.code.y, op.code.z, op.code.w};
        u16x4 o[kNT];
#pragma unroll
        for (int j = 0; j < kNT; ++j)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int c = j * 16 + 4 * g + v;
            const float zf = z[j][v];
            // the forward's verdict: this lane's pixel takes the pooled gradient
            const float dyb = ((cw[j] >> (8 * v)) & 0xFFu) == (unsigned)cur.d ? bf2f(op.dy[j][v]) : 0.f;
            if (APPLY) {
              o[j][v] = f2bf(sm.cf[0][c] * dyb + (zf * sm.cf[4][c] + sm.cf[5][c]));
            } else {
              s1[j][v] += dyb;
              s2[j][v] += dyb * (zf * sm.cf[2][c] + sm.cf[3][c]);
            }
          }
        if constexpr (WG) {
          // dW += dz^T x over the tile's 16 pixels. LDS accesses of one wave complete in
          // program order, so the wave's own stage needs no barrier, only the compiler's order
          WgStage& st = wl.w[wib];
#pragma unroll
          for (int j = 0; j < kNT; ++j)
            *reinterpret_cast<u16x4*>(&st.dz[rl][j * 16 + 4 * g]) = o[j];
          asm volatile("" ::: "memory");
          const unsigned short* xp = &st.xp[0][0];
          v4i16 fb[2];
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[nt][j] = (short)xp[xoff[nt] + 4 * j];
          // A operand: lane group g reads pixels 4g .. 4g+3 x channels jt*16 .. +15 transposed
          // (lane 4q + p supplies row q, columns 4p .. 4p+3; lane i receives column i)
          const unsigned short* arow = &st.dz[4 * g + (rl >> 2)][4 * (rl & 3)];
#pragma unroll
          for (int jt = 0; jt < kNT; ++jt) {
            const v4i16 fa = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(arow + jt * 16));
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
              dwacc[jt][nt] =
                  __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fa, fb[nt], dwacc[jt][nt], 0, 0, 0);
          }
        } else if (APPLY) {
          unsigned short* dst = a.dz + (((size_t)cur.n * a.H + cur.h) * a.W + cur.w) * kK + 4 * g;
#pragma unroll
          for (int j = 0; j < kNT; ++j) *reinterpret_cast<u16x4*>(dst + j * 16) = o[j];
        }
      });
  if (!APPLY) block_sums(s1, s2, a.sums + stat_rep(blockIdx.x) * 2 * kK, rl, g, sm);
  if constexpr (WG) {
    // the block's partial: waves summed in the fixed order ((w0 + w1) + w2) + w3 through LDS
    // (the weight image's space, free after the tile loop), stored by wave 3 as [64][kWgN]
    float* red = reinterpret_cast<float*>(sm.w);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (wib == w) {
#pragma unroll
        for (int jt = 0; jt < kNT; ++jt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const int e = (jt * 2 + nt) * 4 + v;
              float t = dwacc[jt][nt][v];
              if (w > 0) t += red[e * 64 + lane];
              if (w < 3) {
                red[e * 64 + lane] = t;
              } else if (nt * 16 + rl < kWgN) {
                a.wg[(size_t)blockIdx.x * kWgSlab + (jt * 16 + 4 * g + v) * kWgN + nt * 16 + rl] = t;
              }
            }
      }
      if (w < 3) __syncthreads();
    }
  }
}

template <int APPLY>
__global__ __launch_bounds__(256) void l0_bwd_kernel(Args a) {
  l0_bwd_body<APPLY>(a);
}
// the fused variant's 32 accumulators must not cost the pass its 4 waves per SIMD
template <>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void l0_bwd_kernel<2>(
    Args a) {
  l0_bwd_body<2>(a);
}

// Sum of the fused weight gradient's block partials in fixed order (no atomics: reproducible
// by construction). A block owns 4 float4 of the [64][kWgN] partial; its 64 slab lanes each
// sum slabs s, s + 64, ... with kWgBatch loads in flight, then a fixed tree over the lanes.
// The total is added into the gradient ([K][R][S][3] with wkrsc, else [K][3][R][S])
// or, with ``sg.p`` (api.h SgdFuse: the layer has no DGRAD, so its weights are read by nothing
// after this), applied as the optimizer step: master and momentum [K][R][S][3], the bf16
// operand copy [K][R][S][8] with its pad channels untouched.
constexpr int kWgBatch = 8;
__global__ __launch_bounds__(256) void l0_wgrad_finish_kernel(const float* __restrict__ ws,
                                                              int nslab, float* __restrict__ dw,
                                                              int wkrsc, SgdFuse sg) {
  __shared__ float4 red[64][4];
  const bool opt = sg.p != nullptr;
  const float lr = opt ? sched_lr_block(sg.sched, sg.lr) : sg.lr;
  const int e = threadIdx.x & 3, s0 = threadIdx.x >> 2;
  const int i4 = blockIdx.x * 4 + e;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int z = s0; z < nslab; z += 64 * kWgBatch) {
    float4 t[kWgBatch];
#pragma unroll
    for (int u = 0; u < kWgBatch; ++u)
      if (z + 64 * u < nslab)
        t[u] = reinterpret_cast<const float4*>(ws + (size_t)(z + 64 * u) * kWgSlab)[i4];
#pragma unroll
    for (int u = 0; u < kWgBatch; ++u)
      if (z + 64 * u < nslab) { v.x += t[u].x; v.y += t[u].y; v.z += t[u].z; v.w += t[u].w; }
  }
  red[s0][e] = v;
  for (int h = 32; h >= 1; h >>= 1) {
    __syncthreads();
    if (s0 < h) {
      const float4 o = red[s0 + h][e];
      v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      red[s0][e] = v;
    }
  }
  if (s0 != 0) return;
  const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int idx = i4 * 4 + t, k = idx / kWgN, n = idx - k * kWgN;
    if (n >= 27) continue;
    const int tap = n / 3, c = n - tap * 3;
    if (opt) {
      const int mi = k * 27 + n;
      float b = sg.buf[mi];
      const float np = sgd_update1(sg.p[mi], vv[t], b, lr, sg.momentum, sg.wd, sg.grad_scale,
                                   sg.nesterov);
      sg.p[mi] = np;
      sg.buf[mi] = b;
      sg.wc[(k * 9 + tap) * 8 + c] = f2bf(np);
    } else {
      dw[wkrsc ? k * 27 + n : (k * 3 + c) * 9 + tap] += vv[t];
    }
  }
}

// one tile per wave where the grid allows, at most 1024 blocks (4 per CU): every block adds one
// partial sum per channel into a statistics replica, and memory-side atomics serialise per
// address (measured r4j, b256: 1024 blocks 15.3 / 17.3 us backward passes, 4096 blocks 35.6 /
// 26.5 us; 512 / 2048 blocks equal to 1024 within the run-to-run spread)
static unsigned grid_for(int tiles) {
  return (unsigned)std::max(1, std::min(1024, (tiles + 3) / 4));
}

}  // namespace l0
}  // namespace ddp_amd

using namespace ddp_amd;

static bool l0_shape_ok(const ConvGeom* g) {
  return g->C == 8 && g->Creal <= 8 && g->K == l0::kK && g->R == 3 && g->S == 3 &&
         g->stride == 1 && g->pad == 1 && g->P == g->H && g->Q == g->W && g->H % 2 == 0 &&
         g->W % 8 == 0 && (size_t)g->N * g->H * g->W * l0::kK < (1ull << 31);
}

extern "C" int ddp_l0_ok(const ConvGeom* g) { return l0_shape_ok(g) ? 1 : 0; }

static l0::Args l0_args(const ConvGeom* g, const L0Io* io) {
  l0::Args a{};
  a.x = (const unsigned short*)io->x;
  a.wc = (const unsigned short*)io->wc;
  a.bias = io->bias;
  a.N = g->N; a.H = g->H; a.W = g->W;
  a.tiles = g->N * (g->H / 2) * (g->W / 8);
  a.eps = io->eps;
  a.relu = io->relu;
  a.stats = io->stats;
  a.gamma = io->gamma;
  a.beta = io->beta;
  a.coef = io->coef;
  a.y = (unsigned short*)io->y;
  a.dy = (const unsigned short*)io->dy;
  a.sums = io->sums;
  a.dz = (unsigned short*)io->dz;
  a.code = (unsigned*)io->code;
  a.zw = (unsigned short*)io->zw;
  a.dgamma = io->dgamma;
  a.dbeta = io->dbeta;
  return a;
}

// forward: statistics pass + BN / ReLU / pool pass (stats zeroed by the caller); -1 = shape not
// served
extern "C" int ddp_l0_fwd(const ConvGeom* g, const L0Io* io, hipStream_t st) {
  if (!l0_shape_ok(g) || !io->x || !io->wc || !io->stats || !io->gamma || !io->beta ||
      !io->coef || !io->y || !io->code || !io->zw)
    return -1;
  const l0::Args a = l0_args(g, io);
  const unsigned nb = l0::grid_for(a.tiles);
  hipLaunchKernelGGL(l0::l0_stats_kernel, dim3(nb), dim3(256), 0, st, a);
  hipLaunchKernelGGL(l0::l0_fwd_kernel, dim3(nb), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

// backward: sums pass + dz pass (sums zeroed by the caller; coef = the forward's table). With
// ``dz`` the dz pass stores dz for the caller's weight gradient GEMM; with ``dw`` and no ``dz``
// it builds the weight gradient itself (+ the partials' finish, which takes a registered SGD
// step: the layer has no DGRAD). -2 = the fused form does not serve this call (3 real input
// channels only; workspace too small): nothing was launched, the caller takes the dz form.
extern "C" int ddp_l0_bwd(const ConvGeom* g, const L0Io* io, hipStream_t st) {
  const bool fused = !io->dz && io->dw;
  if (!l0_shape_ok(g) || !io->x || !io->wc || !io->coef || !io->dy || !io->sums ||
      (!io->dz && !io->dw) || !io->code || !io->zw)
    return -1;
  l0::Args a = l0_args(g, io);
  const unsigned nb = l0::grid_for(a.tiles);
  if (fused && (g->Creal != 3 || !io->ws || io->ws_elems < (size_t)nb * l0::kWgSlab)) return -2;
  const int windows = g->N * (g->H / 2) * (g->W / 2);
  const unsigned ns = (unsigned)std::max(1, std::min(512, (windows + 127) / 128));
  if (!io->sums_ready)  // (else taken by the next block's dgrad finish, BnBwdFuse::code)
    hipLaunchKernelGGL(l0::l0_sums_kernel, dim3(ns), dim3(256), 0, st, a, windows);
  if (!fused) {
    hipLaunchKernelGGL(l0::l0_bwd_kernel<1>, dim3(nb), dim3(256), 0, st, a);
    return (int)hipGetLastError();
  }
  a.wg = io->ws;
  hipLaunchKernelGGL(l0::l0_bwd_kernel<2>, dim3(nb), dim3(256), 0, st, a);
  SgdFuse sg{};
  if (g->wkrsc) ddp_sgd_fuse_take_final(io->dw, &sg);  // (master and gradient share the layout)
  hipLaunchKernelGGL(l0::l0_wgrad_finish_kernel, dim3(l0::kWgSlab / 16), dim3(256), 0, st,
                     (const float*)io->ws, (int)nb, io->dw, g->wkrsc, sg);
  return (int)hipGetLastError();
}
