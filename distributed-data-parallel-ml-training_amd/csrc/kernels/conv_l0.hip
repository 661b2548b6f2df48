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
//                    (33.5 MB at b256), is never stored
//   l0_wgrad_finish_kernel  fixed-order sum of the block partials, added into the gradient or
//                    (registered SGD step, api.h SgdFuse) applied to the master weights
//   l0_bwd_kernel<1> the dz pass that stores dz for the weight gradient GEMM (ops/layers.py
//                    L0_WGRAD_FUSE = False; the fused variant's reference)
// Every pass runs the same conv code (conv_z) on the same inputs, so z is bit-identical to the
// forward's; the arithmetic of each step is the one of conv_smallk.hip (conv) and bn_act.hip
// (finalize, apply, first-maximum pool rule).
//
// Layout: a wave owns 16 output pixels = 2 image rows x 8 columns = four whole 2x2 pool windows,
// x 64 channels. The tile's pixels are numbered i = 4 * window + d, window 0..3 along the 8
// columns and d = 2r + (c & 1) the position in the window (bn_act.hip order), so pixel i is tile
// row (i >> 1) & 1, column 2 (i >> 2) + (i & 1). The conv is issued as mfma(x, weights): lane
// (g = lane >> 4, rl = lane & 15) gathers tap 4t + g of pixel rl as the A operand and reads the
// B operand from an LDS weight image staged once per block in permuted row order (row j * 16 + rl
// holds channel 4 rl + j). The accumulator of column tile j then holds, in registers v = 0..3,
// z of the four pixels of window g for channel 4 rl + j: a lane owns one pool window x four
// consecutive channels. Everything after the conv follows from that:
//   - the max, the first-maximum position, the ReLU cut and the winner's z of a window are over
//     four registers of one lane: no cross-lane traffic, nothing computed twice, and all 64 lanes
//     store (y and zw 8 B each, 128 B contiguous per window; the code one dword);
//   - bias and the BatchNorm coefficients are 4 values per lane, held in registers;
//   - the backward loads its window's dy (8 B) and code (one dword) once per lane;
//   - the accumulator IS the A operand (row = channel slot rl, k = pixel 4g .. 4g+3) of the
//     weight gradient's v_mfma_f32_16x16x16_bf16: dz goes from the epilogue's registers into
//     the MFMA. Only the tile's 4 x 10 input halo patch (4 of the 8 padded channels) passes
//     through LDS, written from the conv's own fragments and read per lane as the B operand
//     (k = pixel, column = tap * 3 + c: 27 real columns in two 16-column tiles, the five spare
//     columns read the zero pad channel 3). 4 x 2 MFMAs per tile, 32 accumulator registers; row
//     4g + v of accumulator jt is channel 4 (4g + v) + jt.
// The memory formats are independent of the lane layout: y, zw [N][H/2][W/2][64]; code bytes per
// window in the order [g'][j'][v'] for channel j' * 16 + 4 g' + v' (read by l0_sums_kernel and
// conv_igemm.hip BnBwdFuse::code), which for a lane's channels 4 rl + j is dword
// (rl & 3) * 4 + (rl >> 2) of the window's 16, byte j.
// The tile decode uses launch-constant FastDivs (common.h), the tap decode depends only on the
// lane and is done once per kernel. Measured: profiles/l0_lane_layout.md (this layout against
// the lane = pixel layout it replaces, profiles/l0_wgrad_fused.md).
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
  int wb, per_img;           // tiles per tile row (W / 8) and per image, and their FastDivs
  FastDiv wb_d, per_img_d;
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
                             // gradient, 4 = none (ReLU cut), 0xFF = NaN window; bytes
                             // [window][g'][j'][v'] for channel j'*16 + 4g' + v', written by the
                             // forward, read by both backward passes
  unsigned short* zw;        // [N][H/2][W/2][64] bf16: z of the pixel code points to (forward;
                             // the backward sums need nothing else of the window)
  float* dgamma;             // accumulated (arena)
  float* dbeta;
  float* wg;                 // fused weight gradient: [blocks][64][kWgN] fp32 partials
};

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 as_bf(const uint4& v) { return __builtin_bit_cast(bf16x8, v); }

// What depends on the lane alone, decoded once per kernel: the pixel the lane gathers for the
// conv's A operand (pixel rl in window order) and, per k-step, its tap's offset from the tile's
// corner. A tap past the 9 real ones gets a row far outside the image: its bounds check fails.
struct Lane {
  int g, rl;
  int ph[kNKS], pw[kNKS];  // row / column of tap 4t + g of pixel rl, relative to the tile
};

__device__ __forceinline__ Lane lane_setup() {
  Lane ln;
  const int lane = threadIdx.x & 63;
  ln.g = lane >> 4;
  ln.rl = lane & 15;
  const int pr = (ln.rl >> 1) & 1, pc = 2 * (ln.rl >> 2) + (ln.rl & 1);
#pragma unroll
  for (int t = 0; t < kNKS; ++t) {
    const int tap = 4 * t + ln.g;
    const int r = tap / 3, s = tap - r * 3;
    ln.ph[t] = tap < 9 ? pr + r - 1 : -(1 << 20);
    ln.pw[t] = pc + s - 1;
  }
  return ln;
}

// A tile (uniform over the wave): image, pooled row, block of 8 columns
struct Tile {
  int n, hp, cb;
};

__device__ __forceinline__ Tile tile_of(const Args& a, int t) {
  Tile p;
  p.n = fast_div(t, a.per_img_d);
  const int rem = t - p.n * a.per_img;
  p.hp = fast_div(rem, a.wb_d);
  p.cb = rem - p.hp * a.wb;
  return p;
}

// the lane's pool window: window g of the tile
__device__ __forceinline__ size_t window_of(const Args& a, const Tile& p, int g) {
  return ((size_t)p.n * (a.H / 2) + p.hp) * (a.W / 2) + 4 * p.cb + g;
}

// LDS weight image [64 rows][13 taps][8 ch] (12 used taps + 1 pad tap per row spreads the 16
// rows a ds_read_b128 lane group reads over the banks, conv_smallk.hip's stem layout), staged
// once per block: a per-wave register copy costs 48 VGPRs and caps the kernel at 2 waves per
// SIMD. Row j * 16 + rl holds channel 4 rl + j (the lane layout above).
constexpr int kRow = 13;
struct Smem {
  uint4 w[kK * kRow];
  float cf[3][kK];  // forward: 0 scale, 1 shift; backward: 0 scale, 1 / 2 the dz coefficients
};

__device__ __forceinline__ void stage_weights(const Args& a, Smem& sm) {
  for (int i = threadIdx.x; i < kK * 12; i += 256) {
    const int row = i / 12, tap = i - row * 12;
    const int k = 4 * (row & 15) + (row >> 4);
    sm.w[row * kRow + tap] = tap < 9 ? *reinterpret_cast<const uint4*>(a.wc + ((size_t)k * 9 + tap) * 8)
                                     : make_uint4(0, 0, 0, 0);
  }
}

// the lane's 4 values (channels 4 rl .. 4 rl + 3) of a per-channel table
__device__ __forceinline__ void lane4(const float* tab, int rl, float (&v)[kNT]) {
  const float4 q = *reinterpret_cast<const float4*>(tab + 4 * rl);
  v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
}

__device__ __forceinline__ void lane_bias(const Args& a, int rl, float (&b)[kNT]) {
#pragma unroll
  for (int j = 0; j < kNT; ++j) b[j] = a.bias ? a.bias[4 * rl + j] : 0.f;
}

// activation fragments of one tile: the lane loads tap 4t + g of its gathered pixel (16 B)
__device__ __forceinline__ void load_x(const Args& a, const Tile& p, const Lane& ln,
                                       uint4 (&xf)[kNKS]) {
  // (32-bit offsets: l0_shape_ok bounds N * H * W * 64 by 2^31)
  const int corner = (p.n * a.H + 2 * p.hp) * a.W + 8 * p.cb;
#pragma unroll
  for (int t = 0; t < kNKS; ++t) {
    const int h = 2 * p.hp + ln.ph[t], w = 8 * p.cb + ln.pw[t];
    xf[t] = ((unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W)
                ? *reinterpret_cast<const uint4*>(
                      a.x + (unsigned)((corner + ln.ph[t] * a.W + ln.pw[t]) * 8))
                : make_uint4(0, 0, 0, 0);
  }
}

// z[j][v] of the lane's window g: position v, channel 4 rl + j (bf16-rounded, + bias);
// conv_smallk.hip math with the operands exchanged: A = pixels, B = channels
__device__ __forceinline__ void conv_z(const Smem& sm, const uint4 (&xf)[kNKS],
                                       const float (&bias)[kNT], int g, int rl,
                                       float (&z)[kNT][4]) {
  f32x4 acc[kNT];
#pragma unroll
  for (int j = 0; j < kNT; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < kNKS; ++t)
#pragma unroll
    for (int j = 0; j < kNT; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          as_bf(xf[t]), as_bf(sm.w[(j * 16 + rl) * kRow + 4 * t + g]), acc[j], 0, 0, 0);
#pragma unroll
  for (int j = 0; j < kNT; ++j)
#pragma unroll
    for (int v = 0; v < 4; ++v) z[j][v] = bf2f(f2bf(acc[j][v] + bias[j]));
}

// block reduction of per-lane channel sums (lane: channels 4 rl + j of its windows): the 16
// (wave, g) partials of a channel are summed through LDS in the fixed order of their slots ->
// one atomic per channel per block into replica blockIdx.x % kStatRep (conv_smallk.hip scheme)
__device__ __forceinline__ void block_sums(const float (&s1)[kNT], const float (&s2)[kNT],
                                           float* rep, int g, int rl, float (&red)[16][2][kK]) {
  const int slot = (threadIdx.x >> 6) * 4 + g;
  *reinterpret_cast<float4*>(&red[slot][0][4 * rl]) = make_float4(s1[0], s1[1], s1[2], s1[3]);
  *reinterpret_cast<float4*>(&red[slot][1][4 * rl]) = make_float4(s2[0], s2[1], s2[2], s2[3]);
  __syncthreads();
  if (threadIdx.x < 2 * kK) {
    const int k = threadIdx.x / kK, c = threadIdx.x - k * kK;
    float t = red[0][k][c];
#pragma unroll
    for (int i = 1; i < 16; ++i) t += red[i][k][c];
    atomicAdd(rep + k * kK + c, stat_val(t, blockIdx.x));
  }
}

// one tile's global operands: the input fragments and (backward) the pooled gradient and the
// forward's verdicts of the lane's window x 4 channels
struct Ops {
  uint4 x[kNKS];
  u16x4 dy;
  unsigned code;
};

// the lane's code dword within its window's 16 (the byte order of Args::code)
__device__ __forceinline__ int code_dword(int rl) { return (rl & 3) * 4 + (rl >> 2); }

template <bool DY>
__device__ __forceinline__ void load_ops(const Args& a, const Tile& p, const Lane& ln, Ops& o) {
  load_x(a, p, ln, o.x);
  if (DY) {
    const size_t win = window_of(a, p, ln.g);
    o.dy = *reinterpret_cast<const u16x4*>(a.dy + win * kK + 4 * ln.rl);
    o.code = a.code[win * (kK / 4) + code_dword(ln.rl)];
  }
}

// Work split: a block = 4 waves, a wave walks tiles wave, wave + nw, ... (at most 1024 blocks:
// every block ends with one atomic per channel into a statistics replica). Latency is hidden by
// occupancy (waves per SIMD). Called after the block's setup and its barrier.
// PF: the next tile's operands are loaded into registers before this tile's body. Measured per
// kernel (profiles/l0_lane_layout.md): the statistics pass gains (9.3-9.5 vs 9.8-10.1 us at
// b256, 4.7 vs 5.4 us at b32), the forward loses (13.7-14.0 vs 13.1-13.2 us), and the fused
// backward does not fit it into its 128 registers (76 B of scratch), so only l0_stats takes it.
template <bool DY, bool PF, class Body>
__device__ __forceinline__ void tile_loop(const Args& a, const Lane& ln, Body body) {
  const int nw = gridDim.x * 4;
  int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (PF) {
    if (t >= a.tiles) return;
    Ops nxt;
    load_ops<DY>(a, tile_of(a, t), ln, nxt);
    for (; t < a.tiles; t += nw) {
      asm volatile("" ::: "memory");
      const Tile cur = tile_of(a, t);
      const Ops op = nxt;
      if (t + nw < a.tiles) load_ops<DY>(a, tile_of(a, t + nw), ln, nxt);
      body(cur, op);
    }
    return;
  }
  for (; t < a.tiles; t += nw) {
    // keeps the LDS weight reads inside the loop (hoisted, they are 48 VGPRs)
    asm volatile("" ::: "memory");
    const Tile cur = tile_of(a, t);
    Ops op;
    load_ops<DY>(a, cur, ln, op);
    body(cur, op);
  }
}

// forward statistics of z (no store)
__global__ __launch_bounds__(256) void l0_stats_kernel(Args a) {
  __shared__ Smem sm;
  __shared__ float red[16][2][kK];
  const Lane ln = lane_setup();
  float bias[kNT], s1[kNT] = {}, s2[kNT] = {};
  stage_weights(a, sm);
  lane_bias(a, ln.rl, bias);
  __syncthreads();
  tile_loop<false, true>(a, ln, [&](const Tile&, const Ops& op) {
    float z[kNT][4];
    conv_z(sm, op.x, bias, ln.g, ln.rl, z);
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      s1[j] += (z[j][0] + z[j][1]) + (z[j][2] + z[j][3]);
      s2[j] += (z[j][0] * z[j][0] + z[j][1] * z[j][1]) + (z[j][2] * z[j][2] + z[j][3] * z[j][3]);
    }
  });
  block_sums(s1, s2, a.stats + stat_rep(blockIdx.x) * 2 * kK, ln.g, ln.rl, red);
}

__global__ __launch_bounds__(256) void l0_fwd_kernel(Args a) {
  __shared__ Smem sm;
  const Lane ln = lane_setup();
  stage_weights(a, sm);
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
  float bias[kNT], sc[kNT], sh[kNT];
  lane_bias(a, ln.rl, bias);
  __syncthreads();
  lane4(sm.cf[0], ln.rl, sc);
  lane4(sm.cf[1], ln.rl, sh);
  tile_loop<false, false>(a, ln, [&](const Tile& cur, const Ops& op) {
    float z[kNT][4];
    conv_z(sm, op.x, bias, ln.g, ln.rl, z);
    u16x4 o, ow;
    unsigned cw = 0;
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      float y[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        y[v] = z[j][v] * sc[j] + sh[j];  // (bn_act.hip apply expression)
        // NaN-propagating like the pool's max: a NaN in the statistics marks every window
        if (a.relu) y[v] = __builtin_elementwise_maximum(y[v], 0.f);
      }
      // max over the window, NaN-propagating like bn_act.hip's pool
      const float m = __builtin_elementwise_maximum(__builtin_elementwise_maximum(y[0], y[1]),
                                                    __builtin_elementwise_maximum(y[2], y[3]));
      // the gradient's destination: the window's first maximum in window order (bn_act.hip's
      // tie rule), 0xFF when no value equals the max (a NaN window), 4 = none when ReLU zeroed
      // the whole window (its winner had y <= 0); zw is the first maximum's z either way
      unsigned pos = 0xFFu;
      float zs = 0.f;
#pragma unroll
      for (int v = 3; v >= 0; --v) {
        const bool hit = y[v] == m;
        pos = hit ? (unsigned)v : pos;
        zs = hit ? z[j][v] : zs;
      }
      const unsigned cd = pos == 0xFFu ? 0xFFu : (a.relu && !(m > 0.f)) ? 4u : pos;
      cw |= cd << (8 * j);
      o[j] = f2bf(m);
      ow[j] = f2bf(zs);  // (exact: z is bf16-valued)
    }
    const size_t win = window_of(a, cur, ln.g);
    *reinterpret_cast<u16x4*>(a.y + win * kK + 4 * ln.rl) = o;
    *reinterpret_cast<u16x4*>(a.zw + win * kK + 4 * ln.rl) = ow;
    a.code[win * (kK / 4) + code_dword(ln.rl)] = cw;
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
constexpr int kWgN = 28;            // partial's columns: n = tap * 3 + c < 27, + 1 (16-B rows)
constexpr int kWgSlab = kK * kWgN;  // fp32 per block partial (7 KB)
struct alignas(16) WgStage {        // per wave
  unsigned short xp[4 * 10][4];     // this tile's input halo patch [row][column][channels 0..3]
};
template <bool ON> struct WgLds { WgStage w[4]; };
template <> struct WgLds<false> {};

// BN backward through the recomputed z. APPLY = 1: dz stored (+ dgamma / dbeta); 2: dz kept in
// registers and contracted with the input patch into the weight gradient partial
template <int APPLY>
__device__ __forceinline__ void l0_bwd_body(const Args& a) {
  static_assert(APPLY == 1 || APPLY == 2, "dz is stored or chained into the weight gradient");
  constexpr bool WG = APPLY == 2;
  __shared__ Smem sm;
  __shared__ WgLds<WG> wl;
  const Lane ln = lane_setup();
  const int g = ln.g, rl = ln.rl, wib = threadIdx.x >> 6;
  // WG: dW[channel 4 (4g + v) + jt][column nt*16 + rl] of this wave's tiles
  f32x4 dwacc[kNT][2];
  // ... this lane's B-operand source in the patch: column n = nt*16 + rl = tap * 3 + c at the
  // tile pixels 4g .. 4g+3 = window g, positions 0..3 (+0, +1, +10, +11 patch pixels of 4 u16
  // from the window's corner, tile column 2g); n >= 27 reads the zero pad channel 3
  int xoff[2] = {0, 0};
  // ... and where its conv fragments go in the patch: tap (tr, ts) of tile pixel (r, c) is patch
  // position (r + tr, c + ts); -1 = no tap
  int pidx[kNKS] = {0, 0, 0};
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
      xoff[nt] = ((tr * 10) + 2 * g + ts) * 4 + c;
    }
#pragma unroll
    for (int t = 0; t < kNKS; ++t)
      pidx[t] = 4 * t + g < 9 ? (ln.ph[t] + 1) * 10 + ln.pw[t] + 1 : -1;
  }
  stage_weights(a, sm);
  if (threadIdx.x < kK) {
    const int c = threadIdx.x;
    // LDS rows: 0 scale, 1 / 2 with dz = scale * dy_bn + z * [1] + [2], the bn_act.hip apply
    // expression scale * (dy_bn - k1 - xhat * k2) expanded in z; k1 / k2 from the finalize of
    // the backward sums (bn_act.hip bn_finalize_bwd_kernel)
    const float sc = a.coef[c], mu = a.coef[2 * kK + c], is = a.coef[3 * kK + c];
    const float inv_m = 1.f / ((float)a.N * a.H * a.W);
    float t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int r = 0; r < kStatRep; ++r) {
      t1 += a.sums[r * 2 * kK + c];
      t2 += a.sums[r * 2 * kK + kK + c];
    }
    const float k1 = t1 * inv_m, k2 = t2 * inv_m;
    sm.cf[0][c] = sc;
    sm.cf[1][c] = -sc * k2 * is;
    sm.cf[2][c] = sc * (k2 * is * mu - k1);
    if (blockIdx.x == 0) {
      a.coef[4 * kK + c] = k1;
      a.coef[5 * kK + c] = k2;
      if (a.dgamma) a.dgamma[c] += t2;  // one writer per channel
      if (a.dbeta) a.dbeta[c] += t1;
    }
  }
  float bias[kNT], sc[kNT], cz[kNT], c0[kNT];
  lane_bias(a, rl, bias);
  __syncthreads();
  lane4(sm.cf[0], rl, sc);
  lane4(sm.cf[1], rl, cz);
  lane4(sm.cf[2], rl, c0);
  tile_loop<true, false>(a, ln, [&](const Tile& cur, const Ops& op) {
    if constexpr (WG) {
      // the halo patch from the conv's fragments; positions shared by several lanes get the
      // same value
      WgStage& st = wl.w[wib];
#pragma unroll
      for (int t = 0; t < kNKS; ++t)
        if (pidx[t] >= 0)
          *reinterpret_cast<uint2*>(st.xp[pidx[t]]) = make_uint2(op.x[t].x, op.x[t].y);
    }
    float z[kNT][4];
    conv_z(sm, op.x, bias, g, rl, z);
    u16x4 o[kNT];  // o[j][v]: dz of channel 4 rl + j at window position v
#pragma unroll
    for (int j = 0; j < kNT; ++j) {
      const unsigned cd = (op.code >> (8 * j)) & 0xFFu;
      const float dyv = bf2f(op.dy[j]);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        // the forward's verdict: this position takes the pooled gradient
        const float dyb = cd == (unsigned)v ? dyv : 0.f;
        o[j][v] = f2bf(sc[j] * dyb + (z[j][v] * cz[j] + c0[j]));
      }
    }
    if constexpr (WG) {
      // dW += dz^T x over the tile's 16 pixels: o[jt] is the A operand as it stands (row rl =
      // channel 4 rl + jt, k = pixels 4g .. 4g+3). LDS accesses of one wave complete in program
      // order, so the wave's own patch needs no barrier, only the compiler's order
      asm volatile("" ::: "memory");
      const unsigned short* xp = &wl.w[wib].xp[0][0];
      v4i16 fb[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        fb[nt][0] = (short)xp[xoff[nt]];
        fb[nt][1] = (short)xp[xoff[nt] + 4];
        fb[nt][2] = (short)xp[xoff[nt] + 40];
        fb[nt][3] = (short)xp[xoff[nt] + 44];
      }
#pragma unroll
      for (int jt = 0; jt < kNT; ++jt) {
        const v4i16 fa = __builtin_bit_cast(v4i16, o[jt]);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          dwacc[jt][nt] =
              __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fa, fb[nt], dwacc[jt][nt], 0, 0, 0);
      }
    } else {
      // pixel 4g + v: tile row v >> 1, column 2g + (v & 1); 128 B contiguous per 16 lanes
      unsigned short* dst =
          a.dz + (((size_t)cur.n * a.H + 2 * cur.hp) * a.W + 8 * cur.cb + 2 * g) * kK + 4 * rl;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const u16x4 q = {o[0][v], o[1][v], o[2][v], o[3][v]};
        *reinterpret_cast<u16x4*>(dst + ((size_t)(v >> 1) * a.W + (v & 1)) * kK) = q;
      }
    }
  });
  if constexpr (WG) {
    // the block's partial: waves summed in the fixed order ((w0 + w1) + w2) + w3 through LDS
    // (the weight image's space, free after the tile loop), stored by wave 3 as [64][kWgN]
    float* red = reinterpret_cast<float*>(sm.w);
    const int lane = threadIdx.x & 63;
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
                a.wg[(size_t)blockIdx.x * kWgSlab + (4 * (4 * g + v) + jt) * kWgN + nt * 16 + rl] = t;
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
  a.wb = g->W / 8;
  a.per_img = (g->H / 2) * a.wb;
  a.wb_d = make_fastdiv(a.wb);
  a.per_img_d = make_fastdiv(a.per_img);
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
