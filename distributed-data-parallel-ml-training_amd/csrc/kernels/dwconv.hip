// Depthwise 3x3 convolution for gfx950: forward, data gradient and weight gradient of
// Conv2d(C, C, 3, stride 1 | 2, padding 1, groups = C) (MobileNet's 3x3; bf16 NHWC activations,
// fp32 accumulation).
//
// No MFMA. A depthwise conv does 18 FLOP per output element and moves 4 bytes for it (2 in,
// 2 out): it is a streaming kernel, not a GEMM. The grouped kernel (conv_group.hip) turns a
// 32-channel slab into a dense block-diagonal 32 -> 32 conv, 2 * 9 * 32 FLOP per output element
// whatever the group size: at one channel per group that is 32x the useful work. Here every
// multiply-add is a hand-placed VALU fp32 FMA on a value the lane already holds.
//
// Design:
//   * Lane layout. A lane owns one 8-channel chunk (one 16-byte load or store) of one column of
//     the tile. Lane = slot * CL + chunk-lane: the CL chunk lanes of one pixel are consecutive,
//     then consecutive columns, so a wave's global accesses cover whole contiguous runs of NHWC
//     memory (all of a pixel row when C <= 128). CL = C / 8 up to 16 chunks, above that the
//     chunks are split evenly over blockIdx.y; CL need not be a power of two (C = 40: CL = 5,
//     51 columns, one idle lane). When the image is narrower than the 256 / CL columns of a
//     block, the spare column slots take further images (NI images per tile), so the 16x16 ..
//     1x1 layers of a CIFAR-sized input still fill the block.
//   * Weights. The operand copy stays Wc [C][3][3][Cp = 8] (only element 0 of each pitch is
//     read). A block copies its chunks' rows into LDS as they lie in memory, each lane converts
//     its 9 x 8 weights to fp32 once (72 VGPRs) and keeps them over all its tiles. DGRAD at
//     stride 1 is the same kernel with the taps mirrored at this load, no bias, no statistics.
//   * Input reuse. A tile is (chunk group, NI images, TC columns, a band of RB rows). Its input
//     rows and halo go through LDS once, as [image][row][column][chunk lane] 16-byte cells in
//     memory order, zeros stored for padding rows and columns and for idle chunks: the loop has
//     no edge cases. A lane walks down its column with a three-row window in registers (fp32);
//     per output row it reads only the new patch row, three ds_read_b128 at stride 1 (two rows,
//     six reads, at stride 2; the bottom row of one output is the top row of the next). The loop
//     is unrolled over the window's rotation, so no register is moved. Then 72 FMAs in tap order
//     starting from the bias, one rounding to bf16, one 16-byte store.
//   * LDS banks. At stride 1 consecutive lanes read consecutive 16-byte cells (a tap is a shift
//     of the whole wave by CL cells): conflict-free. At stride 2 neighbouring columns lie
//     two cell groups apart: runs of CL * 16 bytes with equal gaps, conflict-free for CL = 16
//     (256-byte runs), two-way conflicts for smaller CL (derived from the bank layout, not
//     measured).
//   * Forward epilogue. Sum and sum of squares of the rounded z stay in the lane's registers
//     over all rows and tiles, meet in LDS, are added per chunk lane in slot order by one
//     thread per channel and moment, and go as ONE atomic per channel per block into replica
//     stat_rep(blockIdx.x). The host gives a block several tiles so that gridDim.x stays within
//     kStatRep of the deterministic build.
//   * DGRAD at stride 2. A lane owns a dz column j and walks down dz rows i with a 2 x 2 window
//     (i .. i + 1, j .. j + 1; zeros past the edge). Per step it writes the four dx pixels
//     (2 i + ph, 2 j + pw) of the parity classes, with the 1, 2, 2 and 4 taps that reach them:
//     72 FMAs per four outputs, every dx element written exactly once, no zero fill.
//   * WGRAD. The same walk; instead of an output the lane adds dz (read straight from memory,
//     one row ahead) times its window into 72 fp32 accumulators that live over all its tiles.
//     The block's lanes of one chunk are added in LDS in slot order, tap by tap, and the block
//     writes one partial [C][9] slice of the workspace. Pixels are split over blocks
//     (gridDim.x) so the grid fills the chip when C / 8 is small. The finish kernel adds the
//     partials in a fixed order into dw: no float atomics, no dependence on the launch order, no
//     optimizer step. For one channel per group [K][1][3][3] and [K][3][3][1] are the same
//     element order.
//
// Limits: tensors below 2^31 elements. A patch never exceeds 64 KB of LDS (one row of the
// widest tile is 8.5 KB), so there is no limit on W.
#include "common.h"
#include "api.h"

#include <algorithm>

namespace ddp_amd {
namespace dw {

constexpr int kLds = 64 * 1024;     // patch budget: two blocks per CU
constexpr int kLdsMin = 18 * 1024;  // 16 chunks of raw weights (18 KB) / statistics (16 KB)
constexpr int kMaxRows = 16;        // output rows of a band

struct Args {
  const unsigned short* in;   // FWD, WGRAD: x; DGRAD: dz
  unsigned short* out;        // FWD: z; DGRAD: dx
  const unsigned short* wc;   // [C][3][3][8]
  const float* bias;          // FWD only (may be null)
  float* stats;               // FWD only (may be null): [kStatRep][2][C]
  const unsigned short* dz;   // WGRAD
  float* ws;                  // WGRAD: partials [split][C][9]
  int N, IH, IW, OH, OW, C;   // I: the tensor the patch is cut from; O: the tensor written
  int LH, LW;                 // rows / columns the lanes walk (stride-2 DGRAD: dz's; else O's)
  int nch, CL, TC, NI, RB;    // chunks, chunk lanes, tile columns, tile images, band rows
  int PR, PW;                 // patch rows, columns
  int ncol, bands, ntiles, tpb;
  FastDiv dCL, dPW, dPR, dTC, dNcol, dBands;
};

struct F8 { float v[8]; };
template <int NC> struct Row { F8 c[NC]; };  // NC columns of one patch row, fp32

__device__ __forceinline__ F8 cvt8(uint4 u) {
  F8 r;
  r.v[0] = __uint_as_float(u.x << 16); r.v[1] = __uint_as_float(u.x & 0xffff0000u);
  r.v[2] = __uint_as_float(u.y << 16); r.v[3] = __uint_as_float(u.y & 0xffff0000u);
  r.v[4] = __uint_as_float(u.z << 16); r.v[5] = __uint_as_float(u.z & 0xffff0000u);
  r.v[6] = __uint_as_float(u.w << 16); r.v[7] = __uint_as_float(u.w & 0xffff0000u);
  return r;
}
__device__ __forceinline__ uint4 pack8(const float* f) {
  uint4 u;
  u.x = (unsigned)f2bf(f[0]) | ((unsigned)f2bf(f[1]) << 16);
  u.y = (unsigned)f2bf(f[2]) | ((unsigned)f2bf(f[3]) << 16);
  u.z = (unsigned)f2bf(f[4]) | ((unsigned)f2bf(f[5]) << 16);
  u.w = (unsigned)f2bf(f[6]) | ((unsigned)f2bf(f[7]) << 16);
  return u;
}
template <int NC>
__device__ __forceinline__ void load_row(Row<NC>& r, const char* p, int cpitch) {
#pragma unroll
  for (int c = 0; c < NC; ++c) r.c[c] = cvt8(*reinterpret_cast<const uint4*>(p + c * cpitch));
}

// the tile's patch -> LDS [image][row][column][chunk lane]; zeros outside the image, past the
// batch and for chunk lanes past C / 8
__device__ __forceinline__ void stage_patch(const Args& a, char* lds, int n0, int ir0, int ic0,
                                            int grp) {
  const int items = a.NI * a.PR * a.PW * a.CL;
#pragma unroll 2
  for (int it = threadIdx.x; it < items; it += 256) {
    const int q = fast_div(it, a.dCL), cl = it - q * a.CL;
    const int t = fast_div(q, a.dPW), pc = q - t * a.PW;
    const int img = fast_div(t, a.dPR), pr = t - img * a.PR;
    const int n = n0 + img, ih = ir0 + pr, iw = ic0 + pc, chunk = grp * a.CL + cl;
    uint4 v = {0u, 0u, 0u, 0u};
    if (n < a.N && ih >= 0 && ih < a.IH && iw >= 0 && iw < a.IW && chunk < a.nch)
      v = *reinterpret_cast<const uint4*>(a.in + (((size_t)n * a.IH + ih) * a.IW + iw) * a.C +
                                          chunk * 8);
    *reinterpret_cast<uint4*>(lds + (size_t)it * 16) = v;
  }
}

// Walk ``nr`` lane rows down the patch column at p: emit(r, top, mid, bot) per row with the
// three patch rows r * S .. r * S + 2, each loaded once. The rotation of the window is unrolled.
template <int S, typename F>
__device__ __forceinline__ void walk3(const char* p, int rpitch, int cpitch, int nr, F&& emit) {
  Row<3> A, B, C;
  if (S == 1) {
    load_row(A, p, cpitch);
    load_row(B, p + rpitch, cpitch);
    for (int r = 0; r < nr; r += 3) {
      const char* q = p + (r + 2) * rpitch;
      load_row(C, q, cpitch);
      emit(r, A, B, C);
      if (r + 1 >= nr) break;
      load_row(A, q + rpitch, cpitch);
      emit(r + 1, B, C, A);
      if (r + 2 >= nr) break;
      load_row(B, q + 2 * rpitch, cpitch);
      emit(r + 2, C, A, B);
    }
  } else {
    load_row(A, p, cpitch);
    for (int r = 0; r < nr; r += 2) {
      const char* q = p + (2 * r + 1) * rpitch;
      load_row(B, q, cpitch);
      load_row(C, q + rpitch, cpitch);
      emit(r, A, B, C);
      if (r + 1 >= nr) break;
      load_row(B, q + 2 * rpitch, cpitch);
      load_row(A, q + 3 * rpitch, cpitch);
      emit(r + 1, C, B, A);
    }
  }
}

// OP 0: FWD, 1: DGRAD, 2: WGRAD; S: the conv stride
template <int S, int OP>
__global__ __launch_bounds__(256) void dwconv_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool D2 = OP == 1 && S == 2;  // parity-class DGRAD
  constexpr int PS = OP == 1 ? 1 : S;     // patch columns / rows per lane column / row
  const int tid = threadIdx.x, grp = blockIdx.y;
  const int CL = a.CL, C = a.C;
  int slot = fast_div(tid, a.dCL);
  const int cl = tid - slot * CL;
  const bool chunk_ok = grp * CL + cl < a.nch;
  const int chunk = chunk_ok ? grp * CL + cl : 0;
  const bool lane_ok = chunk_ok && slot < a.NI * a.TC;
  if (slot >= a.NI * a.TC) slot = 0;  // idle lanes read slot 0's cells and write nothing
  const int img = fast_div(slot, a.dTC), col = slot - img * a.TC;
  const int cpitch = CL * 16, rpitch = a.PW * cpitch;
  const char* lp = smem + ((size_t)(img * a.PR * a.PW + col * PS) * CL + cl) * 16;

  // ---- this lane's 9 x 8 weights, fp32, from the block's rows of Wc
  float w[9][8];
  float bj[8];
  if (OP != 2) {
    const int nc = min(CL, a.nch - grp * CL);
    const uint4* src = reinterpret_cast<const uint4*>(a.wc + (size_t)grp * CL * 576);
    for (int i = tid; i < nc * 72; i += 256) reinterpret_cast<uint4*>(smem)[i] = src[i];
    __syncthreads();
    const unsigned short* wr = reinterpret_cast<const unsigned short*>(smem) +
                               (chunk_ok ? cl : 0) * 576;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        w[t][e] = bf2f(wr[(e * 9 + ((OP == 1 && S == 1) ? 8 - t : t)) * 8]);
#pragma unroll
    for (int e = 0; e < 8; ++e) bj[e] = (OP == 0 && a.bias) ? a.bias[chunk * 8 + e] : 0.f;
  }
  float s1[8] = {}, s2[8] = {};
  const bool red = OP == 0 && a.stats != nullptr;
  float acc[9][8];  // WGRAD
  if (OP == 2) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[t][e] = 0.f;
  }

  const int t0 = blockIdx.x * a.tpb, t1 = min(a.ntiles, t0 + a.tpb);
  for (int tile = t0; tile < t1; ++tile) {
    const int tq = fast_div(tile, a.dNcol), ct = tile - tq * a.ncol;
    const int ng = fast_div(tq, a.dBands), band = tq - ng * a.bands;
    const int n0 = ng * a.NI, r0 = band * a.RB, c0 = ct * a.TC;
    const int nr = min(a.RB, a.LH - r0);
    __syncthreads();  // the raw weights / the previous tile's patch have been read
    stage_patch(a, smem, n0, D2 ? r0 : r0 * PS - 1, D2 ? c0 : c0 * PS - 1, grp);
    __syncthreads();
    const int n = n0 + img, c = c0 + col;
    const bool ok = lane_ok && n < a.N && c < a.LW;

    if (OP == 0 || (OP == 1 && S == 1)) {
      unsigned short* o = a.out + (((size_t)n * a.OH + r0) * a.OW + c) * C + chunk * 8;
      const size_t orow = (size_t)a.OW * C;
      walk3<PS>(lp, rpitch, cpitch, nr, [&](int r, const Row<3>& R0, const Row<3>& R1,
                                            const Row<3>& R2) {
        if (!ok) return;
        float z[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = bj[e];
#pragma unroll
          for (int s = 0; s < 3; ++s) v = __builtin_fmaf(w[s][e], R0.c[s].v[e], v);
#pragma unroll
          for (int s = 0; s < 3; ++s) v = __builtin_fmaf(w[3 + s][e], R1.c[s].v[e], v);
#pragma unroll
          for (int s = 0; s < 3; ++s) v = __builtin_fmaf(w[6 + s][e], R2.c[s].v[e], v);
          z[e] = v;
        }
        const uint4 pk = pack8(z);
        *reinterpret_cast<uint4*>(o + r * orow) = pk;
        if (red) {  // statistics of the stored (bf16-rounded) values
          const F8 q = cvt8(pk);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            s1[e] += q.v[e];
            s2[e] = __builtin_fmaf(q.v[e], q.v[e], s2[e]);
          }
        }
      });
    } else if (D2) {
      // dz window d[i .. i + 1][j .. j + 1]; dx (2 i + ph, 2 j + pw) takes the weight taps
      // (tr, ts) with tr == 1 for ph == 0, tr in {0, 2} for ph == 1 (columns alike), at dz
      // (i + (tr == 0), j + (ts == 0))
      const int oh0 = 2 * r0, ow = 2 * c;
      unsigned short* o = a.out + (((size_t)n * a.OH + oh0) * a.OW + ow) * C + chunk * 8;
      const size_t orow = (size_t)a.OW * C;
      const bool wide = ow + 1 < a.OW;
      auto emit = [&](int i, const Row<2>& T, const Row<2>& Bt) {
        if (!ok) return;
        float x00[8], x01[8], x10[8], x11[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d00 = T.c[0].v[e], d01 = T.c[1].v[e], d10 = Bt.c[0].v[e], d11 = Bt.c[1].v[e];
          // every sum starts from +0, as an accumulator does (a bare product can be -0)
          x00[e] = __builtin_fmaf(d00, w[4][e], 0.f);
          x01[e] = __builtin_fmaf(d00, w[5][e], __builtin_fmaf(d01, w[3][e], 0.f));
          x10[e] = __builtin_fmaf(d00, w[7][e], __builtin_fmaf(d10, w[1][e], 0.f));
          float v = __builtin_fmaf(d11, w[0][e], 0.f);
          v = __builtin_fmaf(d10, w[2][e], v);
          v = __builtin_fmaf(d01, w[6][e], v);
          x11[e] = __builtin_fmaf(d00, w[8][e], v);
        }
        unsigned short* p = o + (size_t)(2 * i) * orow;
        *reinterpret_cast<uint4*>(p) = pack8(x00);
        if (wide) *reinterpret_cast<uint4*>(p + C) = pack8(x01);
        if (oh0 + 2 * i + 1 < a.OH) {
          *reinterpret_cast<uint4*>(p + orow) = pack8(x10);
          if (wide) *reinterpret_cast<uint4*>(p + orow + C) = pack8(x11);
        }
      };
      Row<2> A, B;
      load_row(A, lp, cpitch);
      for (int i = 0; i < nr; i += 2) {
        const char* q = lp + (i + 1) * rpitch;
        load_row(B, q, cpitch);
        emit(i, A, B);
        if (i + 1 >= nr) break;
        load_row(A, q + rpitch, cpitch);
        emit(i + 1, B, A);
      }
    } else {
      // WGRAD: acc[t] += dz * x[t]; dz one row ahead of its use
      const unsigned short* d = a.dz + (((size_t)n * a.OH + r0) * a.OW + c) * C + chunk * 8;
      const size_t orow = (size_t)a.OW * C;
      uint4 nxt = {0u, 0u, 0u, 0u};
      if (ok) nxt = *reinterpret_cast<const uint4*>(d);
      walk3<PS>(lp, rpitch, cpitch, nr, [&](int r, const Row<3>& R0, const Row<3>& R1,
                                            const Row<3>& R2) {
        if (!ok) return;
        const F8 g = cvt8(nxt);
        if (r + 1 < nr) nxt = *reinterpret_cast<const uint4*>(d + (r + 1) * orow);
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            acc[s][e] = __builtin_fmaf(g.v[e], R0.c[s].v[e], acc[s][e]);
            acc[3 + s][e] = __builtin_fmaf(g.v[e], R1.c[s].v[e], acc[3 + s][e]);
            acc[6 + s][e] = __builtin_fmaf(g.v[e], R2.c[s].v[e], acc[6 + s][e]);
          }
      });
    }
  }

  const int nslot = 256 / CL;  // slots whose lanes all exist
  if (OP == 0) {
    if (!red) return;
    // ---- statistics: [lane][moment][8] in LDS, one thread per (chunk lane, moment, channel)
    // adds the slots in order, then one atomic each
    __syncthreads();
    float* sl = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sl[tid * 16 + e] = s1[e];
      sl[tid * 16 + 8 + e] = s2[e];
    }
    __syncthreads();
    if (tid < CL * 16) {
      const int rcl = tid >> 4, j = tid & 15;
      float v = 0.f;
      for (int s = 0; s < nslot; ++s) v += sl[(s * CL + rcl) * 16 + j];
      const int ch = (grp * CL + rcl) * 8 + (j & 7);
      if (grp * CL + rcl < a.nch) {
        float* st = a.stats + (size_t)stat_rep(blockIdx.x) * 2 * C;
        atomicAdd(st + (j >> 3) * C + ch, stat_val(v, blockIdx.x));
      }
    }
  } else if (OP == 2) {
    // ---- the block's lanes of one chunk, added in slot order, tap by tap
    float* rd = reinterpret_cast<float*>(smem);
    float* dst = a.ws + (size_t)blockIdx.x * C * 9;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      __syncthreads();
#pragma unroll
      for (int e = 0; e < 8; ++e) rd[tid * 8 + e] = acc[t][e];
      __syncthreads();
      if (tid < CL * 8) {
        const int rcl = tid >> 3, e = tid & 7;
        float v = 0.f;
        for (int s = 0; s < nslot; ++s) v += rd[(s * CL + rcl) * 8 + e];
        if (grp * CL + rcl < a.nch) dst[((grp * CL + rcl) * 8 + e) * 9 + t] = v;
      }
    }
  }
}

// dw += the partials. A block owns 32 elements; eight lanes per element each add every eighth
// split in split order, then one lane adds the eight sums in lane order: a fixed order, an
// eighth of the serial chain. [K][1][3][3] and [K][3][3][1] enumerate the elements alike.
__global__ __launch_bounds__(256)
void dwconv_wgrad_finish_kernel(const float* __restrict__ ws, float* __restrict__ dw, int total,
                                int splits) {
  __shared__ float red[8][32];
  const int el = threadIdx.x & 31, part = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + el;
  float s = 0.f;
  if (e < total) {
#pragma unroll 4
    for (int sp = part; sp < splits; sp += 8) s += ws[(size_t)sp * total + e];
  }
  red[part][el] = s;
  __syncthreads();
  if (part == 0 && e < total) {
    float v = red[0][el];
#pragma unroll
    for (int i = 1; i < 8; ++i) v += red[i][el];
    dw[e] += v;
  }
}

// ------------------------------------------------------------------ host side
// mode: 0 FWD, 1 DGRAD, 2 WGRAD
static void plan(const ConvGeom* g, int mode, Args* a, size_t* lds) {
  Args& r = *a;
  const bool d2 = mode == 1 && g->stride == 2;
  const int ps = mode == 1 ? 1 : g->stride;
  r.N = g->N; r.C = g->C;
  if (mode == 1) { r.IH = g->P; r.IW = g->Q; r.OH = g->H; r.OW = g->W; }
  else { r.IH = g->H; r.IW = g->W; r.OH = g->P; r.OW = g->Q; }
  r.LH = d2 ? g->P : r.OH;
  r.LW = d2 ? g->Q : r.OW;
  r.nch = r.C / 8;
  const int ngrp = (r.nch + 15) / 16;
  r.CL = (r.nch + ngrp - 1) / ngrp;
  const int tw = 256 / r.CL;
  r.ncol = (r.LW + tw - 1) / tw;
  r.TC = (r.LW + r.ncol - 1) / r.ncol;
  r.NI = std::max(1, std::min(r.N, tw / r.TC));
  r.PW = d2 ? r.TC + 1 : (r.TC - 1) * ps + 3;
  // band: as many rows as the patch budget holds, then evened out over the bands
  const int prmax = kLds / (r.NI * r.PW * r.CL * 16);
  int rb = d2 ? prmax - 1 : (prmax - 3) / ps + 1;
  rb = std::max(1, std::min(std::min(rb, kMaxRows), r.LH));
  r.bands = (r.LH + rb - 1) / rb;
  r.RB = (r.LH + r.bands - 1) / r.bands;
  r.PR = d2 ? r.RB + 1 : (r.RB - 1) * ps + 3;
  r.ntiles = (r.N + r.NI - 1) / r.NI * r.bands * r.ncol;
  // blocks: about 2048, and at most 4096 along x (a block owns its statistics replica in the
  // deterministic build)
  const long long ts = (long long)r.ntiles * ngrp;
  const int tpb = (int)std::min<long long>(16, std::max<long long>(1, (ts + 2047) / 2048));
  r.tpb = std::max(tpb, (r.ntiles + 4095) / 4096);
  r.dCL = make_fastdiv(r.CL);
  r.dPW = make_fastdiv(r.PW);
  r.dPR = make_fastdiv(r.PR);
  r.dTC = make_fastdiv(r.TC);
  r.dNcol = make_fastdiv(r.ncol);
  r.dBands = make_fastdiv(r.bands);
  *lds = std::max((size_t)r.NI * r.PR * r.PW * r.CL * 16, (size_t)kLdsMin);
}

static bool served(const ConvGeom* g, int groups) {
  if (!g || g->N < 1 || g->H < 1 || g->W < 1 || g->C < 8 || g->C % 8) return false;
  if (g->R != 3 || g->S != 3 || g->pad != 1 || (g->stride != 1 && g->stride != 2)) return false;
  if (g->C != g->K || groups != g->C || g->Creal != 1) return false;
  if (g->P != (g->H - 1) / g->stride + 1 || g->Q != (g->W - 1) / g->stride + 1) return false;
  if ((size_t)g->N * g->H * g->W * g->C >= 0x80000000ull) return false;
  return true;
}

template <int OP>
static int launch(const ConvGeom* g, const Args& a, size_t lds, int gx, hipStream_t st) {
  const dim3 grid(gx, (a.nch + a.CL - 1) / a.CL);
  if (g->stride == 2) hipLaunchKernelGGL((dwconv_kernel<2, OP>), grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL((dwconv_kernel<1, OP>), grid, dim3(256), lds, st, a);
  const int e = (int)hipGetLastError();
  return e ? 2 + e : 1;
}

}  // namespace dw
}  // namespace ddp_amd

using namespace ddp_amd;

extern "C" int ddp_dwconv_ok(const ConvGeom* g, int groups) { return dw::served(g, groups) ? 1 : 0; }

extern "C" int ddp_dwconv_fwd(const ConvGeom* g, int groups, const void* x, const void* wc,
                              const float* bias, void* z, float* stats, hipStream_t st) {
  if (!dw::served(g, groups) || !x || !wc || !z) return -1;
  dw::Args a{};
  size_t lds;
  dw::plan(g, 0, &a, &lds);
  a.in = (const unsigned short*)x;
  a.out = (unsigned short*)z;
  a.wc = (const unsigned short*)wc;
  a.bias = bias;
  a.stats = stats;
  return dw::launch<0>(g, a, lds, (a.ntiles + a.tpb - 1) / a.tpb, st);
}

extern "C" int ddp_dwconv_dgrad(const ConvGeom* g, int groups, const void* dz, const void* wc,
                                void* dx, hipStream_t st) {
  if (!dw::served(g, groups) || !dz || !wc || !dx) return -1;
  dw::Args a{};
  size_t lds;
  dw::plan(g, 1, &a, &lds);
  a.in = (const unsigned short*)dz;
  a.out = (unsigned short*)dx;
  a.wc = (const unsigned short*)wc;
  return dw::launch<1>(g, a, lds, (a.ntiles + a.tpb - 1) / a.tpb, st);
}

extern "C" int ddp_dwconv_wgrad(const ConvGeom* g, int groups, const void* dz, const void* x,
                                float* dw_, float* ws, size_t ws_elems, hipStream_t st) {
  if (!dw::served(g, groups) || !dz || !x || !dw_ || !ws) return -1;
  dw::Args a{};
  size_t lds;
  dw::plan(g, 2, &a, &lds);
  const int total = a.C * 9;
  if (ws_elems < (size_t)total) return -2;
  // pixel split: about 1024 blocks, as many as the workspace holds
  const int ngrp = (a.nch + a.CL - 1) / a.CL;
  int splits = std::max(1, std::min(a.ntiles, 1024 / ngrp));
  splits = (int)std::min<size_t>(splits, ws_elems / (size_t)total);
  a.tpb = (a.ntiles + splits - 1) / splits;
  splits = (a.ntiles + a.tpb - 1) / a.tpb;  // every block has at least one tile
  a.in = (const unsigned short*)x;
  a.dz = (const unsigned short*)dz;
  a.ws = ws;
  const int rc = dw::launch<2>(g, a, lds, splits, st);
  if (rc != 1) return rc;
  hipLaunchKernelGGL(dw::dwconv_wgrad_finish_kernel, dim3((total + 31) / 32), dim3(256), 0, st,
                     ws, dw_, total, splits);
  const int e = (int)hipGetLastError();
  return e ? 2 + e : 1;
}
