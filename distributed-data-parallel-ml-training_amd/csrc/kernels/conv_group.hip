// Grouped 3x3 convolution for gfx950: forward, data gradient and weight gradient of
// Conv2d(C, C, 3, stride 1 | 2, padding 1, groups = C / Cg) with Cg in {4, 8, 16, 32}
// (ResNeXt's conv2; bf16 MFMA v_mfma_f32_16x16x32_bf16, fp32 accumulation).
//
// Why a kernel of its own: with 4 to 32 input channels per group an implicit GEMM per group has a
// reduction of 36 to 288 and 4 to 32 output columns, below every tile of conv_igemm.hip. Here the
// work item is (32-channel slab, band of output rows): a slab holds 32 / Cg whole groups, so its
// conv is an independent dense 32 -> 32 3x3 conv whose per-tap weight matrix is block-diagonal,
// and channel slab s of the input feeds only slab s of the output. The dense-ified slab costs
// 2 * 9 * 32 FLOP per output element whatever Cg (derived, not measured: ResNet-50's own conv2
// FLOP count at layer1, an eighth of it at layer4).
//
// Design, and where it leaves the recommended one (32x32x16 MFMA, 18 KB of expanded weights in
// LDS):
//   * MFMA shape 16x16x32, not 32x32x16. One k-step of 32 is exactly one tap of the slab, both
//     shapes run at the same MFMA rate, and the operand / result lane layout is the one every
//     other MFMA kernel of this library uses (operands swapped so that a lane owns one pixel and
//     four consecutive channels: 8-byte bf16 stores).
//   * The expanded weights live in REGISTERS, not LDS: a block copies its slab's rows of Wc
//     ([32][3][3][Cp], at most 18 KB) into LDS as they lie in memory, and every wave gathers its
//     18 fragments (9 taps x 2 halves of the output channels, 72 VGPRs) from it once, writing
//     zeros off the block diagonal. The pad channels of Cg = 4 (Cp = 8) are never read. DGRAD
//     gathers the same copy transposed per group and with the taps mirrored: no Wt copy. The
//     block then walks over ``tpb`` pixel tiles with the weights resident, so the inner loop reads
//     only pixels from LDS (9 ds_read_b128 per 18 MFMAs) and the LDS that held the raw weights
//     is reused for the input patch.
//   * Input patch: the band's input rows plus halo, 64 B per pixel, zeros stored for the padding
//     (rows and columns: no edge cases in the loop), as four chunk planes [chunk][pixel] of 16 B
//     so that 16 consecutive pixels of one chunk are 256 contiguous bytes (conflict-free
//     ds_read_b128 at stride 1; two-way conflicts at stride 2). The nine taps are shifted reads.
//   * Stride-2 DGRAD visits only the taps whose parity reaches an output pixel: the dx pixels of
//     a band are walked in their four (row, column) parity classes, with 1, 2, 2 and 4 taps.
//   * Forward epilogue: bias, bf16 z, BatchNorm statistics of the rounded values kept in
//     registers over all tiles of the block, reduced over the wave (DPP) and the block (LDS), then
//     ONE atomic per channel into replica stat_rep(blockIdx.x) of [kStatRep][2][K]. Blocks of
//     different slabs touch different channels, so in the deterministic build a block still owns
//     every address it adds to (gridDim.x <= kStatRep is kept by the host).
//   * WGRAD: per slab dW[32][9][32] = sum over pixels dz^T x shifted x. The reduction runs over
//     pixels, which NHWC keeps strided, so both operands stay [pixel][32 channels] in LDS and the
//     fragments come from ds_read_b64_tr_b16 (each lane points at its own pixel row, so a tap is
//     again a shifted address). A wave owns whole 32-pixel k-steps and all 36 output tiles
//     (144 accumulator VGPRs, two waves per SIMD); the four waves are added in LDS in wave order
//     and the block writes one fp32 partial [32][9][32] into the workspace. Pixels are split
//     over blocks (C / 32 is only 4 to 32 slabs). The finish kernel adds the partials in split
//     order and adds the diagonal blocks into dw in either master layout: no float atomics, the
//     result does not depend on the launch order. It takes no optimizer step.
//
// Limits: one band of one output row must fit LDS (W <= 800); tensors below 2^31 elements.
#include "common.h"
#include "api.h"

#include <algorithm>
#include <type_traits>

namespace ddp_amd {
namespace gc {

typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef short short8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;

constexpr int kMaxLds = 156 * 1024;
constexpr int kPartial = 32 * 9 * 32;  // fp32 elements of one WGRAD partial

struct Args {
  const unsigned short* in;   // FWD: x [N][IH][IW][C]; DGRAD: dz
  unsigned short* out;        // FWD: z [N][OH][OW][C]; DGRAD: dx
  const unsigned short* wc;   // [C][3][3][Cp]
  const float* bias;          // FWD only (may be null)
  float* stats;               // FWD only (may be null): [kStatRep][2][C]
  const unsigned short* dz;   // WGRAD: [N][OH][OW][C] (``in`` is x)
  float* ws;                  // WGRAD: partials [slab][split][32][9][32]
  int N, IH, IW, OH, OW, C;
  int s;                      // patch pixels per output pixel step (the conv stride; DGRAD: 1)
  int dgrad, lg, Cp;          // lg = log2(Cg)
  int rows, bands, ntiles, tpb;  // output rows per tile, tiles per image, tiles, tiles per block
  int PR, PW, plane;          // patch rows, columns, pixels per chunk plane
  FastDiv dBands, dPW, dOW, dJ0, dJ1;  // dJ0 / dJ1: dx columns of parity 0 / 1 (stride-2 DGRAD)
};

// tile -> image n, first output row r0, output rows in it
__device__ __forceinline__ void tile_of(const Args& a, int tile, int& n, int& r0, int& nr) {
  n = fast_div(tile, a.dBands);
  r0 = (tile - n * a.bands) * a.rows;
  nr = min(a.rows, a.OH - r0);
}

// first input row / column of the patch (MODE 1 = stride-2 DGRAD: dz rows r0 / 2 .., no halo
// before; else the rows of the band at stride s with a one-pixel halo)
template <int MODE>
__device__ __forceinline__ void patch_origin(const Args& a, int r0, int& ir0, int& ic0) {
  ir0 = MODE == 1 ? (r0 >> 1) : r0 * a.s - 1;
  ic0 = MODE == 1 ? 0 : -1;
}

// the slab's 32 channels of the patch pixels -> LDS. PLANES: [chunk][pixel] 16-B planes, else
// [pixel][32] rows of 64 B. Pixels outside the image are stored as zeros.
template <bool PLANES>
__device__ __forceinline__ void stage_patch(const Args& a, char* lds, int n, int ir0, int ic0,
                                            int slab) {
  const int items = a.PR * a.PW * 4;
  const unsigned short* src = a.in + (size_t)n * a.IH * a.IW * a.C + slab * 32;
#pragma unroll 4
  for (int it = threadIdx.x; it < items; it += 256) {
    const int pix = it >> 2, q = it & 3;
    const int pr = fast_div(pix, a.dPW), pc = pix - pr * a.PW;
    const int ih = ir0 + pr, iw = ic0 + pc;
    uint4 v = {0u, 0u, 0u, 0u};
    if (ih >= 0 && ih < a.IH && iw >= 0 && iw < a.IW)
      v = *reinterpret_cast<const uint4*>(src + ((size_t)ih * a.IW + iw) * a.C + q * 8);
    const int off = PLANES ? (q * a.plane + pix) * 16 : pix * 64 + q * 16;
    *reinterpret_cast<uint4*>(lds + off) = v;
  }
}

// ------------------------------------------------------------------ FWD / DGRAD
// MODE 0: all nine taps per output pixel (FWD at stride 1 / 2, DGRAD at stride 1).
// MODE 1: DGRAD at stride 2, the dx pixels of a band in four parity classes.
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4)))
void gconv_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int slab = blockIdx.y;
  const int C = a.C, PW = a.PW;
  __builtin_assume(PW >= 1);

  // ---- the slab's rows of Wc as they lie in memory, then this wave's 18 fragments: row
  // m = 16 hf + fr, k = 8 fq + e. FWD: (m, k) = (output, input) channel of the slab, tap t.
  // DGRAD: (m, k) = (input, output) channel; MODE 0 reads the patch at tap t with the mirrored
  // weight tap 8 - t, MODE 1 indexes the fragments by the weight tap itself.
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.wc + (size_t)slab * 288 * a.Cp);
    for (int i = tid; i < 36 * a.Cp; i += 256) reinterpret_cast<uint4*>(smem)[i] = src[i];
  }
  __syncthreads();
  bf16x8 wf[9][2];
  {
    const unsigned short* wr = reinterpret_cast<const unsigned short*>(smem);
    const int cmask = (1 << a.lg) - 1;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int tw = (a.dgrad && MODE == 0) ? 8 - t : t;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int m = 16 * hf + fr;
        u16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = 8 * fq + e;
          const int co = a.dgrad ? k : m, ci = a.dgrad ? m : k;
          const bool same = (co >> a.lg) == (ci >> a.lg);
          const unsigned short w = wr[(co * 9 + tw) * a.Cp + (ci & cmask)];
          v[e] = same ? w : (unsigned short)0;
        }
        wf[t][hf] = __builtin_bit_cast(bf16x8, v);
      }
    }
  }

  float bj[2][4];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int v = 0; v < 4; ++v)
      bj[hf][v] = a.bias ? a.bias[slab * 32 + 16 * hf + 4 * fq + v] : 0.f;
  float s1[2][4] = {}, s2[2][4] = {};
  const bool red = a.stats != nullptr;

  // one 16-pixel group of outputs: ``base`` = patch pixel of tap (0, 0), ``opix`` = output pixel
  // index in [N][OH][OW]; TAPS = bit t set: tap t is visited, at patch offset off(t)
  auto group = [&](bool valid, int base, size_t opix, auto taps) {
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const char* p = smem + (fq * a.plane + base) * 16;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int off = taps(t);
      if (off < 0) continue;
      const bf16x8 xf = *reinterpret_cast<const bf16x8*>(p + off * 16);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        acc[hf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[t][hf], xf, acc[hf], 0, 0, 0);
    }
    if (!valid) return;
    unsigned short* o = a.out + opix * C + slab * 32 + 4 * fq;
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const f32x4 v = acc[hf];
      uint2 pk;
      pk.x = (unsigned)f2bf(v[0] + bj[hf][0]) | ((unsigned)f2bf(v[1] + bj[hf][1]) << 16);
      pk.y = (unsigned)f2bf(v[2] + bj[hf][2]) | ((unsigned)f2bf(v[3] + bj[hf][3]) << 16);
      *reinterpret_cast<uint2*>(o + 16 * hf) = pk;
      if (red) {  // statistics of the stored (bf16-rounded) values
        const float r0 = __uint_as_float(pk.x << 16), r1 = __uint_as_float(pk.x & 0xffff0000u);
        const float r2 = __uint_as_float(pk.y << 16), r3 = __uint_as_float(pk.y & 0xffff0000u);
        s1[hf][0] += r0; s1[hf][1] += r1; s1[hf][2] += r2; s1[hf][3] += r3;
        s2[hf][0] += r0 * r0; s2[hf][1] += r1 * r1; s2[hf][2] += r2 * r2; s2[hf][3] += r3 * r3;
      }
    }
  };

  const int t0 = blockIdx.x * a.tpb, t1 = min(a.ntiles, t0 + a.tpb);
  for (int tile = t0; tile < t1; ++tile) {
    int n, r0, nr, ir0, ic0;
    tile_of(a, tile, n, r0, nr);
    patch_origin<MODE>(a, r0, ir0, ic0);
    __syncthreads();  // the raw weights / the previous tile's patch have been read
    stage_patch<true>(a, smem, n, ir0, ic0, slab);
    __syncthreads();
    const size_t obase = ((size_t)n * a.OH + r0) * a.OW;
    if (MODE == 0) {
      const int npx = nr * a.OW;
      for (int g = wid; g * 16 < npx; g += 4) {
        const int o = g * 16 + fr;
        const bool valid = o < npx;
        const int oc = valid ? o : 0;
        const int r = fast_div(oc, a.dOW), c = oc - r * a.OW;
        group(valid, (r * PW + c) * a.s, obase + oc,
              [&](int t) { return (t / 3) * PW + t % 3; });
      }
    } else {
      // dx pixel (r0 + 2 i + ph, 2 j + pw) takes the weight taps (tr, ts) with tr == 1 for
      // ph == 0, tr in {0, 2} for ph == 1 (columns alike), at dz pixel (i + (tr == 0),
      // j + (ts == 0)) of the patch
      auto cls = [&](auto PH, auto PWc) {
        constexpr int ph = decltype(PH)::value, pw = decltype(PWc)::value;
        const int ni = (nr - ph + 1) >> 1, nj = (a.OW - pw + 1) >> 1;
        const int npx = ni * nj;
        for (int g = wid; g * 16 < npx; g += 4) {
          const int o = g * 16 + fr;
          const bool valid = o < npx;
          const int oc = valid ? o : 0;
          const int i = fast_div(oc, pw ? a.dJ1 : a.dJ0), j = oc - i * nj;
          group(valid, i * PW + j, obase + (size_t)(2 * i + ph) * a.OW + 2 * j + pw,
                [&](int t) {
                  const int tr = t / 3, ts = t % 3;
                  const bool use = (ph ? tr != 1 : tr == 1) && (pw ? ts != 1 : ts == 1);
                  return use ? (tr == 0 ? PW : 0) + (ts == 0 ? 1 : 0) : -1;
                });
        }
      };
      cls(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
      cls(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
      cls(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
      cls(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
    }
  }
  if (!red) return;

  // ---- statistics: lanes of a 16-lane row hold the same channels (DPP sum), the four waves
  // meet in LDS, then one atomic per channel and moment
  __syncthreads();
  float* sl = reinterpret_cast<float*>(smem);  // [wave][2][32]
#pragma unroll
  for (int hf = 0; hf < 2; ++hf)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float x1 = dpp_sum16(s1[hf][v]), x2 = dpp_sum16(s2[hf][v]);
      if (fr == 0) {
        sl[wid * 64 + 16 * hf + 4 * fq + v] = x1;
        sl[wid * 64 + 32 + 16 * hf + 4 * fq + v] = x2;
      }
    }
  __syncthreads();
  if (tid < 64) {
    const float v = (sl[tid] + sl[64 + tid]) + (sl[128 + tid] + sl[192 + tid]);
    float* st = a.stats + (size_t)stat_rep(blockIdx.x) * 2 * C;
    atomicAdd(st + (tid >> 5) * C + slab * 32 + (tid & 31), stat_val(v, blockIdx.x));
  }
}

// ------------------------------------------------------------------ WGRAD
// LDS: x patch [PR * PW pixels][32] | dz tile [rows * OW + 1 pixels][32], the last pixel zero.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void gconv_wgrad_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int slab = blockIdx.y;
  const int C = a.C, PW = a.PW;
  char* xs = smem;
  char* ds = smem + a.PR * PW * 64;
  const int zrow = a.rows * a.OW;  // the zero pixel of the dz tile

  f32x4 acc[2][2][9];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[i][j][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ds_read_b64_tr_b16: lane 4 q + p of a 16-lane group points at k-row q, channels 4 p .. + 3;
  // lane i of the group receives channel i of the four rows. Two reads, four rows apart, give
  // k = 8 fq .. + 7 of channel fr: this lane's rows are pixels 8 fq + kq and 8 fq + 4 + kq
  const int kq = (lane >> 2) & 3, cb = 8 * (lane & 3);  // cb: byte offset of its four channels
  auto frag = [&](const char* pa, const char* pb) {
    const v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)pa);
    const v4i16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)pb);
    const short8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
  };

  const int per = a.tpb;
  const int t0 = blockIdx.x * per, t1 = min(a.ntiles, t0 + per);
  for (int tile = t0; tile < t1; ++tile) {
    int n, r0, nr, ir0, ic0;
    tile_of(a, tile, n, r0, nr);
    patch_origin<0>(a, r0, ir0, ic0);
    const int npx = nr * a.OW;
    __syncthreads();
    stage_patch<false>(a, xs, n, ir0, ic0, slab);
    {
      // the tile's output pixels are contiguous in [N][OH][OW]
      const unsigned short* src = a.dz + (((size_t)n * a.OH + r0) * a.OW) * C + slab * 32;
      for (int it = tid; it < (zrow + 1) * 4; it += 256) {
        const int o = it >> 2, q = it & 3;
        uint4 v = {0u, 0u, 0u, 0u};
        if (o < npx) v = *reinterpret_cast<const uint4*>(src + (size_t)o * C + q * 8);
        *reinterpret_cast<uint4*>(ds + o * 64 + q * 16) = v;
      }
    }
    __syncthreads();
    for (int ks = wid; ks * 32 < npx; ks += 4) {
      const char* pd[2];
      const char* px[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int o = ks * 32 + 8 * fq + 4 * h + kq;
        const bool valid = o < npx;  // a pixel past the tile: dz row of zeros, x of pixel 0
        const int oc = valid ? o : 0;
        const int r = fast_div(oc, a.dOW), c = oc - r * a.OW;
        pd[h] = ds + (valid ? o : zrow) * 64 + cb;
        px[h] = xs + (r * PW + c) * a.s * 64 + cb;
      }
      bf16x8 dzf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) dzf[i] = frag(pd[0] + 32 * i, pd[1] + 32 * i);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int off = ((t / 3) * PW + t % 3) * 64;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const bf16x8 xf = frag(px[0] + off + 32 * j, px[1] + off + 32 * j);
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[i][j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, dzf[i], acc[i][j][t], 0, 0, 0);
        }
      }
    }
  }

  // ---- the four waves' sums, added in wave order: acc[i][j][t][v] = dW[co = 16 i + fr][t]
  // [ci = 16 j + 4 fq + v]
  float* redf = reinterpret_cast<float*>(smem);  // [32][9][32]
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wid != w) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          float4* p = reinterpret_cast<float4*>(redf + ((16 * i + fr) * 9 + t) * 32 + 16 * j + 4 * fq);
          const f32x4 v = acc[i][j][t];
          float4 o = {v[0], v[1], v[2], v[3]};
          if (w) {
            const float4 q = *p;
            o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w;
          }
          *p = o;
        }
  }
  __syncthreads();
  float4* dst = reinterpret_cast<float4*>(a.ws + ((size_t)slab * gridDim.x + blockIdx.x) * kPartial);
  for (int i = tid; i < kPartial / 4; i += 256) dst[i] = reinterpret_cast<const float4*>(redf)[i];
}

// dw += the slabs' diagonal blocks, partials added in split order. One thread per element of
// the master in [K][3][3][Cg] enumeration, stored in either layout.
__global__ __launch_bounds__(256)
void gconv_wgrad_finish_kernel(const float* __restrict__ ws, float* __restrict__ dw, int total,
                               int splits, int lg, int wkrsc, FastDiv d9) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int Cg = 1 << lg;
  const int cl = e & (Cg - 1), kt = e >> lg;
  const int k = fast_div(kt, d9), t = kt - 9 * k;
  const int slab = k >> 5, co = k & 31;
  const int ci = ((co >> lg) << lg) + cl;
  const float* p = ws + (size_t)slab * splits * kPartial + (co * 9 + t) * 32 + ci;
  float s = 0.f;
  for (int sp = 0; sp < splits; ++sp) s += p[(size_t)sp * kPartial];
  dw[wkrsc ? e : (k * Cg + cl) * 9 + t] += s;
}

// ------------------------------------------------------------------ host side
static int log2_cg(int cg) { return cg == 4 ? 2 : cg == 8 ? 3 : cg == 16 ? 4 : cg == 32 ? 5 : -1; }

// mode: 0 FWD, 1 DGRAD, 2 WGRAD. Returns false when the band does not fit LDS.
static bool plan(const ConvGeom* g, int groups, int mode, Args* a, size_t* lds) {
  const int Cg = g->C / groups;
  const bool d2 = mode == 1 && g->stride == 2;
  Args& r = *a;
  r.N = g->N; r.C = g->C;
  r.lg = log2_cg(Cg);
  r.Cp = (Cg + 7) / 8 * 8;
  r.dgrad = mode == 1;
  if (mode == 1) { r.IH = g->P; r.IW = g->Q; r.OH = g->H; r.OW = g->W; r.s = 1; }
  else { r.IH = g->H; r.IW = g->W; r.OH = g->P; r.OW = g->Q; r.s = g->stride; }
  // about 128 output pixels per tile, whole rows; stride-2 DGRAD: an even number of dx rows
  int rows = std::max(1, 128 / r.OW);
  if (d2) rows = std::max(2, rows & ~1);
  rows = std::min(rows, d2 ? (r.OH + 1) & ~1 : r.OH);
  r.rows = rows;
  r.bands = (r.OH + rows - 1) / rows;
  r.ntiles = r.N * r.bands;
  r.PR = d2 ? rows / 2 + 1 : (rows - 1) * r.s + 3;
  r.PW = d2 ? r.IW + 1 : r.IW + 2;
  r.plane = (r.PR * r.PW + 15) / 16 * 16;
  const int slabs = r.C / 32;
  if (mode == 2) {
    *lds = std::max((size_t)(r.PR * r.PW + rows * r.OW + 1) * 64, (size_t)kPartial * 4);
  } else {
    *lds = std::max((size_t)r.plane * 64, (size_t)288 * r.Cp * 2);
    // blocks: about 2048, and at most kStatRep along x (a block owns its statistics replica
    // in the deterministic build)
    const long long ts = (long long)r.ntiles * slabs;
    int tpb = (int)std::min<long long>(16, std::max<long long>(1, (ts + 2047) / 2048));
    r.tpb = std::max(tpb, (r.ntiles + 4095) / 4096);
  }
  r.dBands = make_fastdiv(r.bands);
  r.dPW = make_fastdiv(r.PW);
  r.dOW = make_fastdiv(r.OW);
  r.dJ0 = make_fastdiv(std::max(1, (r.OW + 1) / 2));
  r.dJ1 = make_fastdiv(std::max(1, r.OW / 2));
  return *lds <= (size_t)kMaxLds;
}

template <typename K>
static void allow_lds(K kernel) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
}

static bool served(const ConvGeom* g, int groups) {
  if (!g || groups < 1 || g->N < 1 || g->H < 1 || g->W < 1 || g->C < 32) return false;
  if (g->R != 3 || g->S != 3 || g->pad != 1 || (g->stride != 1 && g->stride != 2)) return false;
  if (g->C != g->K || g->C % 32 || g->C % groups) return false;
  const int Cg = g->C / groups;
  if (log2_cg(Cg) < 0 || g->Creal != Cg) return false;
  if (g->P != (g->H - 1) / g->stride + 1 || g->Q != (g->W - 1) / g->stride + 1) return false;
  if ((size_t)g->N * g->H * g->W * g->C >= 0x80000000ull) return false;
  Args a{};
  size_t lds;
  for (int mode = 0; mode < 3; ++mode)
    if (!plan(g, groups, mode, &a, &lds)) return false;
  return true;
}

}  // namespace gc
}  // namespace ddp_amd

using namespace ddp_amd;

extern "C" int ddp_gconv_ok(const ConvGeom* g, int groups) { return gc::served(g, groups) ? 1 : 0; }

extern "C" int ddp_gconv_fwd(const ConvGeom* g, int groups, const void* x, const void* wc,
                             const float* bias, void* z, float* stats, hipStream_t st) {
  if (!gc::served(g, groups) || !x || !wc || !z) return -1;
  gc::Args a{};
  size_t lds;
  gc::plan(g, groups, 0, &a, &lds);
  a.in = (const unsigned short*)x;
  a.out = (unsigned short*)z;
  a.wc = (const unsigned short*)wc;
  a.bias = bias;
  a.stats = stats;
  static bool attr = false;
  if (!attr) { gc::allow_lds(gc::gconv_kernel<0>); attr = true; }
  const dim3 grid((a.ntiles + a.tpb - 1) / a.tpb, a.C / 32);
  hipLaunchKernelGGL(gc::gconv_kernel<0>, grid, dim3(256), lds, st, a);
  const int e = (int)hipGetLastError();
  return e ? 2 + e : 1;
}

extern "C" int ddp_gconv_dgrad(const ConvGeom* g, int groups, const void* dz, const void* wc,
                               void* dx, hipStream_t st) {
  if (!gc::served(g, groups) || !dz || !wc || !dx) return -1;
  gc::Args a{};
  size_t lds;
  gc::plan(g, groups, 1, &a, &lds);
  a.in = (const unsigned short*)dz;
  a.out = (unsigned short*)dx;
  a.wc = (const unsigned short*)wc;
  static bool attr = false;
  if (!attr) { gc::allow_lds(gc::gconv_kernel<0>); gc::allow_lds(gc::gconv_kernel<1>); attr = true; }
  const dim3 grid((a.ntiles + a.tpb - 1) / a.tpb, a.C / 32);
  if (g->stride == 2) hipLaunchKernelGGL(gc::gconv_kernel<1>, grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL(gc::gconv_kernel<0>, grid, dim3(256), lds, st, a);
  const int e = (int)hipGetLastError();
  return e ? 2 + e : 1;
}

extern "C" int ddp_gconv_wgrad(const ConvGeom* g, int groups, const void* dz, const void* x,
                               float* dw, float* ws, size_t ws_elems, hipStream_t st) {
  if (!gc::served(g, groups) || !dz || !x || !dw || !ws) return -1;
  gc::Args a{};
  size_t lds;
  gc::plan(g, groups, 2, &a, &lds);
  const int slabs = a.C / 32;
  if (ws_elems < (size_t)slabs * gc::kPartial) return -2;
  // pixel split: about 1024 blocks, as many as the workspace holds
  int splits = std::max(1, std::min(a.ntiles, 1024 / slabs));
  splits = (int)std::min<size_t>(splits, ws_elems / ((size_t)slabs * gc::kPartial));
  a.tpb = (a.ntiles + splits - 1) / splits;
  splits = (a.ntiles + a.tpb - 1) / a.tpb;  // every block has at least one tile
  a.in = (const unsigned short*)x;
  a.dz = (const unsigned short*)dz;
  a.ws = ws;
  static bool attr = false;
  if (!attr) { gc::allow_lds(gc::gconv_wgrad_kernel); attr = true; }
  hipLaunchKernelGGL(gc::gconv_wgrad_kernel, dim3(splits, slabs), dim3(256), lds, st, a);
  int e = (int)hipGetLastError();
  if (e) return 2 + e;
  const int total = a.C * 9 << a.lg;
  hipLaunchKernelGGL(gc::gconv_wgrad_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, st,
                     ws, dw, total, splits, a.lg, g->wkrsc, make_fastdiv(9));
  e = (int)hipGetLastError();
  return e ? 2 + e : 1;
}
