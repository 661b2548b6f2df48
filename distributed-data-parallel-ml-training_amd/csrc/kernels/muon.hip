// Muon for gfx950 (optim/muon.py): the momentum of every orthogonalised tensor goes through five
// Newton-Schulz iterations, a chain of small and medium bf16 GEMMs per tensor per step.
//
//   muon_stage_kernel   G, m', d in registers; bf16(d) into the tensor's wide, zero-padded staging
//                       matrix X0 (transposed where the tensor is tall), sum d^2 per 8192-element
//                       chunk (api.h MuonStage).
//   muon_gemm_kernel    one grouped launch, D = bf16(alpha (A op B) + beta E) over a table of
//                       32 x 32 output tiles of every tensor (api.h MuonGemm): NT for A = X X^T,
//                       NN for B = b A + c A A and X' = a X + B X. Three launches per iteration.
//   (optim.hip)         the MUON items of sgd_pack_kernel read O = X5 and update p and m.
//
// The normalisation 1 / (|d| + 1e-7) is no pass of its own. X0 stays bf16(d), unscaled; the GEMMs
// of the first iteration sum the tensor's chunk partials in their block prologue (the fixed order
// of the trust ratios) and carry s0 = 1 / (sqrt(S) + 1e-7) in their scalars:
//     A0 = bf16((s0 * s0) * (X0 X0^T))                 alpha_pow = 2
//     B0 = bf16(c * (A0 A0) + b * A0)                  A0 is the normalised Gram matrix already
//     X1 = bf16(s0 * (B0 X0) + (a * s0) * X0)          alpha_pow = 1, beta_pow = 1
// which is the iteration on X0 s0 with the one bf16 rounding of the start taken on d, not on d s0.
//
// The GEMM's design. The outputs are small (m x m or m x n, m <= 512 for VGG) and the reductions
// long (n up to 4608 for X X^T), so a tile large enough to reuse operands from LDS would leave most
// of the 256 CUs idle: 512 x 512 in 64 x 64 tiles is 64 blocks. Here a block owns one 32 x 32 tile
// of D (256 tiles at m = 512, 136 with the symmetry) and its four waves SPLIT THE REDUCTION: wave w
// takes the 32-deep k-steps w, w + 4, ... of the whole tile on a 2 x 2 grid of
// v_mfma_f32_16x16x32_bf16 accumulators, and the four partial tiles meet in LDS, added in the
// fixed order ((w0 + w1) + w2) + w3: a split reduction with no workspace, no second launch and no
// float atomics. The split is inside the block rather than across blocks because a finish over
// fp32 slabs in memory would cost more than these GEMMs themselves at m = 128.
//   * [row][k] operands (A of both forms, B of NT) are not staged at all: the MFMA fragment of a
//     k-contiguous operand, row lane % 16, k = 8 (lane / 16) .. + 7, is one 16-byte global load
//     per lane, and the wave that loads a fragment is its only reader.
//   * B of the NN form is [k][col]: each wave copies its own 32 x 32 k-step tile into LDS as it
//     lies in memory (two 16-byte chunks per lane, rows 80 bytes apart) and reads the fragments
//     with ds_read_b64_tr_b16, the transposing read conv_igemm.hip's WGRAD uses. The tile belongs
//     to its wave, so the k-loop takes no block barrier.
//   * Both loops fetch the next k-step's operands into registers before this step's MFMAs.
//   * Operands are swapped in the MFMA (D^T = B^T A^T) so a lane owns one row and four consecutive
//     columns: 16-byte LDS stores of the partial tiles, 8-byte bf16 stores of D.
//   * X X^T and A A are symmetric: only tiles on or above the diagonal are in the table, and an
//     off-diagonal tile is stored a second time transposed (item flag), so the mirrored half
//     holds the same bits.
//   * Every dimension is a multiple of 32, so no load or store is ever predicated; elements of D
//     in the padding are stored as +0 whatever the arithmetic gave (a non-finite step cannot
//     poison the padding of the buffers the next step reads).
#include <type_traits>

#include "common.h"
#include "api.h"

namespace ddp_amd {

typedef short mu_v4i16 __attribute__((ext_vector_type(4)));
typedef short mu_v8i16 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) mu_v4i16 mu_lds_v4i16;

constexpr int kMuChunk = 8192;  // elements per stage block (optim/sgd.py FusedSGD.CHUNK)
constexpr int kMuTile = 32;     // D tile edge, k-step depth and padding granularity
constexpr int kMuPitch = 40;    // bf16 per row of a wave's B tile in LDS (80 bytes: 16-byte chunks
                                // stay aligned, rows 4 apart fall into different banks)

struct MuNoClip {};
template <bool GUARD>
struct MuonStageArgs : std::conditional_t<GUARD, ClipArgs, MuNoClip> {
  const int4* items;
  const MuonTensor* tensors;
  const float* g;
  const float* m;
  float mu, grad_scale;
  int nesterov;
  float* partial;
};

// bf16(d) of tensor element ``el`` into the staging matrix.
__device__ __forceinline__ size_t mu_index(const MuonTensor& t, unsigned r, unsigned c) {
  return t.transposed ? (size_t)c * t.pitch + r : (size_t)r * t.pitch + c;
}

template <bool GUARD>
__global__ __launch_bounds__(256) void muon_stage_kernel(MuonStageArgs<GUARD> a) {
  const int4 it = a.items[blockIdx.x];
  const MuonTensor t = a.tensors[it.w];
  const size_t off = (size_t)(unsigned)it.x;
  const int cnt = it.y, n4 = cnt >> 2;
  const int tid = threadIdx.x;
  float gs = a.grad_scale;
  if constexpr (GUARD) gs *= clip_block(a).c;
  const float* __restrict__ g = a.g + off;
  const float* __restrict__ m = a.m + off;
  const unsigned el0 = (unsigned)(off - (size_t)t.p_offset);  // the chunk's first tensor element
  const unsigned rest = (unsigned)t.rest;
  constexpr int kIter = kMuChunk / (256 * 4);
  float4 gv[kIter], mv[kIter];
#pragma unroll
  for (int j = 0; j < kIter; ++j) {  // every 16-byte load of the chunk in flight at once
    const int i = tid + 256 * j;
    if (i < n4) {
      gv[j] = reinterpret_cast<const float4*>(g)[i];
      mv[j] = reinterpret_cast<const float4*>(m)[i];
    }
  }
  float sd = 0.f;  // one serial fma chain per thread: 4 * kIter (+ 1 tail) terms
#pragma unroll
  for (int j = 0; j < kIter; ++j) {
    const int i = tid + 256 * j;
    if (i < n4) {
      const float* gg = &gv[j].x;
      float* mm = &mv[j].x;
      unsigned short h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = muon_dir(gg[e], mm[e], gs, a.mu, a.nesterov);
        sd = __builtin_fmaf(d, d, sd);
        h[e] = f2bf(d);
      }
      const unsigned el = el0 + 4u * (unsigned)i;
      unsigned r = el / rest, c = el - r * rest;
      if (!t.transposed && c + 3 < rest && (c & 3) == 0) {  // four of one row, 8-byte aligned
        *reinterpret_cast<uint2*>(t.x + (size_t)r * t.pitch + c) =
            make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t.x[mu_index(t, r, c)] = h[e];
          if (++c == rest) { c = 0; ++r; }
        }
      }
    }
  }
  const int tl = (n4 << 2) + tid;  // scalar tail: numel not a multiple of 4
  if (tl < cnt) {
    float mt = m[tl];
    const float d = muon_dir(g[tl], mt, gs, a.mu, a.nesterov);
    sd = __builtin_fmaf(d, d, sd);
    const unsigned el = el0 + (unsigned)tl, r = el / rest;
    t.x[mu_index(t, r, el - r * rest)] = f2bf(d);
  }
  sd = wave_sum(sd);
  __shared__ float s_w[4];  // per wave
  if ((tid & 63) == 0) s_w[tid >> 6] = sd;
  __syncthreads();
  if (tid == 0) a.partial[it.z] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// s0^pow folded into a scalar: one fp32 product per power.
__device__ __forceinline__ float mu_fold(float v, float s0, int pow) {
  if (pow >= 1) v *= s0;
  if (pow >= 2) v *= s0;
  return v;
}

template <bool NN>
__global__ __launch_bounds__(256) void muon_gemm_kernel(const int4* __restrict__ items,
                                                        const MuonGemm* __restrict__ descs,
                                                        const float* __restrict__ partial) {
  __shared__ float red[4][kMuTile * kMuTile];                       // the four waves' partial tiles
  __shared__ unsigned short bt[NN ? 4 : 1][kMuTile * kMuPitch];     // NN: a wave's B k-step tile
  __shared__ float s_s0;
  const int4 it = items[blockIdx.x];
  const MuonGemm g = descs[it.x];
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int fr = lane & 15, fq = lane >> 4;

  float s0 = 1.f;
  if (g.norm_n > 0) {  // (uniform over the block)
    if (tid < 64) {
      float s = 0.f;
      for (int c = tid; c < g.norm_n; c += 64) s += partial[g.norm0 + c];
      s = wave_sum(s);
      if (tid == 0) s_s0 = 1.f / (sqrtf(s) + 1e-7f);
    }
    __syncthreads();
    s0 = s_s0;
  }
  const float alpha = mu_fold(g.alpha, s0, g.alpha_pow), beta = mu_fold(g.beta, s0, g.beta_pow);

  const int row0 = it.y * kMuTile, col0 = it.z * kMuTile;
  // fragment i of A: rows row0 + 16 i + fr, k = 8 fq .. + 7 of the k-step
  const unsigned short* pa = g.a + (size_t)(row0 + fr) * g.lda + 8 * fq;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Both loops keep the next k-step's global loads in flight during the MFMAs of this one.
  bf16x8 fa[2], na[2];
  if constexpr (!NN) {
    const unsigned short* pb = g.b + (size_t)(col0 + fr) * g.ldb + 8 * fq;
    bf16x8 fb[2], nb[2];
    auto fetch = [&](int s) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        na[i] = __builtin_bit_cast(bf16x8, ld8(pa + (size_t)(16 * i) * g.lda + s * kMuTile));
        nb[i] = __builtin_bit_cast(bf16x8, ld8(pb + (size_t)(16 * i) * g.ldb + s * kMuTile));
      }
    };
    if (wid < g.ksteps) fetch(wid);
    for (int s = wid; s < g.ksteps; s += 4) {
#pragma unroll
      for (int i = 0; i < 2; ++i) { fa[i] = na[i]; fb[i] = nb[i]; }
      if (s + 4 < g.ksteps) fetch(s + 4);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    }
  } else {
    // the wave's B tile: rows k0 .. k0 + 31, columns col0 .. col0 + 31, four 16-byte chunks per
    // row; lane l copies chunk l & 3 of rows l >> 2 and 16 + (l >> 2)
    const unsigned short* pb = g.b + (size_t)(lane >> 2) * g.ldb + col0 + 8 * (lane & 3);
    unsigned short* wt = &bt[wid][(lane >> 2) * kMuPitch + 8 * (lane & 3)];
    // ds_read_b64_tr_b16: lane 4 q + p of a 16-lane group points at row q, columns 4 p .. + 3 of a
    // 4 x 16 block; lane i of the group receives column i of the four rows. Two reads, four rows
    // apart, give k = 8 fq .. + 7 of column 16 j + fr.
    const unsigned short* rd = &bt[wid][(8 * fq + ((lane >> 2) & 3)) * kMuPitch + 4 * (lane & 3)];
    // bt[wid] is written and read by this wave alone, and a wave's LDS operations complete in
    // order: no block barrier. The fence waits for the wave's outstanding LDS operations and the
    // wave barrier keeps the compiler from moving LDS accesses of other lanes' data across it.
    auto wave_sync = [] {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
      __builtin_amdgcn_wave_barrier();
    };
    u16x8 b0, b1;
    auto fetch = [&](int s) {
      const int k0 = s * kMuTile;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        na[i] = __builtin_bit_cast(bf16x8, ld8(pa + (size_t)(16 * i) * g.lda + k0));
      b0 = ld8(pb + (size_t)k0 * g.ldb);
      b1 = ld8(pb + (size_t)(k0 + 16) * g.ldb);
    };
    if (wid < g.ksteps) fetch(wid);
    for (int s = wid; s < g.ksteps; s += 4) {
      wave_sync();  // the fragment reads of the step before are done
      st8(wt, b0);
      st8(wt + 16 * kMuPitch, b1);
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = na[i];
      if (s + 4 < g.ksteps) fetch(s + 4);
      wave_sync();
      bf16x8 fb[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const mu_v4i16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mu_lds_v4i16*)(rd + 16 * j));
        const mu_v4i16 hi =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((mu_lds_v4i16*)(rd + 16 * j + 4 * kMuPitch));
        const mu_v8i16 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        fb[j] = __builtin_bit_cast(bf16x8, v);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    }
  }

  // the lane owns rows 16 i + fr, columns 16 j + 4 fq .. + 3 of its wave's partial tile
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      *reinterpret_cast<f32x4*>(&red[wid][(16 * i + fr) * kMuTile + 16 * j + 4 * fq]) = acc[i][j];
  __syncthreads();

  // finish: thread t owns row t >> 3, columns 4 (t & 7) .. + 3
  const int r = tid >> 3, c = 4 * (tid & 7);
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int x = r * kMuTile + c + e;
    v[e] = alpha * (((red[0][x] + red[1][x]) + red[2][x]) + red[3][x]);
  }
  const size_t di = (size_t)(row0 + r) * g.ldd + col0 + c;
  if (g.e) {
    const uint2 ev = *reinterpret_cast<const uint2*>(g.e + di);
    v[0] = __builtin_fmaf(beta, bf2f((unsigned short)(ev.x & 0xffffu)), v[0]);
    v[1] = __builtin_fmaf(beta, bf2f((unsigned short)(ev.x >> 16)), v[1]);
    v[2] = __builtin_fmaf(beta, bf2f((unsigned short)(ev.y & 0xffffu)), v[2]);
    v[3] = __builtin_fmaf(beta, bf2f((unsigned short)(ev.y >> 16)), v[3]);
  }
  unsigned short h[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    h[e] = (row0 + r < g.rows && col0 + c + e < g.cols) ? f2bf(v[e]) : (unsigned short)0;
  *reinterpret_cast<uint2*>(g.d + di) =
      make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
  if (it.w && it.y != it.z) {  // the mirrored tile of a symmetric product (rows == cols)
#pragma unroll
    for (int e = 0; e < 4; ++e) g.d[(size_t)(col0 + c + e) * g.ldd + row0 + r] = h[e];
  }
}

template <bool GUARD>
static int launch_muon_stage(const MuonStage& s, hipStream_t st) {
  MuonStageArgs<GUARD> a{};
  if constexpr (GUARD) static_cast<ClipArgs&>(a) = s.clip;
  a.items = s.items; a.tensors = s.tensors; a.g = s.g; a.m = s.m; a.mu = s.mu;
  a.grad_scale = s.grad_scale; a.nesterov = s.nesterov; a.partial = s.partial;
  hipLaunchKernelGGL(muon_stage_kernel<GUARD>, dim3(s.n_items), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace ddp_amd

using namespace ddp_amd;

extern "C" int ddp_muon_stage(const MuonStage* s, hipStream_t st) {
  if (s->n_items <= 0) return 0;
  if (!s->items || !s->tensors || !s->g || !s->m || !s->partial) return -1;
  const bool guard = s->clip.partial;
  if (guard && s->clip.n_chunks < 0) return -1;
  return (guard ? launch_muon_stage<true> : launch_muon_stage<false>)(*s, st);
}

extern "C" int ddp_muon_gemm(const void* items, int n_items, const MuonGemm* descs,
                             const float* partial, int nn, hipStream_t st) {
  if (n_items <= 0) return 0;
  if (!items || !descs) return -1;
  if (nn)
    hipLaunchKernelGGL(muon_gemm_kernel<true>, dim3(n_items), dim3(256), 0, st,
                       (const int4*)items, descs, partial);
  else
    hipLaunchKernelGGL(muon_gemm_kernel<false>, dim3(n_items), dim3(256), 0, st,
                       (const int4*)items, descs, partial);
  return (int)hipGetLastError();
}
