// Wide classifier head for gfx950: Linear(F, J) with 16 < J <= 128 outputs fused with the mean
// softmax cross-entropy, on v_mfma_f32_16x16x32_bf16 (CIFAR-100's Linear(512, 100)).
//
// linear_ce.hip keeps one row's logits in a wave's registers (kMaxJ = 16 accumulators, one wave
// reduction each); that design does not stretch. Here the logits of 16 rows are one MFMA tile row:
//
// fwd : one launch, a 256-thread block owns 16 batch rows and all JP = ceil16(J) logit columns.
//       The work is split over the four waves by COLUMN TILES (wave w: tiles w and w + 4), not by
//       k-range: every wave then runs the whole k-loop on its own accumulators, no partial tile
//       is ever reduced, and the summation order of a logit does not depend on the wave count.
//       A = the rows' bf16 features, one 16-B global load per lane and k-step (row lane & 15,
//       k 8 (lane >> 4) ..; dead rows of the last block read the last live row).
//       B = W, read from the fp32 master in 32-deep k-chunks by the whole block (coalesced
//       float4 rows), rounded to bf16 (f2bf, RNE) into a two-chunk LDS ring [JP][32] with the
//       columns >= J written as zeros; a lane's fragment is one 16-B LDS read (a tile's 64 lanes
//       read 1 KB contiguous: no bank conflict). One barrier per chunk: chunk c + 1 is fetched
//       into registers while chunk c feeds the MFMAs, and stored into the other ring slot.
//       The 16 x JP fp32 tile is parked in LDS; the softmax epilogue gives each row to one
//       16-lane DPP row (lane l owns columns l, l + 16, ..): bias, max / first argmax, sum of
//       exponentials, loss term and dlogits in softmax_ce_kernel's expressions; row reductions
//       are four DPP steps. One block sum of the 16 loss terms / hits, one atomic each.
// bwd : one launch, block ranges as linear_bwd_kernel: [0, ndx) dx tiles, then dW tiles.
//       dx  (16 rows x 64 features per block, a 16 x 16 tile per wave): dl and the W tile are
//           rounded to bf16 and TRANSPOSED in staging (W[j][f] -> [f][j]) so that K = ceil32(J)
//           is contiguous for both fragments; columns / rows beyond J, B are zeros. g is applied
//           to the fp32 accumulator, the store is bf16 (8 B per lane).
//       dW  (16 classes x 64 features per block, the WHOLE batch as K in 32-row chunks, zero rows
//           past B): dl^T and x^T are staged like the forward's ring. The block owns its dW
//           elements: plain load-add-store, no float atomics, so the release and the
//           deterministic build run the same order. The feature-tile-0 blocks also own db: the
//           unrounded fp32 dl values a thread stages are summed on the way (16 partial sums per
//           class, met in LDS in a fixed order).
// Neither kernel allocates or synchronises with the host: both can be captured.
#include "common.h"
#include "api.h"
#include "linear_wide.h"

namespace ddp_amd {

constexpr int kWfK = 32;                // k-chunk depth: one MFMA k-step
constexpr int kWfLd = kWideMaxJ + 4;    // logit tile row stride (floats; rows stay 16-B aligned)
constexpr int kWbLd = kWideMaxJ + 8;    // dx staging row stride (bf16; 272 B, 16-B aligned)
constexpr int kWbKd = 32 + 8;           // dW staging row stride (bf16; 80 B, 16-B aligned)
constexpr int kWbFt = 64;               // features per backward block (16 per wave)

__device__ __forceinline__ bf16x8 lds_frag(const unsigned short* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
  return (unsigned)f2bf(lo) | ((unsigned)f2bf(hi) << 16);
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
// max with the lowest index among equals over the 16 lanes of a DPP row, result in every lane
template <int CTRL>
__device__ __forceinline__ void argmax_step(float& mx, int& arg) {
  const float om = dpp_f<CTRL>(mx);
  const int oa = dpp_i<CTRL>(arg);
  if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }
}

// SOFT: ``soft`` = one SoftTarget, passed to the soft instantiation only (linear_ce.hip's rule).
template <bool SOFT, class... Soft>
__global__ __launch_bounds__(256) void linear_wide_fwd_kernel(
    const unsigned short* __restrict__ x, const float* __restrict__ W, const float* __restrict__ b,
    const long long* __restrict__ labels, int B, int F, int J, float inv_b, float* logits_out,
    float* dlogits, float* loss_sum, int* correct, float* loss_acc, Soft... soft) {
  static_assert(sizeof...(Soft) == (SOFT ? 1 : 0), "SoftTarget goes to the soft instantiation");
  __shared__ __attribute__((aligned(16))) unsigned short ring[2][kWideMaxJ * kWfK];
  __shared__ __attribute__((aligned(16))) float tile[16][kWfLd];
  __shared__ float lrow[16];
  __shared__ int hrow[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;  // fragment row / column index and k-group
  const int NT = (J + 15) >> 4;              // column tiles, <= 8
  const int row0 = blockIdx.x * 16;
  const int nch = F / kWfK;
  const int nv = NT * 16 * (kWfK / 4);       // float4s of one W chunk [JP][32]

  // W chunk c -> registers: float4 e of the chunk is W[e / 8][32 c + 4 (e % 8) ..]
  float4 wv[4];
  auto fetch = [&](int c) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i, r = e >> 3;
      wv[i] = (e < nv && r < J)
                  ? *reinterpret_cast<const float4*>(W + (size_t)r * F + c * kWfK + 4 * (e & 7))
                  : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      if (e < nv)
        *reinterpret_cast<uint2*>(&ring[buf][4 * e]) =
            make_uint2(pack2(wv[i].x, wv[i].y), pack2(wv[i].z, wv[i].w));
    }
  };
  const unsigned short* xa = x + (size_t)min(row0 + fr, B - 1) * F + 8 * fq;

  f32x4 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  fetch(0);
  u16x8 xn = ld8(xa);
  for (int c = 0; c < nch; ++c) {
    stash(c & 1);
    const bf16x8 fa = __builtin_bit_cast(bf16x8, xn);
    __syncthreads();  // slot c & 1 is complete; every wave is done with slot (c + 1) & 1
    if (c + 1 < nch) {
      fetch(c + 1);
      xn = ld8(xa + (c + 1) * kWfK);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int ct = wid + 4 * t;
      if (ct < NT) {
        const bf16x8 fb = lds_frag(&ring[c & 1][(ct * 16 + fr) * kWfK + 8 * fq]);
        // operands swapped as in conv_igemm.hip: the lane owns row fr, columns 4 fq .. + 3
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, fa, acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int ct = wid + 4 * t;
    if (ct < NT) *reinterpret_cast<f32x4*>(&tile[fr][ct * 16 + 4 * fq]) = acc[t];
  }
  __syncthreads();

  // ---- softmax epilogue: row r = one DPP row of 16 lanes, lane l owns columns l + 16 t
  const int r = tid >> 4, l = tid & 15;
  const bool live = row0 + r < B;
  const int row = live ? row0 + r : B - 1;  // dead rows recompute the last row, store nothing
  float z[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int col = l + 16 * t;
    z[t] = col < J ? tile[r][col] + (b ? b[col] : 0.f) : 0.f;
    if (live && logits_out && col < J) logits_out[(size_t)row * J + col] = z[t];
  }
  if (!labels) return;  // logits only (uniform over the block)
  float mx = z[0];      // J > 16: every lane owns column l
  int arg = l;
#pragma unroll
  for (int t = 1; t < 8; ++t)
    if (l + 16 * t < J && z[t] > mx) { mx = z[t]; arg = l + 16 * t; }
  argmax_step<0xB1>(mx, arg);
  argmax_step<0x4E>(mx, arg);
  argmax_step<0x141>(mx, arg);
  argmax_step<0x140>(mx, arg);
  float se = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t)
    if (l + 16 * t < J) se += __expf(z[t] - mx);
  se = dpp_sum16(se);
  const float lse = mx + __logf(se);
  const int y = (int)labels[row];
  if (live && dlogits) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int col = l + 16 * t;
      if (col < J) {
        const float p = __expf(z[t] - lse);
        float tg = col == y ? 1.f : 0.f;
        if constexpr (SOFT) tg = SoftRow(only(soft...), row, y, J).target(col, y);
        dlogits[(size_t)row * J + col] = (p - tg) * inv_b;
      }
    }
  }
  // the label's logit: its owner contributes it, the other 15 lanes +0 (an exact sum)
  float ly = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t)
    if (l + 16 * t == y && y < J) ly = z[t];
  ly = dpp_sum16(ly);
  if constexpr (SOFT) {
    const SoftRow sr(only(soft...), row, y, J);
    float lyb = 0.f, sz = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      if (l + 16 * t == sr.yb && sr.yb < J) lyb = z[t];
      if (l + 16 * t < J) sz += z[t];
    }
    lyb = dpp_sum16(lyb);
    sz = dpp_sum16(sz);
    ly = sr.term(ly, lyb, sz);
  }
  if (l == 0) {
    lrow[r] = live ? (lse - ly) * inv_b : 0.f;
    hrow[r] = (live && arg == y) ? 1 : 0;
  }
  __syncthreads();
  if (tid == 0) {
    float ls = 0.f;
    int h = 0;
    for (int k = 0; k < 16; ++k) { ls += lrow[k]; h += hrow[k]; }
    if (loss_sum) atomicAdd(loss_sum, ls);
    if (loss_acc) atomicAdd(loss_acc, ls);  // running sum across steps
    if (correct) atomicAdd(correct, h);
  }
}

// dx tile: rows 16 rb .., features 64 fx .. (wave w: 16 w ..), K = ceil32(J)
__device__ __forceinline__ void wide_dx_block(unsigned short* smem, const float* __restrict__ dl,
                                              const float* __restrict__ W, int B, int F, int J,
                                              float g, unsigned short* dx, int rb, int fx) {
  unsigned short* As = smem;               // [16][kWbLd] bf16(dl), zeros beyond B / J
  unsigned short* Ws = smem + 16 * kWbLd;  // [64][kWbLd] bf16(W)^T, zeros beyond J / F
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int KP = (J + 31) & ~31;
  const int row0 = rb * 16, f0 = fx * kWbFt;
  {
    const int r = tid >> 4, c = tid & 15;
    for (int col = c; col < KP; col += 16)
      As[r * kWbLd + col] =
          f2bf((row0 + r < B && col < J) ? dl[(size_t)(row0 + r) * J + col] : 0.f);
    // two class rows x four features per thread: a (j, j + 1) pair is one 4-B LDS store
    const int f4 = 4 * (tid & 15), jp = 2 * (tid >> 4);
    const bool fok = f0 + f4 < F;
    for (int j = jp; j < KP; j += 32) {
      float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f), w1 = w0;
      if (fok && j < J) w0 = *reinterpret_cast<const float4*>(W + (size_t)j * F + f0 + f4);
      if (fok && j + 1 < J) w1 = *reinterpret_cast<const float4*>(W + (size_t)(j + 1) * F + f0 + f4);
      *reinterpret_cast<unsigned*>(&Ws[(f4 + 0) * kWbLd + j]) = pack2(w0.x, w1.x);
      *reinterpret_cast<unsigned*>(&Ws[(f4 + 1) * kWbLd + j]) = pack2(w0.y, w1.y);
      *reinterpret_cast<unsigned*>(&Ws[(f4 + 2) * kWbLd + j]) = pack2(w0.z, w1.z);
      *reinterpret_cast<unsigned*>(&Ws[(f4 + 3) * kWbLd + j]) = pack2(w0.w, w1.w);
    }
  }
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int kk = 0; kk < KP; kk += 32) {
    const bf16x8 fa = lds_frag(As + fr * kWbLd + kk + 8 * fq);
    const bf16x8 fb = lds_frag(Ws + (wid * 16 + fr) * kWbLd + kk + 8 * fq);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, fa, acc, 0, 0, 0);
  }
  // the lane owns row fr, features 16 wid + 4 fq .. + 3 of the tile
  const int row = row0 + fr, f = f0 + wid * 16 + 4 * fq;
  if (row < B && f < F)
    *reinterpret_cast<uint2*>(dx + (size_t)row * F + f) =
        make_uint2(pack2(acc[0] * g, acc[1] * g), pack2(acc[2] * g, acc[3] * g));
}

// dW tile: classes 16 jt .., features 64 fx .. (wave w: 16 w ..), K = the whole batch; + db
__device__ __forceinline__ void wide_dw_block(unsigned short* smem, float (*dbp)[16],
                                              const float* __restrict__ dl,
                                              const unsigned short* __restrict__ x, int B, int F,
                                              int J, float g, float* dW, float* db, int jt,
                                              int fx) {
  constexpr int SLOT = (16 + kWbFt) * kWbKd;  // [16][kWbKd] bf16(dl)^T, then [64][kWbKd] x^T
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int j0 = jt * 16, f0 = fx * kWbFt;
  const int nch = (B + 31) >> 5;
  // staging roles: dl[b0 + bs (+ 16)][j0 + dj] and 8 features of x[b0 + xb]
  const int dj = tid & 15, bs = tid >> 4;
  const int xb = tid >> 3, xf = 8 * (tid & 7);
  const bool jok = j0 + dj < J, xok = f0 + xf < F;
  float dv[2], dbsum = 0.f;
  uint4 xv;  // 8 bf16 features of one batch row
  auto fetch = [&](int c) {
    const int b0 = c * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rb = b0 + bs + 16 * i;
      dv[i] = (jok && rb < B) ? dl[(size_t)rb * J + j0 + dj] : 0.f;
      dbsum += dv[i];
    }
    xv = (xok && b0 + xb < B)
             ? *reinterpret_cast<const uint4*>(x + (size_t)(b0 + xb) * F + f0 + xf)
             : make_uint4(0u, 0u, 0u, 0u);
  };
  auto stash = [&](int buf) {
    unsigned short* Dt = smem + buf * SLOT;
    unsigned short* Xt = Dt + 16 * kWbKd;
#pragma unroll
    for (int i = 0; i < 2; ++i) Dt[dj * kWbKd + bs + 16 * i] = f2bf(dv[i]);
    unsigned short* xt = Xt + xf * kWbKd + xb;
    xt[0 * kWbKd] = (unsigned short)xv.x; xt[1 * kWbKd] = (unsigned short)(xv.x >> 16);
    xt[2 * kWbKd] = (unsigned short)xv.y; xt[3 * kWbKd] = (unsigned short)(xv.y >> 16);
    xt[4 * kWbKd] = (unsigned short)xv.z; xt[5 * kWbKd] = (unsigned short)(xv.z >> 16);
    xt[6 * kWbKd] = (unsigned short)xv.w; xt[7 * kWbKd] = (unsigned short)(xv.w >> 16);
  };
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  fetch(0);
  for (int c = 0; c < nch; ++c) {
    stash(c & 1);
    __syncthreads();  // slot c & 1 is complete; every wave is done with slot (c + 1) & 1
    if (c + 1 < nch) fetch(c + 1);
    const unsigned short* Dt = smem + (c & 1) * SLOT;
    const unsigned short* Xt = Dt + 16 * kWbKd;
    const bf16x8 fa = lds_frag(Dt + fr * kWbKd + 8 * fq);
    const bf16x8 fb = lds_frag(Xt + (wid * 16 + fr) * kWbKd + 8 * fq);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, fa, acc, 0, 0, 0);
  }
  // the lane owns class j0 + fr, features 16 wid + 4 fq .. + 3: this block alone adds to them
  const int j = j0 + fr, f = f0 + wid * 16 + 4 * fq;
  if (j < J && f < F) {
    float4* p = reinterpret_cast<float4*>(dW + (size_t)j * F + f);
    float4 o = *p;
    o.x += acc[0] * g; o.y += acc[1] * g; o.z += acc[2] * g; o.w += acc[3] * g;
    *p = o;
  }
  if (fx == 0 && db) {  // (uniform over the block)
    dbp[bs][dj] = dbsum;
    __syncthreads();
    if (tid < 16 && j0 + tid < J) {
      float s = 0.f;
      for (int k = 0; k < 16; ++k) s += dbp[k][tid];
      db[j0 + tid] += s * g;
    }
  }
}

// dx and dW / db in ONE launch: blocks [0, ndx) are dx tiles (feature tile fastest), the rest
// dW tiles.
__global__ __launch_bounds__(256) void linear_wide_bwd_kernel(
    const float* __restrict__ dl, const unsigned short* __restrict__ x,
    const float* __restrict__ W, int B, int F, int J, const float* gscale, unsigned short* dx,
    float* dW, float* db, int ndx, int nfx) {
  __shared__ __attribute__((aligned(16))) unsigned short smem[(16 + kWbFt) * kWbLd];
  __shared__ float dbp[16][16];
  static_assert(2 * (16 + kWbFt) * kWbKd <= (16 + kWbFt) * kWbLd, "the dW ring fits the dx tiles");
  const float g = gscale ? *gscale : 1.f;
  const int bid = blockIdx.x;
  if (bid < ndx) {
    wide_dx_block(smem, dl, W, B, F, J, g, dx, bid / nfx, bid % nfx);
  } else {
    const int t = bid - ndx;
    wide_dw_block(smem, dbp, dl, x, B, F, J, g, dW, db, t / nfx, t % nfx);
  }
}

static bool wide_ok(int B, int F, int J) {
  return J > 16 && J <= kWideMaxJ && F > 0 && F % kWfK == 0 && F <= kMaxHeadF && B >= 1;
}

int linear_wide_fwd(const void* x, const float* W, const float* b, const long long* labels, int B,
                    int F, int J, float* logits, float* dlogits, float* loss_sum, int* correct,
                    float* loss_acc, const SoftTarget* soft, hipStream_t st) {
  if (!wide_ok(B, F, J) || !x || !W) return -1;
  const dim3 grid((B + 15) / 16);
  if (soft)
    hipLaunchKernelGGL((linear_wide_fwd_kernel<true, SoftTarget>), grid, dim3(256), 0, st,
                       (const unsigned short*)x, W, b, labels, B, F, J, 1.f / (float)B, logits,
                       dlogits, loss_sum, correct, loss_acc, *soft);
  else
    hipLaunchKernelGGL((linear_wide_fwd_kernel<false>), grid, dim3(256), 0, st,
                       (const unsigned short*)x, W, b, labels, B, F, J, 1.f / (float)B, logits,
                       dlogits, loss_sum, correct, loss_acc);
  return (int)hipGetLastError();
}

int linear_wide_bwd(const float* dlogits, const void* x, const float* W, int B, int F, int J,
                    const float* gscale, void* dx, float* dW, float* db, hipStream_t st) {
  if (!wide_ok(B, F, J) || !dlogits || !x || !W || !dW) return -1;
  const int nfx = (F + kWbFt - 1) / kWbFt;
  const int ndx = dx ? ((B + 15) / 16) * nfx : 0;
  const int ndw = ((J + 15) / 16) * nfx;
  hipLaunchKernelGGL(linear_wide_bwd_kernel, dim3(ndx + ndw), dim3(256), 0, st, dlogits,
                     (const unsigned short*)x, W, B, F, J, gscale, (unsigned short*)dx, dW, db,
                     ndx, nfx);
  return (int)hipGetLastError();
}

}  // namespace ddp_amd
