// Optimizer and weight-layout kernels for gfx950.
//
// Reference parity: optim.SGD(lr=0.1, momentum=0.9, weight_decay=1e-4) over the 34 VGG-11
// parameter tensors (part1/main.py:124-125, step at :77) — SURVEY.md §2.B N2g. Here ONE
// launch updates the whole flat fp32 parameter arena (all tensors are views into it):
//     d = g * grad_scale + wd * p ; buf = momentum * buf + d ; d = nesterov ? d + momentum*buf : buf
//     p -= lr * d
// A zero-initialised momentum buffer reproduces torch's "buf = clone(d) on the first step"
// exactly (momentum * 0 + d == d), so the kernel needs no first-step flag (graph friendly).
// With AdamW (optim/adamw.py, api.h AdamArgs) the same launch applies Adam with decoupled weight
// decay instead: the momentum arena holds the first moment, one more arena the second, and the
// bias corrections of the step come from a device table next to the learning rate's. With LAMB
// (optim/lamb.py, api.h LambArgs) a norms launch over p, g, m, v runs in front (lamb_norms_kernel)
// and the same launch scales every adapted tensor's AdamW-style update by |w| / |update|.
//
// pack_conv_weights re-lays the fp32 master weights (PyTorch [K][C][R][S]) into the two bf16
// MFMA operand layouts used by conv_igemm.hip: Wc [K][R][S][Cpad] (fwd) and Wt [C][R][S][K]
// (dgrad); all conv tensors of the model in one launch (blockIdx.y = tensor).
#include <type_traits>

#include "common.h"
#include "api.h"

namespace ddp_amd {

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ buf, size_t n, float lr,
                                                  float momentum, float wd, float grad_scale,
                                                  int nesterov, const LrSched* sched) {
  lr = sched_lr_block(sched, lr);
  const size_t n4 = n / 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 bv = reinterpret_cast<float4*>(buf)[i];
    float* pp = &pv.x;
    const float* gg = &gv.x;
    float* bb = &bv.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      pp[e] = sgd_update1(pp[e], gg[e], bb[e], lr, momentum, wd, grad_scale, nesterov);
    }
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(buf)[i] = bv;
  }
  // scalar tail
  for (size_t i = n4 * 4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    p[i] = sgd_update1(p[i], g[i], buf[i], lr, momentum, wd, grad_scale, nesterov);
  }
}

constexpr int kMaxPack = 64;
struct PackTable {
  PackDesc d[kMaxPack];
  int n;
};

__device__ __forceinline__ size_t master_index(const PackDesc& d, int k, int c, int r, int s) {
  return d.krsc ? (((size_t)k * d.R + r) * d.S + s) * d.Cr + c
                : (((size_t)k * d.Cr + c) * d.R + r) * d.S + s;
}

// Element i of Wc [k][r][s][c] from the master: bf16(p[k][c][r][s]), +0 in the padded channels.
// Index: the index type of the caller's loop (its divisions stay as wide as they were).
template <class Index>
__device__ __forceinline__ unsigned short wc_from_master(const PackDesc& d, Index i) {
  const int c = (int)(i % d.C);
  const Index t1 = i / d.C;
  const int s = (int)(t1 % d.S);
  const Index t2 = t1 / d.S;
  const int r = (int)(t2 % d.R);
  const int k = (int)(t2 / d.R);
  return f2bf(c < d.Cr ? d.p[master_index(d, k, c, r, s)] : 0.f);
}

__global__ __launch_bounds__(256) void pack_conv_weights_kernel(PackTable t) {
  const PackDesc d = t.d[blockIdx.y];
  const int rs = d.R * d.S;
  const size_t total = (size_t)d.K * rs * d.C;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += stride) {
    if (d.wc) d.wc[i] = wc_from_master(d, i);
    if (d.wt) {  // i indexes Wt [c][r][s][k]
      const int k = (int)(i % d.K);
      const size_t t1 = i / d.K;
      const int s = (int)(t1 % d.S);
      const size_t t2 = t1 / d.S;
      const int r = (int)(t2 % d.R);
      const int c = (int)(t2 / d.R);
      const float v = c < d.Cr ? d.p[master_index(d, k, c, r, s)] : 0.f;
      d.wt[i] = f2bf(v);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Fused SGD + weight re-pack: ONE launch updates the whole arena and writes the bf16 MFMA
// operand copies of every conv weight from the freshly updated values (no second pass over the
// fp32 weights). One kernel, sgd_pack_kernel<LARS, GUARD, EMA, ADAM, LAMB>, one block per work
// item (int4; "SGD" below is the launch's element rule, AdamW's under ADAM, LAMB's under LAMB):
//   {0, offset, count, -}        plain elementwise chunk;
//   {2, rel_offset, count, desc} elementwise chunk of a conv weight stored [K][R][S][C] (the GPU
//                                arena layout, C == Cr, or 1x1): its bf16 copy Wc has the same
//                                index order, so it is written in the same pass (count multiple
//                                of 4, base 4-aligned: arena tensors are 64-aligned);
//   {1, desc, k0, c0}            one TK x TC x (R*S) tile of a conv weight that needs a layout
//                                change (channel-padded input layer, or a [K][C][R][S] master),
//                                staged through LDS so that the Wc ([k][r][s][c], c fastest) and
//                                optional Wt ([c][r][s][k], k fastest) writes are coalesced;
//   {3, offset, count, slot_offset | -1}  this rank's shard of a sharded bucket — SGD on the fp32
//                                master + momentum, bf16 operand image of the new values
//                                (``shadow``), fp32 send slot of the small tensors (offset, count
//                                and slot_offset multiples of 4: 64-aligned tensors, shards of
//                                n/w with n % 64 == 0 and w | 8); compiled out under ADAM;
//   {4, offset, count, -}        clear gradients outside this rank's shard (count multiple of 4);
//   {5, rel_offset, count, desc} operand re-pack only — the fp32 master was already updated by
//                                the backward (conv_igemm.hip ConvArgs::sgd); bf16(p) into the
//                                operand copy (as item 2).
// The kind is the low byte of the first word. Bit 8 (kItemNoDecay) on an updating item (kinds
// 0-3): its tensor is not weight-decayed (optim/sgd.py ``no_decay``) — the block runs the same
// rule with wd = 0, taken once per block in front of the prologues that use it. Never set on
// kinds 4 and 5.
// Conv descriptors: api.h ConvDesc. Arguments: api.h SgdHyper, LarsArgs, ClipArgs, EmaArgs,
// AdamArgs, LambArgs.
constexpr int kTileElems = 9216;  // fp32 LDS tile (36 KB)
constexpr int kItemKindMask = 0xff;
constexpr int kItemNoDecay = 0x100;

__device__ __forceinline__ int item_kind(const int4& it) { return it.x & kItemKindMask; }

__host__ __device__ __forceinline__ void tile_dims(int RS, int* TK, int* TC) {
  if (RS == 1) { *TK = 64; *TC = 64; }
  else if (RS <= 9) { *TK = 32; *TC = 32; }
  else { *TK = 8; *TC = 16; }
}

// The step's error word (SegmentedDDPStep: a device-side wait timed out), read ONCE per block:
// every thread of the block takes the same branch, so no thread can leave while others still
// wait at a barrier of a tile item or of last_block_done (the word may flip during the launch).
__device__ __forceinline__ bool block_skip(const unsigned* skip) {
  if (!skip) return false;  // (a kernel argument: uniform)
  __shared__ unsigned s_skip;
  if (threadIdx.x == 0) s_skip = __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  return s_skip != 0u;
}

// Last-block-done hand-off: every block's writes are fenced, the block that takes the last
// ticket resets the ticket and release-increments the flag (acquired by flag_wait_kernel).
__device__ __forceinline__ bool last_block_done(unsigned* done) {
  __syncthreads();
  __shared__ unsigned last;
  if (threadIdx.x == 0) {
    __threadfence();
    const unsigned t = __hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last = (t == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  return last != 0u;
}

__device__ __forceinline__ void signal_flag(unsigned* done, unsigned* signal) {
  if (threadIdx.x == 0) {
    __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(signal, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Stage the schedule's next step (api.h LrSched), by one thread of the launch that ends the
// step. A skipped update stages it too: the step still counts.
__device__ __forceinline__ void sched_stage(LrSched* s) {
  const unsigned k = __hip_atomic_load(&s->step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&s->next, k + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One element update of the fused launch. LARS = false: sgd_update1, ``trust`` unused (the
// plain instantiation compiles to what it was before LARS existed). LARS = true: the same fma
// chain with the weight-decayed gradient multiplied by the tensor's trust ratio first (a ratio
// of exactly 1.0 reproduces the plain update bit for bit).
//
// ADAM = true: the AdamW rule of api.h AdamArgs on (p, g, m = b, v) with this block's AdamRule.
// sqrtf and / are correctly rounded: hipcc's default for fp32 (the build passes no -ffast-math
// and leaves -fhip-fp32-correctly-rounded-divide-sqrt on; tests/test_gpu_adamw_exact.py fails
// the day that is not so). ``v`` is unread and unwritten without ADAM.
struct NoAdam {};
struct AdamRule {
  float nla, nlw;  // -(lr * a1), -(lr * wd): one fp32 product each, once per block
  float a2, eps, omb1, beta2, omb2;
};
// LAMB = true (requires ADAM): the rule of api.h LambArgs. lamb_dir is AdamW's first five lines
// and the update direction r with the weight decay inside; the norms kernel and the update body
// both take r from it, every fma written out, so the two passes form the same bits.
struct LambDir {
  float a1, a2, wd, eps, omb1, beta2, omb2;
};
struct LambRule : LambDir {
  float nlt;       // -(lr * trust): one fp32 product, once per block
  bool skip_word;  // SgdHyper::skip, read once per block in front of the trust ratio
};
template <bool ADAM, bool LAMB>
using RuleOf = std::conditional_t<LAMB, LambRule, std::conditional_t<ADAM, AdamRule, NoAdam>>;

__device__ __forceinline__ float lamb_dir(float p, float g, float& m, float& v, float gs,
                                          const LambDir& d) {
  const float G = g * gs;
  m = __builtin_fmaf(d.omb1, G - m, m);
  v = __builtin_fmaf(d.omb2 * G, G, d.beta2 * v);
  const float den = __builtin_fmaf(sqrtf(v), d.a2, d.eps);
  const float u = m / den;
  return __builtin_fmaf(d.wd, p, d.a1 * u);
}

template <bool LARS, bool ADAM, bool LAMB>
__device__ __forceinline__ float sgd1(float p, float g, float& b, float& v, const SgdHyper& h,
                                      float trust, const RuleOf<ADAM, LAMB>& r) {
  if constexpr (LAMB) {
    return __builtin_fmaf(r.nlt, lamb_dir(p, g, b, v, h.grad_scale, r), p);
  } else if constexpr (ADAM) {
    const float G = g * h.grad_scale;
    b = __builtin_fmaf(r.omb1, G - b, b);
    v = __builtin_fmaf(r.omb2 * G, G, r.beta2 * v);
    const float den = __builtin_fmaf(sqrtf(v), r.a2, r.eps);
    const float u = b / den;
    return __builtin_fmaf(r.nla, u, __builtin_fmaf(r.nlw, p, p));
  } else if constexpr (!LARS) {
    return sgd_update1(p, g, b, h.lr, h.momentum, h.wd, h.grad_scale, h.nesterov);
  } else {
    float d = trust * __builtin_fmaf(h.wd, p, g * h.grad_scale);
    if (h.momentum != 0.f) {
      b = __builtin_fmaf(h.momentum, b, d);
      d = h.nesterov ? __builtin_fmaf(h.momentum, b, d) : b;
    }
    return __builtin_fmaf(-h.lr, d, p);
  }
}

// Weight EMA (api.h EmaArgs) of the elements the launch updates, in the same pass: the new p is
// in registers, so the average costs one read and one write of its own arena and no launch.
// The lerp form keeps e to the bit where p_new == e; two roundings, the subtraction and the fma.
// EMA = false: an empty argument and no code (the plain instantiations compile to what they were).
struct NoEma {};
template <bool EMA>
using EmaOf = std::conditional_t<EMA, EmaArgs, NoEma>;

__device__ __forceinline__ float ema_lerp(float e, float np, float one_minus_decay) {
  return __builtin_fmaf(one_minus_decay, np - e, e);
}

// One element, by its arena index.
template <bool EMA>
__device__ __forceinline__ void ema1(const EmaOf<EMA>& m, size_t i, float np) {
  if constexpr (EMA) m.ema[i] = ema_lerp(m.ema[i], np, m.one_minus_decay);
}

// The EMA's element of arena index i (null without EMA: never read).
template <bool EMA>
__device__ __forceinline__ float* ema_at(const EmaOf<EMA>& m, size_t i) {
  if constexpr (EMA) return m.ema + i;
  else return nullptr;
}

// The second moment's element of arena index i (``v`` is null without ADAM: never read).
template <bool ADAM>
__device__ __forceinline__ float* v_at(float* v, size_t i) {
  if constexpr (ADAM) return v + i;
  else return nullptr;
}

// One element by its arena index, every path that is not 16 bytes wide: p, buf (and v) stored,
// +0 into g under zero_grad, the EMA; returns the new p.
template <bool LARS, bool EMA, bool ADAM, bool LAMB>
__device__ __forceinline__ float update1(float* __restrict__ p, float* __restrict__ g,
                                         float* __restrict__ buf, float* v, size_t i,
                                         const SgdHyper& h, float trust, const EmaOf<EMA>& m,
                                         const RuleOf<ADAM, LAMB>& r) {
  float b = buf[i];
  float vv = 0.f;  // (unused without ADAM)
  if constexpr (ADAM) vv = v[i];
  const float np = sgd1<LARS, ADAM, LAMB>(p[i], g[i], b, vv, h, trust, r);
  p[i] = np;
  buf[i] = b;
  if constexpr (ADAM) v[i] = vv;
  if (h.zero_grad) g[i] = 0.f;
  ema1<EMA>(m, i, np);  // (the arena index, as p: the EMA has the masters' layout)
  return np;
}

// The update of four elements (16-byte aligned) on float4 registers: p and buf (and v: v_at of
// the same index) stored, +0 into g under zero_grad, the EMA of the four (``e``: ema_at of the
// same index); returns the new p.
template <bool LARS, bool EMA, bool ADAM, bool LAMB>
__device__ __forceinline__ float4 sgd4(float* p, float* g, float* buf, float* v,
                                       const SgdHyper& h, float trust, float* e,
                                       const EmaOf<EMA>& m, const RuleOf<ADAM, LAMB>& r) {
  float4 pv = *reinterpret_cast<float4*>(p);
  const float4 gv = *reinterpret_cast<const float4*>(g);
  float4 bv = *reinterpret_cast<float4*>(buf);
  float4 vv = make_float4(0.f, 0.f, 0.f, 0.f);  // (unused without ADAM)
  if constexpr (ADAM) vv = *reinterpret_cast<const float4*>(v);
  float4 ev;  // (unused without EMA)
  if constexpr (EMA) ev = *reinterpret_cast<const float4*>(e);
  pv.x = sgd1<LARS, ADAM, LAMB>(pv.x, gv.x, bv.x, vv.x, h, trust, r);
  pv.y = sgd1<LARS, ADAM, LAMB>(pv.y, gv.y, bv.y, vv.y, h, trust, r);
  pv.z = sgd1<LARS, ADAM, LAMB>(pv.z, gv.z, bv.z, vv.z, h, trust, r);
  pv.w = sgd1<LARS, ADAM, LAMB>(pv.w, gv.w, bv.w, vv.w, h, trust, r);
  *reinterpret_cast<float4*>(p) = pv;
  *reinterpret_cast<float4*>(buf) = bv;
  if constexpr (ADAM) *reinterpret_cast<float4*>(v) = vv;
  if (h.zero_grad) *reinterpret_cast<float4*>(g) = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (EMA) {
    ev.x = ema_lerp(ev.x, pv.x, m.one_minus_decay);
    ev.y = ema_lerp(ev.y, pv.y, m.one_minus_decay);
    ev.z = ema_lerp(ev.z, pv.z, m.one_minus_decay);
    ev.w = ema_lerp(ev.w, pv.w, m.one_minus_decay);
    *reinterpret_cast<float4*>(e) = ev;
  }
  return pv;
}

__device__ __forceinline__ uint2 bf16x4(const float4& v) {
  return make_uint2((unsigned)f2bf(v.x) | ((unsigned)f2bf(v.y) << 16),
                    (unsigned)f2bf(v.z) | ((unsigned)f2bf(v.w) << 16));
}

// Arena offset of an elementwise item's first element (kinds 0, 3, 4: absolute; 2, 5: relative
// to their conv master).
__device__ __forceinline__ size_t elem_offset(const int4& it, const ConvDesc* __restrict__ descs) {
  const int kind = item_kind(it);
  return (kind == 2 || kind == 5 ? (size_t)descs[it.w].p_offset : 0) + (unsigned)it.y;
}

// A tile item {1, desc, k0, c0}: TK x TC x (R*S) weights from (k0, c0), cut at the tensor's edges.
struct Tile {
  size_t poff;
  int K, Cr, C, RS, TC, k0, c0;
  int tk, tcr, tcp;  // filters, real channels and padded channels (Wc width) of this tile
  bool krsc;
  __device__ Tile(const ConvDesc& d, const int4& it)
      : poff((size_t)d.p_offset), K((int)d.K), Cr((int)d.Cr), C((int)d.C),
        RS((int)d.R * (int)d.S), k0(it.z), c0(it.w), krsc(d.krsc != 0) {
    int TK;
    tile_dims(RS, &TK, &TC);
    tk = min(TK, K - k0);
    tcr = max(0, min(TC, Cr - c0));
    tcp = min(TC, C - c0);
  }
  // LDS tile layout [kl][cl][rs]
  __device__ int lds(int kl, int cl, int rs) const { return (kl * TC + cl) * RS + rs; }
  // f(arena index, LDS index) for every master element of the tile's real channels, in runs of
  // contiguous floats: tcr * RS of p[k][c][r][s], or tcr channels per (k, r, s) of p[k][r][s][c].
  // The update and the skipped step's clear both walk the tile through this.
  template <class F>
  __device__ __forceinline__ void for_each_master(F&& f) const {
    if (!krsc) {
      const int run = tcr * RS;
      for (int idx = threadIdx.x; idx < tk * run; idx += 256) {
        const int kl = idx / run, e = idx - kl * run;
        f(poff + (size_t)(k0 + kl) * Cr * RS + (size_t)c0 * RS + e, kl * TC * RS + e);
      }
    } else {
      for (int idx = threadIdx.x; idx < tk * RS * tcr; idx += 256) {
        const int cl = idx % tcr, t = idx / tcr;
        const int rs = t % RS, kl = t / RS;
        f(poff + ((size_t)(k0 + kl) * RS + rs) * Cr + c0 + cl, lds(kl, cl, rs));
      }
    }
  }
};

// ---------------------------------------------------------------------------------------------
// LARS (You et al. 2017; optim/lars.py): every adapted tensor's update is multiplied by its
// trust ratio eta * |w| / (|g * grad_scale| + wd * |w| + eps), both norms over the tensor's own
// elements. Gradient guard (optim/sgd.py max_grad_norm / skip_nonfinite): clipping by the norm
// of the whole gradient, and skipping a step whose norm is not finite. The update launch
// consumes and clears the gradient in one pass and runs inside a replayed graph, so both live
// here, in two launches each, no float atomics, so the result does not depend on block scheduling:
//   1) chunk_sums_kernel<WITH_P>: one block per 8192-element chunk (the chunking of the SGD
//      items) stores {sum p^2, sum (g * grad_scale)^2} (LARS, float2) or sum (g * grad_scale)^2
//      alone (the guard, float: half the bytes) into the slot of the chunk's GLOBAL number
//      (numbered over the whole arena: per-bucket launches on different streams never share one);
//   2) the prologue of sgd_pack_kernel: wave 0 of every block sums partials in one fixed order
//      (lane l adds chunks l, l + 64, ... serially, then wave_sum) and broadcasts the result
//      through LDS — every block of every launch gets the same bits.
//      LARS: its tensor's partials give the ratio; the block that owns the tensor's first work
//      item also stores it for the host (LARS.trust_ratios).
//      GUARD: ALL partials of the arena give
//          norm = sqrt(S);  c = min(1, max_norm / (norm + eps)) (1 without a max_norm)
//      and the body runs with grad_scale * c. c == 1.0 reproduces the plain update bit for bit.
//      A norm that is not finite (an Inf / NaN gradient, or S beyond fp32) with skip_nonfinite
//      set: item kinds 0-3 only clear their gradient range (with zero_grad; a stale NaN would
//      poison every later step, the kernels accumulate into the arena), kinds 4 and 5 run as they
//      are; the data cursor, the completion signal and the schedule staging go on as in any
//      step. The ``skip`` word keeps precedence: with it set nothing is touched or recorded.
// The sums are read from memory the first launch wrote, so a zero_grad in the second one is safe.
constexpr int kNormChunk = 8192;  // elements per chunk block (optim/sgd.py FusedSGD.CHUNK)

struct NoP {};
struct WithP { const float* p; };
template <bool WITH_P>
struct ChunkSumArgs : std::conditional_t<WITH_P, WithP, NoP> {
  const int4* items;  // {arena offset (multiple of 4), count <= kNormChunk, global chunk number, -}
  const float* g;
  float grad_scale;
  std::conditional_t<WITH_P, float2, float>* partial;
};

template <bool WITH_P>
__global__ __launch_bounds__(256) void chunk_sums_kernel(ChunkSumArgs<WITH_P> a) {
  const int4 it = a.items[blockIdx.x];
  const size_t off = (size_t)(unsigned)it.x;
  const int cnt = it.y, n4 = cnt >> 2;
  const int tid = threadIdx.x;
  const float* __restrict__ p = nullptr;  // (stays null and unread without WITH_P)
  if constexpr (WITH_P) p = a.p + off;
  const float* __restrict__ g = a.g + off;
  const float4* p4 = reinterpret_cast<const float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  constexpr int kIter = kNormChunk / (256 * 4);
  // (The two forms of the zero below are what each instantiation was compiled from before the
  // two kernels became one, and they stay: with the named zero the compiler splits the two-operand
  // loads into dwords at 74 VGPRs, 6 waves per SIMD; with the temporary it keeps them 16 bytes
  // wide at 92 VGPRs, 5 waves. Which is faster was not measured.)
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 pv[WITH_P ? kIter : 1], gv[kIter];
#pragma unroll
  for (int j = 0; j < kIter; ++j) {  // every 16-byte load of the chunk in flight at once
    const int i = tid + 256 * j;
    if constexpr (WITH_P) {
      pv[j] = i < n4 ? p4[i] : z;
      gv[j] = i < n4 ? g4[i] : z;
    } else {
      gv[j] = i < n4 ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  float sp = 0.f, sg = 0.f;  // one serial fma chain per thread: 4 * kIter (+ 1 tail) terms
#pragma unroll
  for (int j = 0; j < kIter; ++j) {
    const float* pp = &pv[WITH_P ? j : 0].x;
    const float* gg = &gv[j].x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gs = gg[e] * a.grad_scale;
      if constexpr (WITH_P) sp = __builtin_fmaf(pp[e], pp[e], sp);
      sg = __builtin_fmaf(gs, gs, sg);
    }
  }
  const int t = (n4 << 2) + tid;  // scalar tail: numel not a multiple of 4
  if (t < cnt) {
    const float gs = g[t] * a.grad_scale;
    if constexpr (WITH_P) sp = __builtin_fmaf(p[t], p[t], sp);
    sg = __builtin_fmaf(gs, gs, sg);
  }
  if constexpr (WITH_P) sp = wave_sum(sp);
  sg = wave_sum(sg);
  __shared__ std::conditional_t<WITH_P, float2, float> s_w[4];  // per wave
  if ((tid & 63) == 0) {
    if constexpr (WITH_P) s_w[tid >> 6] = make_float2(sp, sg);
    else s_w[tid >> 6] = sg;
  }
  __syncthreads();
  if (tid == 0) {
    if constexpr (WITH_P) {
      a.partial[it.z] = make_float2(((s_w[0].x + s_w[1].x) + s_w[2].x) + s_w[3].x,
                                    ((s_w[0].y + s_w[1].y) + s_w[2].y) + s_w[3].y);
    } else {
      a.partial[it.z] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
    }
  }
}

// This block's trust ratio (1.0: excluded tensor, zero norm, item without an update). Every
// condition but the partial loop's trip count is uniform over the block.
// GUARD: clip first — the gradient norm is that of the clipped gradient, c * gn, with no second
// pass: sum (g gs c)^2 = c^2 * sum (g gs)^2.
template <bool GUARD>
__device__ __forceinline__ float lars_trust_block(const LarsArgs& a, float wd, float c) {
  __shared__ float s_trust;
  if (threadIdx.x < 64) {
    const int2 sd = a.side[blockIdx.x];
    float t = 1.f;
    if (sd.x >= 0) {
      const int4 tn = a.tensors[sd.x];
      if (tn.z) {
        float sp = 0.f, sg = 0.f;
        for (int c = threadIdx.x; c < tn.y; c += 64) {
          const float2 v = a.partial[tn.x + c];
          sp += v.x;
          sg += v.y;
        }
        const float wn = sqrtf(wave_sum(sp));
        float gn = sqrtf(wave_sum(sg));
        if constexpr (GUARD) gn *= c;
        if (wn > 0.f && gn > 0.f) t = a.eta * wn / (gn + wd * wn + a.eps);
      }
      if (sd.y && threadIdx.x == 0) a.trust[sd.x] = t;
    }
    if (threadIdx.x == 0) s_trust = t;
  }
  __syncthreads();
  return s_trust;
}

// LAMB (api.h LambArgs): the same block prologue and the same fixed order of the sums, with the
// ratio wn / rn, rn the norm of the update direction that lamb_norms_kernel formed (from the clipped
// gradient under the guard). (The loop is written out a second time: moved into a function of its
// own, it changes the branch polarity hipcc picks in the four LARS instantiations, and those stay
// instruction for instruction what they were.)
__device__ __forceinline__ float lamb_trust_block(const LambArgs& a) {
  __shared__ float s_trust;
  if (threadIdx.x < 64) {
    const int2 sd = a.side[blockIdx.x];
    float t = 1.f;
    if (sd.x >= 0) {
      const int4 tn = a.tensors[sd.x];
      if (tn.z) {
        float sp = 0.f, sr = 0.f;
        for (int c = threadIdx.x; c < tn.y; c += 64) {
          const float2 v = a.partial[tn.x + c];
          sp += v.x;
          sr += v.y;
        }
        const float wn = sqrtf(wave_sum(sp)), rn = sqrtf(wave_sum(sr));
        if (wn > 0.f && rn > 0.f) t = wn / rn;
      }
      if (sd.y && threadIdx.x == 0) a.trust[sd.x] = t;
    }
    if (threadIdx.x == 0) s_trust = t;
  }
  __syncthreads();
  return s_trust;
}

// The guard's verdict of this step, the same in every block of the launch.
struct GuardState {
  float norm, c;  // sqrt(sum (g * grad_scale)^2) over every parameter element; clip coefficient
  int skipped;    // non-finite norm with skip_nonfinite: the launch only clears the gradients
  float* stats;   // ClipArgs::stats
  int count;      // this launch ends the step: a skipped step is counted
};

__device__ __forceinline__ GuardState clip_block(const ClipArgs& a) {
  __shared__ float s_norm, s_c;
  __shared__ int s_skipped;
  if (threadIdx.x < 64) {
    float s = 0.f;
    for (int c = threadIdx.x; c < a.n_chunks; c += 64) s += a.partial[c];
    const float norm = sqrtf(wave_sum(s));
    float c = 1.f;
    if (a.flags & 1) {
      const float q = a.max_norm / (norm + a.eps);
      c = q >= 1.f ? 1.f : q;  // a NaN norm gives a NaN coefficient, as the arithmetic says
    }
    if (threadIdx.x == 0) {
      s_norm = norm;
      s_c = c;
      s_skipped = ((a.flags & 2) && !(norm <= 3.402823466e+38f)) ? 1 : 0;
    }
  }
  __syncthreads();
  return GuardState{s_norm, s_c, s_skipped, a.stats, (a.flags & 4) ? 1 : 0};
}

// A skipped step's share of a work item of kind 0-3: its gradient range, cleared.
__device__ __forceinline__ void guard_clear(const int4& it, const ConvDesc* __restrict__ descs,
                                            float* __restrict__ g) {
  if (item_kind(it) == 1) {
    Tile(descs[it.y], it).for_each_master([&](size_t gi, int) { g[gi] = 0.f; });
    return;
  }
  float* gp = g + elem_offset(it, descs);
  for (int i = threadIdx.x; i < it.z; i += 256) gp[i] = 0.f;
}

template <bool LARS, bool GUARD, bool EMA, bool ADAM, bool LAMB>
__device__ __forceinline__ void sgd_pack_body(const int4* __restrict__ items,
                                              const ConvDesc* __restrict__ descs,
                                              float* __restrict__ p, float* __restrict__ g,
                                              float* __restrict__ buf, const SgdHyper& h,
                                              float* tile, float trust, const GuardState& gd,
                                              const EmaOf<EMA>& m, float* v,
                                              const RuleOf<ADAM, LAMB>& r) {
  const int4 it = items[blockIdx.x];
  const int kind = item_kind(it);
  const int tid = threadIdx.x;
  if (h.counter && blockIdx.x == 0 && tid == 0) atomicAdd(h.counter, h.delta);
  if constexpr (LAMB) {  // (the kernel read the word already: it stores no ratio either)
    if (r.skip_word) return;
  } else {
    if (block_skip(h.skip)) return;
  }
  if constexpr (GUARD) {
    if (blockIdx.x == 0 && tid == 0) {  // behind the skip word: a timed-out step records nothing
      gd.stats[0] = gd.norm;
      gd.stats[1] = gd.c;
      if (gd.skipped && gd.count) {
        unsigned* n = reinterpret_cast<unsigned*>(gd.stats + 2);
        *n = *n + 1u;
      }
    }
    if (gd.skipped && kind != 4 && kind != 5) {
      if (h.zero_grad) guard_clear(it, descs, g);
      return;
    }
  }
  const int cnt = it.z;  // (elementwise items)
  switch (kind) {
    case 0: {
      const size_t off = elem_offset(it, descs);
      for (int i = tid * 4; i < cnt; i += 256 * 4) {
        if (i + 4 <= cnt && ((off + i) & 3) == 0) {
          sgd4<LARS, EMA, ADAM, LAMB>(p + off + i, g + off + i, buf + off + i, v_at<ADAM>(v, off + i),
                                h, trust, ema_at<EMA>(m, off + i), m, r);
        } else {
          for (int e = i; e < min(cnt, i + 4); ++e)
            update1<LARS, EMA, ADAM, LAMB>(p, g, buf, v, off + e, h, trust, m, r);
        }
      }
      break;
    }
    case 3: {
      if constexpr (!ADAM) {  // (no sharded AdamW: optim/adamw.py refuses before such a table)
        const size_t off = elem_offset(it, descs);
        float* slot = it.w >= 0 && h.slot ? h.slot + it.w : nullptr;
        for (int i = tid * 4; i < cnt; i += 256 * 4) {
          const float4 pv = sgd4<LARS, EMA, ADAM, LAMB>(p + off + i, g + off + i, buf + off + i, nullptr,
                                                  h, trust, ema_at<EMA>(m, off + i), m, r);
          if (h.shadow) *reinterpret_cast<uint2*>(h.shadow + off + i) = bf16x4(pv);
          if (slot) *reinterpret_cast<float4*>(slot + i) = pv;
        }
      }
      break;
    }
    case 4: {
      const size_t off = elem_offset(it, descs);
      for (int i = tid * 4; i < cnt; i += 256 * 4)
        *reinterpret_cast<float4*>(g + off + i) = make_float4(0.f, 0.f, 0.f, 0.f);
      break;
    }
    case 2: {  // no LDS staging: the operand copy has the master's own index order
      const size_t base = elem_offset(it, descs);
      unsigned short* wc = descs[it.w].wc + (unsigned)it.y;
      for (int i = tid * 4; i < cnt; i += 256 * 4) {
        const float4 pv = sgd4<LARS, EMA, ADAM, LAMB>(p + base + i, g + base + i, buf + base + i,
                                                v_at<ADAM>(v, base + i), h, trust,
                                                ema_at<EMA>(m, base + i), m, r);
        *reinterpret_cast<uint2*>(wc + i) = bf16x4(pv);
      }
      break;
    }
    case 5: {
      const size_t base = elem_offset(it, descs);
      unsigned short* wc = descs[it.w].wc + (unsigned)it.y;
      for (int i = tid * 4; i < cnt; i += 256 * 4)
        *reinterpret_cast<uint2*>(wc + i) = bf16x4(*reinterpret_cast<const float4*>(p + base + i));
      break;
    }
    case 1: {
      const ConvDesc& d = descs[it.y];
      const Tile t(d, it);
      // 1) SGD on the master for the tile's real channels, new values into the LDS tile
      t.for_each_master([&](size_t gi, int li) {
        tile[li] = update1<LARS, EMA, ADAM, LAMB>(p, g, buf, v, gi, h, trust, m, r);
      });
      __syncthreads();
      // 2) Wc[k][r][s][c] (c fastest, zero for padded channels)
      if (d.wc) {
        for (int idx = tid; idx < t.tk * t.RS * t.tcp; idx += 256) {
          const int cl = idx % t.tcp, q = idx / t.tcp;
          const int rs = q % t.RS, kl = q / t.RS;
          const float v = cl < t.tcr ? tile[t.lds(kl, cl, rs)] : 0.f;
          d.wc[((size_t)(t.k0 + kl) * t.RS + rs) * t.C + t.c0 + cl] = f2bf(v);
        }
      }
      // 3) Wt[c][r][s][k] (k fastest)
      if (d.wt) {
        for (int idx = tid; idx < t.tcr * t.RS * t.tk; idx += 256) {
          const int kl = idx % t.tk, q = idx / t.tk;
          const int rs = q % t.RS, cl = q / t.RS;
          d.wt[((size_t)(t.c0 + cl) * t.RS + rs) * t.K + t.k0 + kl] = f2bf(tile[t.lds(kl, cl, rs)]);
        }
      }
      break;
    }
  }
}

// The kernel's arguments behind the tables and arenas (their __restrict__ keeps the table reads
// scalar): SgdHyper, then LarsArgs, ClipArgs, EmaArgs, AdamArgs and LambArgs only in the
// instantiations that read them (an empty base takes no kernarg bytes; an empty struct argument
// would).
struct NoLars {};
struct NoClip {};
struct NoLamb {};
template <bool LARS, bool GUARD, bool EMA, bool ADAM, bool LAMB = false>
struct UpdateArgs : SgdHyper, std::conditional_t<LARS, LarsArgs, NoLars>,
                    std::conditional_t<GUARD, ClipArgs, NoClip>, EmaOf<EMA>,
                    std::conditional_t<ADAM, AdamArgs, NoAdam>,
                    std::conditional_t<LAMB, LambArgs, NoLamb> {};
static_assert(sizeof(UpdateArgs<false, false, false, false>) == 96 &&
              sizeof(UpdateArgs<false, true, false, false>) == 128 &&
              sizeof(UpdateArgs<true, false, false, false>) == 136 &&
              sizeof(UpdateArgs<true, true, false, false>) == 168 &&
              sizeof(UpdateArgs<false, false, true, false>) == 112 &&
              sizeof(UpdateArgs<false, true, true, false>) == 144 &&
              sizeof(UpdateArgs<true, false, true, false>) == 152 &&
              sizeof(UpdateArgs<true, true, true, false>) == 184 &&
              sizeof(UpdateArgs<false, false, false, true>) == 136 &&
              sizeof(UpdateArgs<false, true, false, true>) == 168 &&
              sizeof(UpdateArgs<false, false, true, true>) == 152 &&
              sizeof(UpdateArgs<false, true, true, true>) == 184 &&
              sizeof(UpdateArgs<false, false, false, true, true>) == 168 &&
              sizeof(UpdateArgs<false, true, false, true, true>) == 200 &&
              sizeof(UpdateArgs<false, false, true, true, true>) == 184 &&
              sizeof(UpdateArgs<false, true, true, true, true>) == 216,
              "kernarg bytes of the sixteen instantiations (ADAM excludes LARS, LAMB needs ADAM)");

// ADAM: this step's {learning rate, a1, a2} (api.h AdamArgs), read once per block where the plain
// instantiations read the learning rate: thread 0 loads, LDS broadcast, one barrier. The step
// word is the schedule's (common.h sched_lr): no launch that reads it writes it.
__device__ __forceinline__ AdamRule adam_rule_block(const AdamArgs& a, const SgdHyper& h) {
  __shared__ float s_rule[3];
  if (threadIdx.x == 0) {
    const LrSched* s = h.sched;
    const unsigned k = __hip_atomic_load(&s->step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned n = s->n;
    const float lr = reinterpret_cast<const float*>(s + 1)[k < n ? k : n - 1];
    const float2 bc = a.bias[k < a.n_bias ? k : a.n_bias - 1];
    s_rule[0] = -(lr * bc.x);
    s_rule[1] = -(lr * h.wd);
    s_rule[2] = bc.y;
  }
  __syncthreads();
  return AdamRule{s_rule[0], s_rule[1], s_rule[2], a.eps, a.omb1, a.beta2, a.omb2};
}

// LAMB: this step's learning rate (into ``lr``) and the update direction's constants, both passes'
// (lamb_norms_kernel, the LAMB instantiations of sgd_pack_kernel): the table reads of
// adam_rule_block, the products left to lamb_dir and to the trust ratio.
__device__ __forceinline__ LambDir lamb_dir_block(const AdamArgs& a, const LrSched* s, float wd,
                                                  float* lr) {
  __shared__ float s_tab[3];
  if (threadIdx.x == 0) {
    const unsigned k = __hip_atomic_load(&s->step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned n = s->n;
    const float2 bc = a.bias[k < a.n_bias ? k : a.n_bias - 1];
    s_tab[0] = reinterpret_cast<const float*>(s + 1)[k < n ? k : n - 1];
    s_tab[1] = bc.x;
    s_tab[2] = bc.y;
  }
  __syncthreads();
  *lr = s_tab[0];
  return LambDir{s_tab[1], s_tab[2], wd, a.eps, a.omb1, a.beta2, a.omb2};
}

// LAMB's norms pass (api.h LambNorms): chunk_sums_kernel's shape over p, g, m, v. One block per
// chunk item forms m', v', u and r of its elements in registers, stores none of them, and writes
// {sum p^2, sum r^2} into the chunk's global slot. GUARD: r is not linear in the clip coefficient,
// so the block takes it from the guard's partials first (clip_block: the update launch's own
// fixed-order sum, the same bits) and forms r from g * (grad_scale * c). On a step the guard will
// skip the sums may be anything: no block of the update reads them.
template <bool GUARD>
struct LambNormArgs : std::conditional_t<GUARD, ClipArgs, NoClip> {
  const int4* items;  // as ChunkSumArgs::items; bit 0 of the fourth field: wd = 0 for this chunk
  const float* p;
  const float* g;
  const float* m;
  const LrSched* sched;
  float wd, grad_scale;
  AdamArgs adam;      // v (read only), the bias table and the rule's constants
  float2* partial;
};

template <bool GUARD>
__global__ __launch_bounds__(256) void lamb_norms_kernel(LambNormArgs<GUARD> a) {
  const int4 it = a.items[blockIdx.x];
  const size_t off = (size_t)(unsigned)it.x;
  const int cnt = it.y, n4 = cnt >> 2;
  const int tid = threadIdx.x;
  float lr;  // (not needed here)
  const LambDir d = lamb_dir_block(a.adam, a.sched, (it.w & 1) ? 0.f : a.wd, &lr);
  float gs = a.grad_scale;
  if constexpr (GUARD) gs *= clip_block(a).c;
  const float* __restrict__ p = a.p + off;
  const float* __restrict__ g = a.g + off;
  const float* __restrict__ m = a.m + off;
  const float* __restrict__ v = a.adam.v + off;
  constexpr int kIter = kNormChunk / (256 * 4);
  float4 pv[kIter], gv[kIter], mv[kIter], vv[kIter];
#pragma unroll
  for (int j = 0; j < kIter; ++j) {  // every 16-byte load of the chunk in flight at once
    const int i = tid + 256 * j;
    if (i < n4) {
      pv[j] = reinterpret_cast<const float4*>(p)[i];
      gv[j] = reinterpret_cast<const float4*>(g)[i];
      mv[j] = reinterpret_cast<const float4*>(m)[i];
      vv[j] = reinterpret_cast<const float4*>(v)[i];
    }
  }
  float sp = 0.f, sr = 0.f;  // one serial fma chain per thread: 4 * kIter (+ 1 tail) terms
#pragma unroll
  for (int j = 0; j < kIter; ++j) {
    if (tid + 256 * j < n4) {  // (no zero stand-ins: with eps == 0 they would give u = 0 / 0)
      const float* pp = &pv[j].x;
      const float* gg = &gv[j].x;
      float* mm = &mv[j].x;
      float* ww = &vv[j].x;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float r = lamb_dir(pp[e], gg[e], mm[e], ww[e], gs, d);
        sp = __builtin_fmaf(pp[e], pp[e], sp);
        sr = __builtin_fmaf(r, r, sr);
      }
    }
  }
  const int t = (n4 << 2) + tid;  // scalar tail: numel not a multiple of 4
  if (t < cnt) {
    float mt = m[t], vt = v[t];
    const float r = lamb_dir(p[t], g[t], mt, vt, gs, d);
    sp = __builtin_fmaf(p[t], p[t], sp);
    sr = __builtin_fmaf(r, r, sr);
  }
  sp = wave_sum(sp);
  sr = wave_sum(sr);
  __shared__ float2 s_w[4];  // per wave
  if ((tid & 63) == 0) s_w[tid >> 6] = make_float2(sp, sr);
  __syncthreads();
  if (tid == 0) {
    a.partial[it.z] = make_float2(((s_w[0].x + s_w[1].x) + s_w[2].x) + s_w[3].x,
                                  ((s_w[0].y + s_w[1].y) + s_w[2].y) + s_w[3].y);
  }
}

template <bool LARS, bool GUARD, bool EMA, bool ADAM, bool LAMB>
__global__ __launch_bounds__(256) void sgd_pack_kernel(const int4* __restrict__ items,
                                                       const ConvDesc* __restrict__ descs,
                                                       float* __restrict__ p,
                                                       float* __restrict__ g,
                                                       float* __restrict__ buf,
                                                       UpdateArgs<LARS, GUARD, EMA, ADAM, LAMB> a) {
  static_assert(!(LARS && ADAM), "AdamW has no trust ratios");
  static_assert(ADAM || !LAMB, "LAMB is a rule on AdamW's moments");
  __shared__ float tile[kTileElems];
  SgdHyper h = a;
  // (a scalar load and a block-uniform select: the item table is const __restrict__)
  if (items[blockIdx.x].x & kItemNoDecay) h.wd = 0.f;
  RuleOf<ADAM, LAMB> rule{};
  float* v = nullptr;  // (stays null and unread without ADAM)
  if constexpr (LAMB) {
    static_cast<LambDir&>(rule) = lamb_dir_block(a, h.sched, h.wd, &h.lr);
    v = a.v;
  } else if constexpr (ADAM) {
    rule = adam_rule_block(a, h);
    v = a.v;
  } else {
    h.lr = sched_lr_block(h.sched, h.lr);
  }
  if (h.sched_advance && blockIdx.x == 0 && threadIdx.x == 0) sched_stage(h.sched);
  GuardState gd{0.f, 1.f, 0, nullptr, 0};
  if constexpr (GUARD) gd = clip_block(a);
  float trust = 1.f;
  // (a skipped step leaves the stored ratios as they are)
  if constexpr (LARS) trust = GUARD && gd.skipped ? 1.f : lars_trust_block<GUARD>(a, h.wd, gd.c);
  if constexpr (LAMB) {  // (the skip word keeps precedence: nothing is touched or recorded)
    rule.skip_word = block_skip(h.skip);
    const bool none = rule.skip_word || (GUARD && gd.skipped);
    rule.nlt = -(h.lr * (none ? 1.f : lamb_trust_block(a)));
  }
  if constexpr (GUARD) h.grad_scale *= gd.c;
  sgd_pack_body<LARS, GUARD, EMA, ADAM, LAMB>(items, descs, p, g, buf, h, tile, trust, gd, a, v,
                                              rule);
  if (h.signal && last_block_done(h.done)) signal_flag(h.done, h.signal);
}

// Tail of a pipelined step with sharded buckets (parallel/zero.py ShardedBf16Update.tail): one
// block per segment copies gathered small-tensor values (fp32 send slots of every rank) into
// the fp32 parameter arena; the last block to finish re-packs the bf16 operand copies of the
// channel-padded conv weights among them (their masters are complete only now) and signals
// the step's "every parameter updated" flag. Segment entries: int4 {src, dst, count, -}.
constexpr int kMaxTailPack = 4;
struct TailArgs {
  const int4* segs;
  int n_segs;
  const float* src;
  float* dst;
  PackDesc pack[kMaxTailPack];
  int n_pack;
  unsigned* done;
  unsigned* signal;
  const unsigned* skip;
};

__global__ __launch_bounds__(256) void shard_tail_kernel(TailArgs a) {
  const bool skipped = block_skip(a.skip);
  if (!skipped && (int)blockIdx.x < a.n_segs) {
    const int4 e = a.segs[blockIdx.x];
    const float* s = a.src + (size_t)(unsigned)e.x;
    float* d = a.dst + (size_t)(unsigned)e.y;
    for (int i = threadIdx.x; i < e.z; i += 256) d[i] = s[i];
  }
  if (!last_block_done(a.done)) return;
  __threadfence();  // acquire side: the other blocks' copies are visible to this block
  if (!skipped) {
    for (int q = 0; q < a.n_pack; ++q) {
      const PackDesc& d = a.pack[q];
      const int total = d.K * d.R * d.S * d.C;
      for (int i = threadIdx.x; i < total; i += 256) d.wc[i] = wc_from_master(d, i);
    }
    __syncthreads();
    __threadfence();
  }
  if (a.signal) signal_flag(a.done, a.signal);
  else if (threadIdx.x == 0) __hip_atomic_store(a.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void counter_add_kernel(int* c, int delta, LrSched* sched, int sched_mode) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (c) *c += delta;
  if (!sched) return;
  if (sched_mode == 1) sched_stage(sched);
  const unsigned k = __hip_atomic_load(&sched->next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&sched->step, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LARS, bool GUARD, bool EMA, bool ADAM = false, bool LAMB = false>
static int launch_update(const UpdateLaunch& u, hipStream_t st) {
  UpdateArgs<LARS, GUARD, EMA, ADAM, LAMB> a{};
  static_cast<SgdHyper&>(a) = u.h;
  a.sched_advance = a.sched && a.sched_advance ? 1 : 0;
  if constexpr (LARS) static_cast<LarsArgs&>(a) = u.lars;
  if constexpr (GUARD) static_cast<ClipArgs&>(a) = u.clip;
  if constexpr (EMA) static_cast<EmaArgs&>(a) = u.ema;
  if constexpr (ADAM) static_cast<AdamArgs&>(a) = u.adam;
  if constexpr (LAMB) static_cast<LambArgs&>(a) = u.lamb;
  hipLaunchKernelGGL((sgd_pack_kernel<LARS, GUARD, EMA, ADAM, LAMB>), dim3(u.n_items), dim3(256), 0,
                     st, u.items, u.descs, u.p, u.g, u.buf, a);
  return (int)hipGetLastError();
}

template <bool GUARD>
static int launch_lamb_norms(const LambNorms& n, hipStream_t st) {
  LambNormArgs<GUARD> a{};
  if constexpr (GUARD) static_cast<ClipArgs&>(a) = n.clip;
  a.items = n.items; a.p = n.p; a.g = n.g; a.m = n.m; a.sched = n.sched;
  a.wd = n.wd; a.grad_scale = n.grad_scale; a.adam = n.adam; a.partial = n.partial;
  hipLaunchKernelGGL(lamb_norms_kernel<GUARD>, dim3(n.n_items), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

template <bool WITH_P, class Partial>
static int launch_chunk_sums(const void* items, int n_items, const float* p, const float* g,
                             float grad_scale, Partial* partial, hipStream_t st) {
  if (n_items <= 0) return 0;
  ChunkSumArgs<WITH_P> a{};
  if constexpr (WITH_P) a.p = p;
  a.items = (const int4*)items; a.g = g; a.grad_scale = grad_scale; a.partial = partial;
  hipLaunchKernelGGL(chunk_sums_kernel<WITH_P>, dim3(n_items), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace ddp_amd

using namespace ddp_amd;

extern "C" int ddp_sgd(float* p, const float* g, float* buf, size_t n, float lr, float momentum,
                       float wd, float grad_scale, int nesterov, const LrSched* sched,
                       hipStream_t st) {
  size_t blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p, g, buf, n, lr,
                     momentum, wd, grad_scale, nesterov, sched);
  return (int)hipGetLastError();
}

extern "C" int ddp_pack_conv_weights(const PackDesc* descs, int n, hipStream_t st) {
  for (int base = 0; base < n; base += kMaxPack) {
    PackTable t{};
    t.n = n - base < kMaxPack ? n - base : kMaxPack;
    size_t maxel = 0;
    for (int i = 0; i < t.n; ++i) {
      t.d[i] = descs[base + i];
      const size_t el = (size_t)t.d[i].K * t.d[i].R * t.d[i].S * t.d[i].C;
      if (el > maxel) maxel = el;
    }
    size_t bx = (maxel + 255) / 256;
    if (bx > 512) bx = 512;
    hipLaunchKernelGGL(pack_conv_weights_kernel, dim3((unsigned)bx, t.n), dim3(256), 0, st, t);
  }
  return (int)hipGetLastError();
}

extern "C" int ddp_sgd_pack(const UpdateLaunch* u, hipStream_t st) {
  if (u->n_items <= 0) return 0;
  const bool lars = u->lars.side, guard = u->clip.partial;
  if (guard && (!u->clip.stats || u->clip.n_chunks < 0)) return -1;
  if (lars && (!u->lars.tensors || !u->lars.partial || !u->lars.trust)) return -1;
  const bool lamb = u->lamb.side;
  if (lamb && (!u->adam.v || lars || !u->lamb.tensors || !u->lamb.partial || !u->lamb.trust))
    return -1;
  if (u->adam.v) {  // AdamW: the step number comes from the schedule's step word
    if (lars || !u->adam.bias || !u->adam.n_bias || !u->h.sched) return -1;
    if (lamb) {
      if (u->ema.ema)
        return (guard ? launch_update<false, true, true, true, true>
                      : launch_update<false, false, true, true, true>)(*u, st);
      return (guard ? launch_update<false, true, false, true, true>
                    : launch_update<false, false, false, true, true>)(*u, st);
    }
    if (u->ema.ema)
      return (guard ? launch_update<false, true, true, true>
                    : launch_update<false, false, true, true>)(*u, st);
    return (guard ? launch_update<false, true, false, true>
                  : launch_update<false, false, false, true>)(*u, st);
  }
  if (u->ema.ema)
    return (lars ? (guard ? launch_update<true, true, true> : launch_update<true, false, true>)
                 : (guard ? launch_update<false, true, true> : launch_update<false, false, true>))(*u, st);
  return (lars ? (guard ? launch_update<true, true, false> : launch_update<true, false, false>)
               : (guard ? launch_update<false, true, false> : launch_update<false, false, false>))(*u, st);
}

extern "C" int ddp_grad_sumsq(const void* items, int n_items, const float* g, float grad_scale,
                              float* partial, hipStream_t st) {
  return launch_chunk_sums<false>(items, n_items, nullptr, g, grad_scale, partial, st);
}

extern "C" int ddp_lars_norms(const void* items, int n_items, const float* p, const float* g,
                              float grad_scale, void* partial, hipStream_t st) {
  return launch_chunk_sums<true>(items, n_items, p, g, grad_scale, (float2*)partial, st);
}

extern "C" int ddp_lamb_norms(const LambNorms* n, hipStream_t st) {
  if (n->n_items <= 0) return 0;
  const bool guard = n->clip.partial;
  if (!n->items || !n->p || !n->g || !n->m || !n->adam.v || !n->partial) return -1;
  if (!n->adam.bias || !n->adam.n_bias || !n->sched || (guard && n->clip.n_chunks < 0)) return -1;
  return (guard ? launch_lamb_norms<true> : launch_lamb_norms<false>)(*n, st);
}

extern "C" int ddp_shard_tail(const void* segs, int n_segs, const float* src, float* dst,
                              const PackDesc* pack, int n_pack, unsigned* done, unsigned* signal,
                              const unsigned* skip, hipStream_t st) {
  if (n_pack > kMaxTailPack || !done) return -1;
  TailArgs a{};
  a.segs = (const int4*)segs; a.n_segs = n_segs; a.src = src; a.dst = dst;
  for (int i = 0; i < n_pack; ++i) a.pack[i] = pack[i];
  a.n_pack = n_pack; a.done = done; a.signal = signal; a.skip = skip;
  hipLaunchKernelGGL(shard_tail_kernel, dim3(n_segs > 0 ? n_segs : 1), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

// Host-side tile shape so Python can build the item table.
extern "C" void ddp_sgd_tile_dims(int RS, int* TK, int* TC) { tile_dims(RS, TK, TC); }

// Floats of the tile kernel's LDS tile: a tile item needs TK * TC * R * S of them, and the
// Python table builder refuses a tensor that needs more.
extern "C" int ddp_sgd_tile_limit() { return kTileElems; }

extern "C" int ddp_counter_add(int* c, int delta, LrSched* sched, int sched_mode,
                               hipStream_t st) {
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(64), 0, st, c, delta, sched, sched_mode);
  return (int)hipGetLastError();
}
