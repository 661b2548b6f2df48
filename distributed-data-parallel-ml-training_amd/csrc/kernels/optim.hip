// Optimizer and weight-layout kernels for gfx950.
//
// Reference parity: optim.SGD(lr=0.1, momentum=0.9, weight_decay=1e-4) over the 34 VGG-11
// parameter tensors (part1/main.py:124-125, step at :77) — SURVEY.md §2.B N2g. Here ONE
// launch updates the whole flat fp32 parameter arena (all tensors are views into it):
//     d = g * grad_scale + wd * p ; buf = momentum * buf + d ; d = nesterov ? d + momentum*buf : buf
//     p -= lr * d
// A zero-initialised momentum buffer reproduces torch's "buf = clone(d) on the first step"
// exactly (momentum * 0 + d == d), so the kernel needs no first-step flag (graph friendly).
//
// pack_conv_weights re-lays the fp32 master weights (PyTorch [K][C][R][S]) into the two bf16
// MFMA operand layouts used by conv_igemm.hip: Wc [K][R][S][Cpad] (fwd) and Wt [C][R][S][K]
// (dgrad); all conv tensors of the model in one launch (blockIdx.y = tensor).
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

__global__ __launch_bounds__(256) void pack_conv_weights_kernel(PackTable t) {
  const PackDesc d = t.d[blockIdx.y];
  const int rs = d.R * d.S;
  const size_t total = (size_t)d.K * rs * d.C;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += stride) {
    if (d.wc) {  // i indexes Wc [k][r][s][c]
      const int c = (int)(i % d.C);
      const size_t t1 = i / d.C;
      const int s = (int)(t1 % d.S);
      const size_t t2 = t1 / d.S;
      const int r = (int)(t2 % d.R);
      const int k = (int)(t2 / d.R);
      const float v = c < d.Cr ? d.p[master_index(d, k, c, r, s)] : 0.f;
      d.wc[i] = f2bf(v);
    }
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
// fp32 weights). Work items (int4): {0, offset, count, -} = plain elementwise chunk;
// {2, rel_offset, count, desc} = elementwise chunk of a conv weight stored [K][R][S][C] (the GPU
// arena layout): its bf16 copy Wc has the same index order, so it is written in the same pass;
// {1, desc, k0, c0} = one TK x TC x (R*S) tile of a conv weight that needs a layout change
// (channel-padded input layer, or a [K][C][R][S] master), staged through LDS so that the Wc
// ([k][r][s][c], c fastest) and optional Wt ([c][r][s][k], k fastest) writes are coalesced.
// Conv descriptor (int64 x 12): {p_offset, K, Cr, C, R, S, wc_ptr, wt_ptr, krsc, -, -, -};
// krsc selects the fp32 master layout ([K][R][S][Cr] vs [K][Cr][R][S]).
constexpr int kTileElems = 9216;  // fp32 LDS tile (36 KB)

__device__ __forceinline__ void tile_dims(int RS, int* TK, int* TC) {
  if (RS == 1) { *TK = 64; *TC = 64; }
  else if (RS <= 9) { *TK = 32; *TC = 32; }
  else { *TK = 8; *TC = 16; }
}

struct SgdHyper {
  float lr, momentum, wd, grad_scale;
  int nesterov;
  int zero_grad;  // write 0 to every gradient after use (replaces the next step's zero_grad fill)
  int* counter;   // optional step counter (data cursor): += delta by one thread
  int delta;
  // optional error word (engine/step.py SegmentedDDPStep): non-zero when a device-side wait for
  // a gradient bucket timed out — the update is then skipped instead of applying gradients
  // that were never averaged (the host raises on the error at its next check)
  const unsigned* skip;
  // sharded update with a bf16 operand all-gather (parallel/zero.py ShardedBf16Update): item 3
  // also stores bf16(new p) into ``shadow`` (the bf16 operand image of the arena, same element
  // index) and, for the small fp32-wire tensors, the new p into ``slot`` (the all-gather send slot)
  unsigned short* shadow;
  float* slot;
  // optional completion signal (engine/step.py SegmentedDDPStep, last bucket): the last block
  // to finish (``done`` ticket, reset by it) release-increments ``signal`` — the step's
  // "every parameter updated" flag without a separate signal launch
  unsigned* done;
  unsigned* signal;
  // optional learning-rate schedule (api.h LrSched): every block reads this step's rate from the
  // table instead of ``lr``; ``sched_advance``: this launch ends the training step — block 0
  // stages the next step (``next``, read by no block here; a later launch makes it current)
  LrSched* sched;
  int sched_advance;
};

// Last-block-done hand-off: every block's writes are fenced, the block that takes the last
// ticket resets the ticket and release-increments the flag (acquired by flag_wait_kernel).
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
template <bool LARS>
__device__ __forceinline__ float sgd1(float p, float g, float& b, const SgdHyper& h, float trust) {
  if constexpr (!LARS) {
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

// Gradient guard of the clipped instantiations (ClipArgs below): this step's verdict, the same
// in every block of the launch.
struct GuardState {
  float norm, c;  // sqrt(sum (g * grad_scale)^2) over every parameter element; clip coefficient
  int skipped;    // non-finite norm with skip_nonfinite: the launch only clears the gradients
  float* stats;   // {norm, c, skipped steps (uint32), -}, stored by block 0
  int count;      // this launch ends the step: a skipped step is counted
};

template <bool LARS, bool GUARD = false>
__device__ void sgd_pack_body(const int4* __restrict__ items, const long long* __restrict__ descs,
                              float* __restrict__ p, float* __restrict__ g,
                              float* __restrict__ buf, const SgdHyper& h, float* tile,
                              float trust, GuardState gd = GuardState{});

__global__ __launch_bounds__(256) void sgd_pack_kernel(const int4* __restrict__ items,
                                                       const long long* __restrict__ descs,
                                                       float* __restrict__ p,
                                                       float* __restrict__ g,
                                                       float* __restrict__ buf, SgdHyper h) {
  __shared__ float tile[kTileElems];
  h.lr = sched_lr_block(h.sched, h.lr);
  if (h.sched_advance && blockIdx.x == 0 && threadIdx.x == 0) sched_stage(h.sched);
  sgd_pack_body<false>(items, descs, p, g, buf, h, tile, 1.f);
  if (h.signal && last_block_done(h.done)) signal_flag(h.done, h.signal);
}

// ---------------------------------------------------------------------------------------------
// LARS (You et al. 2017; optim/lars.py): every adapted tensor's update is multiplied by its
// trust ratio eta * |w| / (|g * grad_scale| + wd * |w| + eps), both norms over the tensor's own
// elements. Two launches, no float atomics, so the result does not depend on block scheduling:
//   1) lars_norms_kernel: one block per 8192-element chunk (the chunking of the SGD items) stores
//      {sum p^2, sum (g * grad_scale)^2} of its chunk into the slot of the chunk's GLOBAL number
//      (numbered over the whole arena: per-bucket launches on different streams never share one);
//   2) lars_pack_kernel, the LARS instantiation of the fused SGD + re-pack body: wave 0 of every
//      block sums its tensor's partials in one fixed order (lane l adds chunks l, l + 64, ...
//      serially, then wave_sum), computes the ratio and broadcasts it through LDS; the block
//      that owns the tensor's first work item also stores it for the host (LARS.trust_ratios).
// The norms are read from memory the first launch wrote, so a zero_grad in the second one is safe.
struct LarsArgs {
  const int2* side;       // per work item: {parameter index | -1 (no ratio: item 5), first item}
  const int4* tensors;    // per parameter: {first global chunk, chunks, adapted, -}
  const float2* partial;  // per global chunk: {sum p^2, sum (g * grad_scale)^2}
  float* trust;           // per parameter (written)
  float eta, eps;
};

constexpr int kNormChunk = 8192;  // elements per norm block (optim/lars.py LARS.CHUNK)

__global__ __launch_bounds__(256) void lars_norms_kernel(const int4* __restrict__ items,
                                                         const float* __restrict__ p,
                                                         const float* __restrict__ g,
                                                         float grad_scale,
                                                         float2* __restrict__ partial) {
  // {arena offset (multiple of 4), count <= kNormChunk, global chunk number, -}
  const int4 it = items[blockIdx.x];
  const size_t off = (size_t)(unsigned)it.x;
  const int cnt = it.y, n4 = cnt >> 2;
  const int tid = threadIdx.x;
  const float4* p4 = reinterpret_cast<const float4*>(p + off);
  const float4* g4 = reinterpret_cast<const float4*>(g + off);
  constexpr int kIter = kNormChunk / (256 * 4);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 pv[kIter], gv[kIter];
#pragma unroll
  for (int j = 0; j < kIter; ++j) {  // every 16-byte load of the chunk in flight at once
    const int i = tid + 256 * j;
    pv[j] = i < n4 ? p4[i] : z;
    gv[j] = i < n4 ? g4[i] : z;
  }
  float sp = 0.f, sg = 0.f;  // one serial fma chain per thread: 4 * kIter (+ 1 tail) terms
#pragma unroll
  for (int j = 0; j < kIter; ++j) {
    const float* pp = &pv[j].x;
    const float* gg = &gv[j].x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gs = gg[e] * grad_scale;
      sp = __builtin_fmaf(pp[e], pp[e], sp);
      sg = __builtin_fmaf(gs, gs, sg);
    }
  }
  const int t = (n4 << 2) + tid;  // scalar tail: numel not a multiple of 4
  if (t < cnt) {
    const float pt = p[off + t], gs = g[off + t] * grad_scale;
    sp = __builtin_fmaf(pt, pt, sp);
    sg = __builtin_fmaf(gs, gs, sg);
  }
  sp = wave_sum(sp);
  sg = wave_sum(sg);
  __shared__ float2 s_w[4];
  if ((tid & 63) == 0) s_w[tid >> 6] = make_float2(sp, sg);
  __syncthreads();
  if (tid == 0) {
    partial[it.z] = make_float2(((s_w[0].x + s_w[1].x) + s_w[2].x) + s_w[3].x,
                                ((s_w[0].y + s_w[1].y) + s_w[2].y) + s_w[3].y);
  }
}

// This block's trust ratio (1.0: excluded tensor, zero norm, item without an update). Every
// condition but the partial loop's trip count is uniform over the block.
// GUARD (the clipped instantiation): clip first — the gradient norm is that of the clipped
// gradient, c * gn, with no second pass: sum (g gs c)^2 = c^2 * sum (g gs)^2.
template <bool GUARD = false>
__device__ __forceinline__ float lars_trust_block(const LarsArgs& a, float wd, float c = 1.f) {
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

__global__ __launch_bounds__(256) void lars_pack_kernel(const int4* __restrict__ items,
                                                        const long long* __restrict__ descs,
                                                        float* __restrict__ p,
                                                        float* __restrict__ g,
                                                        float* __restrict__ buf, SgdHyper h,
                                                        LarsArgs la) {
  __shared__ float tile[kTileElems];
  h.lr = sched_lr_block(h.sched, h.lr);
  if (h.sched_advance && blockIdx.x == 0 && threadIdx.x == 0) sched_stage(h.sched);
  const float trust = lars_trust_block(la, h.wd);
  sgd_pack_body<true>(items, descs, p, g, buf, h, tile, trust);
  if (h.signal && last_block_done(h.done)) signal_flag(h.done, h.signal);
}

// ---------------------------------------------------------------------------------------------
// Gradient clipping and non-finite step skipping (optim/sgd.py max_grad_norm / skip_nonfinite).
// The update launch consumes and clears the gradient in one pass and runs inside a replayed
// graph, so the guard lives here, in two launches like LARS:
//   1) grad_sumsq_kernel: one block per 8192-element chunk of every parameter (the chunking and
//      the whole-arena chunk numbers of lars_norms_kernel) stores sum (g * grad_scale)^2 of its
//      chunk: half the bytes of the LARS norms pass, no float atomics;
//   2) the clipped instantiations of the fused update: wave 0 of every block sums ALL partials of
//      the arena in one fixed order (lane l adds chunks l, l + 64, ... serially, then wave_sum) —
//      every block of every launch gets the same bits —
//          norm = sqrt(S);  c = min(1, max_norm / (norm + eps)) (1 without a max_norm)
//      and the body runs with grad_scale * c. c == 1.0 reproduces the plain update bit for bit.
//      A norm that is not finite (an Inf / NaN gradient, or S beyond fp32) with skip_nonfinite
//      set: item kinds 0-3 only clear their gradient range (with zero_grad; a stale NaN would
//      poison every later step, the kernels accumulate into the arena), kinds 4 and 5 run as they
//      are; the data cursor, the completion signal and the schedule staging go on as in any
//      step. The ``skip`` word keeps precedence: with it set nothing is touched or recorded.
struct ClipArgs {
  const float* partial;  // per global chunk: sum (g * grad_scale)^2 (grad_sumsq_kernel)
  int n_chunks;          // chunks of the whole arena
  float max_norm, eps;
  int flags;             // 1: clip to max_norm, 2: skip a non-finite step, 4: count a skipped step
  float* stats;          // GuardState::stats
};

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const int4* __restrict__ items,
                                                         const float* __restrict__ g,
                                                         float grad_scale,
                                                         float* __restrict__ partial) {
  // {arena offset (multiple of 4), count <= kNormChunk, global chunk number, -}
  const int4 it = items[blockIdx.x];
  const size_t off = (size_t)(unsigned)it.x;
  const int cnt = it.y, n4 = cnt >> 2;
  const int tid = threadIdx.x;
  const float4* g4 = reinterpret_cast<const float4*>(g + off);
  constexpr int kIter = kNormChunk / (256 * 4);
  float4 gv[kIter];
#pragma unroll
  for (int j = 0; j < kIter; ++j) {  // every 16-byte load of the chunk in flight at once
    const int i = tid + 256 * j;
    gv[j] = i < n4 ? g4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float sg = 0.f;  // one serial fma chain per thread: 4 * kIter (+ 1 tail) terms
#pragma unroll
  for (int j = 0; j < kIter; ++j) {
    const float* gg = &gv[j].x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gs = gg[e] * grad_scale;
      sg = __builtin_fmaf(gs, gs, sg);
    }
  }
  const int t = (n4 << 2) + tid;  // scalar tail: numel not a multiple of 4
  if (t < cnt) {
    const float gs = g[off + t] * grad_scale;
    sg = __builtin_fmaf(gs, gs, sg);
  }
  sg = wave_sum(sg);
  __shared__ float s_w[4];
  if ((tid & 63) == 0) s_w[tid >> 6] = sg;
  __syncthreads();
  if (tid == 0) partial[it.z] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// This step's verdict, computed by wave 0 of every block from the same partials in the same
// order and broadcast through LDS (as lars_trust_block).
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
__device__ __forceinline__ void guard_clear(const int4& it, const long long* __restrict__ descs,
                                            float* __restrict__ g) {
  const int tid = threadIdx.x;
  if (it.x == 0 || it.x == 3) {
    float* gp = g + (size_t)(unsigned)it.y;
    for (int i = tid; i < it.z; i += 256) gp[i] = 0.f;
    return;
  }
  if (it.x == 2) {
    float* gp = g + (size_t)descs[12 * it.w] + (unsigned)it.y;
    for (int i = tid; i < it.z; i += 256) gp[i] = 0.f;
    return;
  }
  const long long* d = descs + 12 * it.y;  // kind 1: the tile's real channels (as the body)
  const size_t poff = (size_t)d[0];
  const int K = (int)d[1], Cr = (int)d[2], RS = (int)d[4] * (int)d[5];
  int TK, TC;
  tile_dims(RS, &TK, &TC);
  const int k0 = it.z, c0 = it.w;
  const int tk = min(TK, K - k0);
  const int tcr = max(0, min(TC, Cr - c0));
  if (d[8] == 0) {
    const int run = tcr * RS;
    for (int idx = tid; idx < tk * run; idx += 256) {
      const int kl = idx / run, e = idx - kl * run;
      g[poff + (size_t)(k0 + kl) * Cr * RS + (size_t)c0 * RS + e] = 0.f;
    }
  } else {
    for (int idx = tid; idx < tk * RS * tcr; idx += 256) {
      const int cl = idx % tcr, t = idx / tcr;
      const int rs = t % RS, kl = t / RS;
      g[poff + ((size_t)(k0 + kl) * RS + rs) * Cr + c0 + cl] = 0.f;
    }
  }
}

template <bool LARS, bool GUARD>
__device__ void sgd_pack_body(const int4* __restrict__ items, const long long* __restrict__ descs,
                              float* __restrict__ p, float* __restrict__ g,
                              float* __restrict__ buf, const SgdHyper& h, float* tile,
                              float trust, GuardState gd) {
  const int4 it = items[blockIdx.x];
  const int tid = threadIdx.x;
  if (h.counter && blockIdx.x == 0 && tid == 0) atomicAdd(h.counter, h.delta);
  if (block_skip(h.skip)) return;
  if constexpr (GUARD) {
    if (blockIdx.x == 0 && tid == 0) {  // behind the skip word: a timed-out step records nothing
      gd.stats[0] = gd.norm;
      gd.stats[1] = gd.c;
      if (gd.skipped && gd.count) {
        unsigned* n = reinterpret_cast<unsigned*>(gd.stats + 2);
        *n = *n + 1u;
      }
    }
    if (gd.skipped && it.x != 4 && it.x != 5) {
      if (h.zero_grad) guard_clear(it, descs, g);
      return;
    }
  }
  if (it.x == 0) {
    const size_t off = (size_t)(unsigned)it.y;
    const int cnt = it.z;
    for (int i = tid * 4; i < cnt; i += 256 * 4) {
      if (i + 4 <= cnt && ((off + i) & 3) == 0) {
        float4 pv = *reinterpret_cast<float4*>(p + off + i);
        const float4 gv = *reinterpret_cast<const float4*>(g + off + i);
        float4 bv = *reinterpret_cast<float4*>(buf + off + i);
        pv.x = sgd1<LARS>(pv.x, gv.x, bv.x, h, trust);
        pv.y = sgd1<LARS>(pv.y, gv.y, bv.y, h, trust);
        pv.z = sgd1<LARS>(pv.z, gv.z, bv.z, h, trust);
        pv.w = sgd1<LARS>(pv.w, gv.w, bv.w, h, trust);
        *reinterpret_cast<float4*>(p + off + i) = pv;
        *reinterpret_cast<float4*>(buf + off + i) = bv;
        if (h.zero_grad) *reinterpret_cast<float4*>(g + off + i) = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        for (int e = i; e < min(cnt, i + 4); ++e) {
          float b = buf[off + e];
          p[off + e] = sgd1<LARS>(p[off + e], g[off + e], b, h, trust);
          buf[off + e] = b;
          if (h.zero_grad) g[off + e] = 0.f;
        }
      }
    }
    return;
  }
  if (it.x == 3) {
    // {3, offset, count, slot_offset | -1}: this rank's shard of a sharded bucket — SGD on the
    // fp32 master + momentum, bf16 operand image of the new values, fp32 send slot of the
    // small tensors (offset, count and slot_offset multiples of 4: 64-aligned tensors, shards
    // of n/w with n % 64 == 0 and w | 8)
    const size_t off = (size_t)(unsigned)it.y;
    const int cnt = it.z;
    float* slot = it.w >= 0 && h.slot ? h.slot + it.w : nullptr;
    for (int i = tid * 4; i < cnt; i += 256 * 4) {
      float4 pv = *reinterpret_cast<float4*>(p + off + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + off + i);
      float4 bv = *reinterpret_cast<float4*>(buf + off + i);
      pv.x = sgd1<LARS>(pv.x, gv.x, bv.x, h, trust);
      pv.y = sgd1<LARS>(pv.y, gv.y, bv.y, h, trust);
      pv.z = sgd1<LARS>(pv.z, gv.z, bv.z, h, trust);
      pv.w = sgd1<LARS>(pv.w, gv.w, bv.w, h, trust);
      *reinterpret_cast<float4*>(p + off + i) = pv;
      *reinterpret_cast<float4*>(buf + off + i) = bv;
      if (h.zero_grad) *reinterpret_cast<float4*>(g + off + i) = make_float4(0.f, 0.f, 0.f, 0.f);
      if (h.shadow) {
        uint2 pk;
        pk.x = (unsigned)f2bf(pv.x) | ((unsigned)f2bf(pv.y) << 16);
        pk.y = (unsigned)f2bf(pv.z) | ((unsigned)f2bf(pv.w) << 16);
        *reinterpret_cast<uint2*>(h.shadow + off + i) = pk;
      }
      if (slot) *reinterpret_cast<float4*>(slot + i) = pv;
    }
    return;
  }
  if (it.x == 4) {
    // {4, offset, count, -}: clear gradients outside this rank's shard (count multiple of 4)
    const size_t off = (size_t)(unsigned)it.y;
    for (int i = tid * 4; i < it.z; i += 256 * 4)
      *reinterpret_cast<float4*>(g + off + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  if (it.x == 5) {
    // {5, offset in the tensor, count, desc}: operand re-pack only — the fp32 master was already
    // updated by the backward (conv_igemm.hip ConvArgs::sgd); bf16(p) into the operand copy
    // (same index order as item 2; count multiple of 4)
    const long long* d = descs + 12 * it.w;
    const size_t base = (size_t)d[0] + (unsigned)it.y;
    unsigned short* wc = reinterpret_cast<unsigned short*>(d[6]) + (unsigned)it.y;
    for (int i = tid * 4; i < it.z; i += 256 * 4) {
      const float4 pv = *reinterpret_cast<const float4*>(p + base + i);
      uint2 pk;
      pk.x = (unsigned)f2bf(pv.x) | ((unsigned)f2bf(pv.y) << 16);
      pk.y = (unsigned)f2bf(pv.z) | ((unsigned)f2bf(pv.w) << 16);
      *reinterpret_cast<uint2*>(wc + i) = pk;
    }
    return;
  }
  if (it.x == 2) {
    // conv weight whose bf16 operand copy has the master's own index order ([K][R][S][C] with
    // C == Cr, or 1x1): elementwise update + bf16 store, no LDS staging
    const long long* d = descs + 12 * it.w;
    const size_t base = (size_t)d[0] + (unsigned)it.y;
    unsigned short* wc = reinterpret_cast<unsigned short*>(d[6]) + (unsigned)it.y;
    const int cnt = it.z;  // multiple of 4, base 4-aligned (arena tensors are 64-aligned)
    for (int i = tid * 4; i < cnt; i += 256 * 4) {
      float4 pv = *reinterpret_cast<float4*>(p + base + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + base + i);
      float4 bv = *reinterpret_cast<float4*>(buf + base + i);
      pv.x = sgd1<LARS>(pv.x, gv.x, bv.x, h, trust);
      pv.y = sgd1<LARS>(pv.y, gv.y, bv.y, h, trust);
      pv.z = sgd1<LARS>(pv.z, gv.z, bv.z, h, trust);
      pv.w = sgd1<LARS>(pv.w, gv.w, bv.w, h, trust);
      *reinterpret_cast<float4*>(p + base + i) = pv;
      *reinterpret_cast<float4*>(buf + base + i) = bv;
      if (h.zero_grad) *reinterpret_cast<float4*>(g + base + i) = make_float4(0.f, 0.f, 0.f, 0.f);
      uint2 pk;
      pk.x = (unsigned)f2bf(pv.x) | ((unsigned)f2bf(pv.y) << 16);
      pk.y = (unsigned)f2bf(pv.z) | ((unsigned)f2bf(pv.w) << 16);
      *reinterpret_cast<uint2*>(wc + i) = pk;
    }
    return;
  }
  const long long* d = descs + 12 * it.y;
  const size_t poff = (size_t)d[0];
  const int K = (int)d[1], Cr = (int)d[2], C = (int)d[3], R = (int)d[4], S = (int)d[5];
  unsigned short* wc = reinterpret_cast<unsigned short*>(d[6]);
  unsigned short* wt = reinterpret_cast<unsigned short*>(d[7]);
  const int RS = R * S;
  int TK, TC;
  tile_dims(RS, &TK, &TC);
  const int k0 = it.z, c0 = it.w;
  const int tk = min(TK, K - k0);
  const int tcr = max(0, min(TC, Cr - c0));  // real channels in this tile
  const int tcp = min(TC, C - c0);           // padded channels in this tile (Wc width)
  const bool krsc = d[8] != 0;
  if (!krsc) {
    // 1) SGD on p[k][c][r][s] for the tile's real channels; runs of tcr*RS contiguous floats
    const int run = tcr * RS;
    for (int idx = tid; idx < tk * run; idx += 256) {
      const int kl = idx / run, e = idx - kl * run;
      const size_t gi = poff + (size_t)(k0 + kl) * Cr * RS + (size_t)c0 * RS + e;
      float b = buf[gi];
      const float np = sgd1<LARS>(p[gi], g[gi], b, h, trust);
      p[gi] = np;
      buf[gi] = b;
      if (h.zero_grad) g[gi] = 0.f;
      tile[kl * TC * RS + e] = np;  // tile layout [kl][cl][rs]
    }
  } else {
    // 1) SGD on p[k][r][s][c]: runs of tcr contiguous channels per (k, r, s)
    for (int idx = tid; idx < tk * RS * tcr; idx += 256) {
      const int cl = idx % tcr, t = idx / tcr;
      const int rs = t % RS, kl = t / RS;
      const size_t gi = poff + ((size_t)(k0 + kl) * RS + rs) * Cr + c0 + cl;
      float b = buf[gi];
      const float np = sgd1<LARS>(p[gi], g[gi], b, h, trust);
      p[gi] = np;
      buf[gi] = b;
      if (h.zero_grad) g[gi] = 0.f;
      tile[kl * TC * RS + cl * RS + rs] = np;
    }
  }
  __syncthreads();
  // 2) Wc[k][r][s][c] (c fastest, zero for padded channels)
  if (wc) {
    for (int idx = tid; idx < tk * RS * tcp; idx += 256) {
      const int cl = idx % tcp, t = idx / tcp;
      const int rs = t % RS, kl = t / RS;
      const float v = cl < tcr ? tile[(kl * TC + cl) * RS + rs] : 0.f;
      wc[((size_t)(k0 + kl) * RS + rs) * C + c0 + cl] = f2bf(v);
    }
  }
  // 3) Wt[c][r][s][k] (k fastest)
  if (wt) {
    for (int idx = tid; idx < tcr * RS * tk; idx += 256) {
      const int kl = idx % tk, t = idx / tk;
      const int rs = t % RS, cl = t / RS;
      wt[((size_t)(c0 + cl) * RS + rs) * K + k0 + kl] = f2bf(tile[(kl * TC + cl) * RS + rs]);
    }
  }
}

// The clipped instantiations of the two kernels above (ClipArgs): the same launch, body and
// arguments, run with grad_scale * c.
__global__ __launch_bounds__(256) void sgd_clip_pack_kernel(const int4* __restrict__ items,
                                                            const long long* __restrict__ descs,
                                                            float* __restrict__ p,
                                                            float* __restrict__ g,
                                                            float* __restrict__ buf, SgdHyper h,
                                                            ClipArgs ca) {
  __shared__ float tile[kTileElems];
  h.lr = sched_lr_block(h.sched, h.lr);
  if (h.sched_advance && blockIdx.x == 0 && threadIdx.x == 0) sched_stage(h.sched);
  const GuardState gd = clip_block(ca);
  h.grad_scale *= gd.c;
  sgd_pack_body<false, true>(items, descs, p, g, buf, h, tile, 1.f, gd);
  if (h.signal && last_block_done(h.done)) signal_flag(h.done, h.signal);
}

__global__ __launch_bounds__(256) void lars_clip_pack_kernel(const int4* __restrict__ items,
                                                             const long long* __restrict__ descs,
                                                             float* __restrict__ p,
                                                             float* __restrict__ g,
                                                             float* __restrict__ buf, SgdHyper h,
                                                             LarsArgs la, ClipArgs ca) {
  __shared__ float tile[kTileElems];
  h.lr = sched_lr_block(h.sched, h.lr);
  if (h.sched_advance && blockIdx.x == 0 && threadIdx.x == 0) sched_stage(h.sched);
  const GuardState gd = clip_block(ca);
  // (a skipped step leaves the stored ratios as they are)
  const float trust = gd.skipped ? 1.f : lars_trust_block<true>(la, h.wd, gd.c);
  h.grad_scale *= gd.c;
  sgd_pack_body<true, true>(items, descs, p, g, buf, h, tile, trust, gd);
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
      const int rs = d.R * d.S;
      const int total = d.K * rs * d.C;
      for (int i = threadIdx.x; i < total; i += 256) {  // Wc [k][r][s][c], zero padded c
        const int c = i % d.C, t1 = i / d.C;
        const int sx = t1 % d.S, t2 = t1 / d.S;
        const int r = t2 % d.R, k = t2 / d.R;
        const float v = c < d.Cr ? d.p[master_index(d, k, c, r, sx)] : 0.f;
        d.wc[i] = f2bf(v);
      }
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

extern "C" int ddp_sgd_pack(const void* items, int n_items, const long long* descs, float* p,
                            float* g, float* buf, float lr, float momentum, float wd,
                            float grad_scale, int nesterov, int zero_grad, int* counter,
                            int delta, const unsigned* skip, unsigned short* shadow, float* slot,
                            unsigned* done, unsigned* signal, LrSched* sched, int sched_advance,
                            const void* lars_side, const void* lars_tensors,
                            const void* lars_partial, float* lars_trust, float lars_eta,
                            float lars_eps, const float* clip_partial, int clip_chunks,
                            float clip_max_norm, float clip_eps, int clip_flags,
                            float* clip_stats, hipStream_t st) {
  SgdHyper h{lr, momentum, wd, grad_scale, nesterov, zero_grad, counter, delta, skip, shadow, slot,
             done, signal, sched, sched && sched_advance ? 1 : 0};
  if (n_items <= 0) return 0;
  if (clip_partial && (!clip_stats || clip_chunks < 0)) return -1;
  ClipArgs ca{clip_partial, clip_chunks, clip_max_norm, clip_eps, clip_flags, clip_stats};
  if (lars_side) {
    if (!lars_tensors || !lars_partial || !lars_trust) return -1;
    LarsArgs la{(const int2*)lars_side, (const int4*)lars_tensors, (const float2*)lars_partial,
                lars_trust, lars_eta, lars_eps};
    if (clip_partial) {
      hipLaunchKernelGGL(lars_clip_pack_kernel, dim3(n_items), dim3(256), 0, st,
                         (const int4*)items, descs, p, g, buf, h, la, ca);
      return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(lars_pack_kernel, dim3(n_items), dim3(256), 0, st, (const int4*)items,
                       descs, p, g, buf, h, la);
    return (int)hipGetLastError();
  }
  if (clip_partial) {
    hipLaunchKernelGGL(sgd_clip_pack_kernel, dim3(n_items), dim3(256), 0, st, (const int4*)items,
                       descs, p, g, buf, h, ca);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(sgd_pack_kernel, dim3(n_items), dim3(256), 0, st, (const int4*)items, descs,
                     p, g, buf, h);
  return (int)hipGetLastError();
}

extern "C" int ddp_grad_sumsq(const void* items, int n_items, const float* g, float grad_scale,
                              float* partial, hipStream_t st) {
  if (n_items <= 0) return 0;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(n_items), dim3(256), 0, st, (const int4*)items, g,
                     grad_scale, partial);
  return (int)hipGetLastError();
}

extern "C" int ddp_lars_norms(const void* items, int n_items, const float* p, const float* g,
                              float grad_scale, void* partial, hipStream_t st) {
  if (n_items <= 0) return 0;
  hipLaunchKernelGGL(lars_norms_kernel, dim3(n_items), dim3(256), 0, st, (const int4*)items, p, g,
                     grad_scale, (float2*)partial);
  return (int)hipGetLastError();
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

// Host-side tile shape (must match tile_dims above) so Python can build the item table.
extern "C" void ddp_sgd_tile_dims(int RS, int* TK, int* TC) {
  if (RS == 1) { *TK = 64; *TC = 64; }
  else if (RS <= 9) { *TK = 32; *TC = 32; }
  else { *TK = 8; *TC = 16; }
}

// Floats of the tile kernel's LDS tile: a tile item needs TK * TC * R * S of them, and the
// Python table builder refuses a tensor that needs more.
extern "C" int ddp_sgd_tile_limit() { return kTileElems; }

extern "C" int ddp_counter_add(int* c, int delta, LrSched* sched, int sched_mode,
                               hipStream_t st) {
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(64), 0, st, c, delta, sched, sched_mode);
  return (int)hipGetLastError();
}
