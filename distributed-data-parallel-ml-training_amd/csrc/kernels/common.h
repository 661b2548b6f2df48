// Shared device helpers for the gfx950 (CDNA4) kernel library.
// Activations are NHWC bf16; master weights / gradients / optimizer state are fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>

#include "api.h"

namespace ddp_amd {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int kWave = 64;  // CDNA wavefront width (never 32)

// Debug builds (DDP_AMD_DEBUG_BUILD=1 -> -DDDP_AMD_DEBUG, see _build.py): device-side bounds /
// shape checks that print the failing condition and stop the offending thread's work. No-ops
// in release builds. (GPU sanitizers are not available on this pool; this plus
// HIP_LAUNCH_BLOCKING=1 localises a faulting kernel)
#ifdef DDP_AMD_DEBUG
#define DDP_DEVICE_CHECK(cond)                                                              \
  do {                                                                                      \
    if (!(cond)) {                                                                          \
      printf("[ddp_amd debug] %s:%d check failed: %s (block %d thread %d)\n", __FILE__,     \
             __LINE__, #cond, (int)blockIdx.x, (int)threadIdx.x);                           \
      return;                                                                               \
    }                                                                                       \
  } while (0)
#else
#define DDP_DEVICE_CHECK(cond) \
  do {                        \
  } while (0)
#endif

// Replica of a block's BatchNorm-statistics partial sums (api.h kStatRep) and the value it adds:
// release builds spread blocks over the replicas; the deterministic build gives each block its
// own replica and poisons replica 0 with NaN when a grid outgrows kStatRep.
__device__ __forceinline__ int stat_rep(int b) {
#ifdef DDP_AMD_DETERMINISTIC
  return b < kStatRep ? b : 0;
#else
  return b % kStatRep;
#endif
}
__device__ __forceinline__ float stat_val(float v, int b) {
#ifdef DDP_AMD_DETERMINISTIC
  return b < kStatRep ? v : __builtin_nanf("");
#else
  (void)b;
  return v;
#endif
}

// One SGD element update (torch.optim.SGD: d = g + wd p; b = m b + d; d = nesterov ? d + m b : b;
// p -= lr d), with every multiply-add an explicit fma in one fixed order: the optimizer launch
// (optim.hip) and the SGD in the WGRAD finish (conv_igemm.hip) are separate translation units,
// and left to -ffp-contract they round differently (1 ulp; tests/test_gpu_deterministic.py).
__device__ __forceinline__ float sgd_update1(float p, float g, float& b, float lr, float momentum,
                                             float wd, float grad_scale, int nesterov) {
  float d = __builtin_fmaf(wd, p, g * grad_scale);
  if (momentum != 0.f) {
    b = __builtin_fmaf(momentum, b, d);
    d = nesterov ? __builtin_fmaf(momentum, b, d) : b;
  }
  return __builtin_fmaf(-lr, d, p);
}

// Learning rate of the current step from the device schedule (api.h LrSched). The step word is
// never written by a launch that reads it, only by launches stream-ordered between the end of
// one step and the next step's first reader, so all readers of one step see the same value.
__device__ __forceinline__ float sched_lr(const LrSched* s) {
  const unsigned k = __hip_atomic_load(&s->step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned n = s->n;
  return reinterpret_cast<const float*>(s + 1)[k < n ? k : n - 1];
}
// ... read once per block: thread 0 loads, LDS broadcast, barrier. ``s`` must be uniform over
// the block (a kernel argument); null keeps the immediate value and takes no barrier.
__device__ __forceinline__ float sched_lr_block(const LrSched* s, float lr) {
  if (!s) return lr;
  __shared__ float s_lr;
  if (threadIdx.x == 0) s_lr = sched_lr(s);
  __syncthreads();
  return s_lr;
}

// bf16 <-> fp32 bit conversions. round-to-nearest-even; NaN kept NaN.
__device__ __forceinline__ float bf2f(unsigned short h) {
  return __uint_as_float(((unsigned int)h) << 16);
}
// A plain cast lowers to v_cvt_pk_bf16_f32 (RNE, NaN-preserving) on gfx950 -O3.
__device__ __forceinline__ unsigned short f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float round_bf(float f) { return bf2f(f2bf(f)); }

// 16-byte vector load/store of 8 bf16 values as raw u16 lanes.
__device__ __forceinline__ u16x8 ld8(const unsigned short* p) {
  return *reinterpret_cast<const u16x8*>(p);
}
__device__ __forceinline__ void st8(unsigned short* p, u16x8 v) {
  *reinterpret_cast<u16x8*>(p) = v;
}

// DPP lane exchange within each 16-lane row (ctrl: quad_perm / row_half_mirror / row_mirror)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// Sum over the 16 lanes of a DPP row, result in every lane of the row: quad_perm [1,0,3,2] and
// [2,3,0,1], row_half_mirror, row_mirror — four DPP adds instead of four ds_bpermute round
// trips through the LDS unit (__shfl_xor).
__device__ __forceinline__ float dpp_sum16(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  return v;
}
__device__ __forceinline__ float lane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
// Full-wave reductions, result in every lane; all 64 lanes must be active (uniform control
// flow): DPP within the rows, then the four row results through v_readlane.
__device__ __forceinline__ float wave_sum(float v) {
  v = dpp_sum16(v);
  return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0x140>(v));
  return fmaxf(fmaxf(lane_f(v, 0), lane_f(v, 16)), fmaxf(lane_f(v, 32), lane_f(v, 48)));
}

// Bijective XCD-aware block remap (cdna_hip_programming.md §5 "XCD swizzle must be bijective"):
// consecutive logical tiles land on the same XCD (shared L2) instead of round-robin.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  const int nx = 8;
  if (nwg < nx) return orig;
  const int q = nwg / nx, r = nwg % nx;
  const int xcd = orig % nx, idx = orig / nx;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// x / d for 0 <= x < 2^31 with a multiplier precomputed on the host (make_fastdiv, d >= 1):
// q = (mulhi(x, mul) + x) >> sh. Every divisor that is fixed for a launch travels as one of
// these in the kernel arguments: a runtime integer division is a 30-40 instruction software
// routine on this ISA, a FastDiv is a multiply-high, an add and a shift — scalar instructions
// when x is uniform over the wave.
struct FastDiv {
  unsigned mul;
  int sh;
};
__device__ __forceinline__ int fast_div(int x, FastDiv d) {
  return (int)((__umulhi((unsigned)x, d.mul) + (unsigned)x) >> d.sh);
}
inline FastDiv make_fastdiv(int d) {
  FastDiv f;
  int sh = 0;
  while ((1ll << sh) < d) ++sh;
  f.sh = sh;
  f.mul = (unsigned)((((1ull << sh) - (unsigned long long)d) << 32) / (unsigned long long)d + 1);
  return f;
}

// In-kernel cycle stamps of the conv GEMM work items — diagnostic builds only
// (-DDDP_CONV_STAMPS, _build.py variant "stamps"; tools/probes/conv_item_stamps.py). The shipped
// builds compile none of this. A stamped kernel records, per work item, the shader-clock cycles
// its first wave spent in setup (index math, gather state), in the k-loop (prologue DMA
// included) and in the epilogue. Buffer: word 0 counts the records, word 4 + 4 i.. holds record
// i = {tag, setup, k-loop, epilogue}; records past ``cap`` are counted but not written.
#ifdef DDP_CONV_STAMPS
struct ConvStampBuf {
  unsigned* buf;
  int cap;
};
extern ConvStampBuf g_conv_stamps;  // host: the buffer the next launches record into (or null)
__device__ __forceinline__ unsigned long long stamp_now() {
  // the scheduling barriers pin the read between the phases it separates
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t = __builtin_readcyclecounter();
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
__device__ __forceinline__ void stamp_put(const ConvStampBuf& s, unsigned tag, unsigned long long t0,
                                          unsigned long long t1, unsigned long long t2,
                                          unsigned long long t3) {
  if (!s.buf || threadIdx.x != 0) return;
  const unsigned i = atomicAdd(s.buf, 1u);
  if (i >= (unsigned)s.cap) return;
  unsigned* r = s.buf + 4 + 4 * (size_t)i;
  r[0] = tag;
  r[1] = (unsigned)(t1 - t0);
  r[2] = (unsigned)(t2 - t1);
  r[3] = (unsigned)(t3 - t2);
}
#endif

// Counter-based RNG (splitmix-style 32-bit hash); identical formula in data/synthetic.py.
__host__ __device__ __forceinline__ uint32_t hash_u32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ uint32_t hash3(uint32_t a, uint32_t b, uint32_t c) {
  return hash_u32(a ^ hash_u32(b ^ hash_u32(c + 0x9e3779b9u)));
}

}  // namespace ddp_amd
