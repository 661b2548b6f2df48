// What the normalisation kernels that keep a tile in registers share (group_norm.hip,
// ghost_bn.hip): a lane's 16-byte vector of 8 bf16 channels as fp32, and the ONE expression of
// xhat and the pre-activation that a forward and its backward's recompute both use.
#pragma once
#include "common.h"

namespace ddp_amd {
namespace tile {

struct F8 { float v[8]; };

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
__device__ __forceinline__ F8 ldf8(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  return F8{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}

// xhat and the pre-activation: ONE expression for the forward and the backward's recompute
__device__ __forceinline__ float xhat_of(float z, float mu, float is) { return (z - mu) * is; }
__device__ __forceinline__ float pre_of(float xh, float g, float b) { return __builtin_fmaf(xh, g, b); }

}  // namespace tile
}  // namespace ddp_amd
