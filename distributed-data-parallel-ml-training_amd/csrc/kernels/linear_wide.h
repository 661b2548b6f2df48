// What the two classifier-head translation units share: the soft-target rule of the loss kernels
// (linear_ce.hip, linear_wide.hip) and the launchers of the wide head (linear_wide.hip), which
// linear_ce.hip's entry points route 16 < J <= 128 to.
#pragma once
#include "common.h"

namespace ddp_amd {

constexpr int kMaxHeadF = 1024;
constexpr int kWideMaxJ = 128;

// Soft targets (api.h SoftTarget; label smoothing E and mixup partner yb with weight lam) of one
// row, as the SOFT instantiations of the loss kernels evaluate them:
//   t_j       = fma(1 - E, wa [j == ya] + wb [j == yb], E / J)
//   loss term = fma(E / J, sum_j z_j, (1 - E) * fma(wa, z_ya, wb * z_yb))
// with (wa, wb) = (lam, 1 - lam), or (1, 0) when yb == ya (lam + (1 - lam) is 1 without a
// rounding). E = 0, lam = 1 or yb == ya gives t = onehot(ya) and the term z_ya, bit for bit.
struct SoftRow {
  float om, u, wa, wb;  // 1 - E, E / J, the two label weights
  int yb;
  __device__ __forceinline__ SoftRow(const SoftTarget& s, int row, int ya, int J) {
    const float lam = s.lam ? *s.lam : 1.f;
    yb = s.labels_b ? (int)s.labels_b[row] : ya;
    om = 1.f - s.smoothing;
    u = s.smoothing / (float)J;
    wa = yb == ya ? 1.f : lam;
    wb = yb == ya ? 0.f : 1.f - lam;
  }
  __device__ __forceinline__ float target(int j, int ya) const {
    return __builtin_fmaf(om, (j == ya ? wa : 0.f) + (j == yb ? wb : 0.f), u);
  }
  __device__ __forceinline__ float term(float z_ya, float z_yb, float sum_z) const {
    return __builtin_fmaf(u, sum_z, om * __builtin_fmaf(wa, z_ya, wb * z_yb));
  }
};
__device__ __forceinline__ const SoftTarget& only(const SoftTarget& s) { return s; }

// The wide head: 16 < J <= kWideMaxJ, F % 32 == 0, F <= kMaxHeadF, B >= 1; -1 otherwise, else
// the HIP error code of the one launch. Arguments as ddp_linear_ce_fwd[_soft] / ddp_linear_bwd.
int linear_wide_fwd(const void* x, const float* W, const float* b, const long long* labels, int B,
                    int F, int J, float* logits, float* dlogits, float* loss_sum, int* correct,
                    float* loss_acc, const SoftTarget* soft, hipStream_t st);
int linear_wide_bwd(const float* dlogits, const void* x, const float* W, int B, int F, int J,
                    const float* gscale, void* dx, float* dW, float* db, hipStream_t st);

}  // namespace ddp_amd
