// wab_policy_opt.h — parameter blocks of the device policy's optimizer step (wab_policy_opt.hip;
// wab_policy_adam_step in include/wab.h), shared with the C-ABI host code.
#pragma once

#include "wab_policy.h"

namespace wab {

constexpr int kAdamSegment = 1024;  // elements of one workgroup's subtree of the norm's pair tree
constexpr int kAdamTensors = 10;    // w1, b1, w2, b2, w3, b3, wa, ba, wv, bv (wab_policy_weights)

// wab_adam_state (include/wab.h), device memory
struct AdamState {
  uint64_t step, skipped;
  double beta1_pow, beta2_pow;
  float grad_norm, clip_scale;
  uint64_t reserved;
};

// The call's constants: wab_adam_config and what the host derives from it alone (the contract's
// float casts; the same bits wherever they are made).
struct AdamConsts {
  double lr, beta1, beta2, max_grad_norm;
  float b1f, omb1, b2f, omb2, epsf, wdf, decayf;
  int32_t decay;  // 0: none, 1: L2 (added to the gradient), 2: decoupled (the parameter shrinks first)
};

// Flat order of the norm: the ten tensors one after the other, each row-major.  P < 2^32
// (in_features <= 2^20, widths <= 256).
struct AdamFlat {
  const float* g[kAdamTensors];
  uint32_t off[kAdamTensors + 1];  // off[t]: first flat index of tensor t; off[10] = P
};

inline AdamFlat adam_flat(const PolicyDims& d) {
  AdamFlat f = {};
  const uint32_t n[kAdamTensors] = {(uint32_t)d.h1 * (uint32_t)d.F, (uint32_t)d.h1, (uint32_t)d.h2 * (uint32_t)d.h1,
                                    (uint32_t)d.h2, (uint32_t)d.h3 * (uint32_t)d.h2, (uint32_t)d.h3,
                                    (uint32_t)d.A * (uint32_t)d.h3, (uint32_t)d.A, (uint32_t)d.h3, 1u};
  f.off[0] = 0;
  for (int t = 0; t < kAdamTensors; ++t) f.off[t + 1] = f.off[t] + n[t];
  return f;
}

// The norm's partial sums in the workspace: level 0 holds one double per 1024 flat elements, each
// further level one per 1024 of the level before, until at most 1024 are left (`last`, `n_last`):
// those the update and the finish launches sum themselves.  At most two levels (P < 2^32 / 8).
struct AdamLevels {
  int32_t n_levels;
  uint32_t count[3];   // doubles of each level
  uint32_t offset[3];  // its first double in the workspace
  uint32_t total;      // doubles
};

inline AdamLevels adam_levels(uint32_t P) {
  AdamLevels L = {};
  uint32_t n = (P + (uint32_t)kAdamSegment - 1u) / (uint32_t)kAdamSegment, o = 0;
  for (;;) {
    L.count[L.n_levels] = n;
    L.offset[L.n_levels] = o;
    o += n;
    ++L.n_levels;
    if (n <= (uint32_t)kAdamSegment) break;
    n = (n + (uint32_t)kAdamSegment - 1u) / (uint32_t)kAdamSegment;
  }
  L.total = o;
  return L;
}

struct AdamNormParams {
  AdamFlat flat;
  double* part;  // level 0
};

struct AdamMidParams {
  const double* in;
  uint32_t n_in;
  double* out;
};

struct AdamUpdateParams {
  PolicyDims d;
  AdamConsts c;
  const double* part;  // the last level
  uint32_t n_part;     // <= 1024
  const AdamState* state;
  PolicyTensors<const float*> g;  // gradients
  PolicyTensors<float*> p, m, v;  // parameters, exp_avg, exp_avg_sq
  uint16_t* w;  // the policy's packed bf16 image
  float* b;     // its padded biases
};

struct AdamFinishParams {
  AdamConsts c;
  const double* part;
  uint32_t n_part;
  AdamState* state;
};

// the kernels (wab_policy_opt.hip), launched from wab_capi_policy.hip
__global__ void wab_adam_norm_kernel(AdamNormParams p);
__global__ void wab_adam_mid_kernel(AdamMidParams p);
__global__ void wab_adam_update_kernel(AdamUpdateParams p);
__global__ void wab_adam_finish_kernel(AdamFinishParams p);

}  // namespace wab
