// wab_policy.h — parameter blocks and the packed-weight layout of the device policy
// (wab_policy.hip; wab_policy_* in include/wab.h), shared with the C-ABI host code.
#pragma once

#include "wab_build_guard.h"

#include <stdint.h>

namespace wab {

constexpr int kPolicyEnvs = 128;     // envs per workgroup: every weight fragment is read once per 128 envs
constexpr int kPolicyMaxWidth = 256; // hidden widths h1, h2, h3
constexpr int kPolicyMaxActions = 8;
constexpr int kPolicyMaxChunk = 256; // input features staged per pass (columns of the LDS chunk)
constexpr uint32_t SITE_POLICY = 11; // keyed-RNG site of the action draw (first id free in oracle/keyed_rng.py)
constexpr int32_t kActSample = 0, kActGreedy = 1;  // WAB_ACT_* (include/wab.h): the action rule's modes

// Packed weights: one layer is NT x KS fragments of 64 lanes x 8 bf16 (1 KB each), fragment
// (nt, ks) at ((nt * KS + ks) * 64 + lane) * 8: lane l holds W[32 nt + (l & 31)][16 ks + 8 (l >> 5)
// + j], j = 0..7 (the A operand of v_mfma_f32_32x32x16_bf16), zero outside [out, in).  The head
// layer is one tile: rows 0..7 the action head (rows >= n_actions zero), row 8 the value head.
// Biases are fp32, padded with zeros to 32 NT (head: [0, 8) actions, [8] value).
struct PolicyDims {
  int32_t F, h1, h2, h3, A;
  int32_t KS1, KS2, KS3, KS4;  // k-steps of 16: ceil(F / 16), ceil(h1 / 16), ceil(h2 / 16), ceil(h3 / 16)
  int32_t NT1, NT2, NT3;       // 32-unit tiles: ceil(h / 32)
  // element offsets into the image (uint16 units for w*, float units for b*, from their own bases)
  uint32_t w1, w2, w3, wh, w_total;
  uint32_t b1, b2, b3, bh, b_total;
};

__host__ __device__ inline PolicyDims policy_dims(int F, int h1, int h2, int h3, int A) {
  PolicyDims d;
  d.F = F; d.h1 = h1; d.h2 = h2; d.h3 = h3; d.A = A;
  d.KS1 = (F + 15) / 16; d.KS2 = (h1 + 15) / 16; d.KS3 = (h2 + 15) / 16; d.KS4 = (h3 + 15) / 16;
  d.NT1 = (h1 + 31) / 32; d.NT2 = (h2 + 31) / 32; d.NT3 = (h3 + 31) / 32;
  uint32_t o = 0;
  d.w1 = o; o += (uint32_t)(d.NT1 * d.KS1) * 512u;
  d.w2 = o; o += (uint32_t)(d.NT2 * d.KS2) * 512u;
  d.w3 = o; o += (uint32_t)(d.NT3 * d.KS3) * 512u;
  d.wh = o; o += (uint32_t)d.KS4 * 512u;
  d.w_total = o;
  o = 0;
  d.b1 = o; o += (uint32_t)d.NT1 * 32u;
  d.b2 = o; o += (uint32_t)d.NT2 * 32u;
  d.b3 = o; o += (uint32_t)d.NT3 * 32u;
  d.bh = o; o += 32u;
  d.b_total = o;
  return d;
}

// LDS of the forward pass for a workgroup of `envs` envs: region A holds the input chunk
// [envs][KC + 8] bf16 during layer 1, then X2 [envs][32 NT2 + 8]; region B holds X1, then X3.  Row
// pitches are an odd number of 16-byte units, so the 16-byte fragment reads of 8 consecutive rows
// hit 8 different bank groups.  The one derivation for wab_policy_kernel, wab_policy_bwd_kernel
// (GradPlan) and the rollout's policy phase (RollPolicy, behind the step's own LDS).
struct PolicyLds {
  int32_t KC, n_chunks;               // columns per chunk (a multiple of 16), chunks
  int32_t pitch_in, pitch1, pitch2, pitch3;  // elements
  uint32_t off_b;                     // byte offset of region B
  uint32_t total;                     // bytes
};

constexpr uint32_t kPolicyLdsBudget = 80u * 1024u;  // act, grad: two workgroups per CU
constexpr uint32_t kPolicyLdsNoBudget = 0xFFFFFFFFu;  // rollout: chunks of kPolicyMaxChunk, whatever their bytes

// `budget`: the bytes the chunk is sized to together with region B (at least X2's bytes, which
// region A holds anyway, at least one k-step, at most kPolicyMaxChunk columns)
__host__ __device__ inline PolicyLds policy_lds(const PolicyDims& d, int envs, uint32_t budget) {
  PolicyLds L;
  L.pitch1 = 32 * d.NT1 + 8;
  L.pitch2 = 32 * d.NT2 + 8;
  L.pitch3 = 32 * d.NT3 + 8;
  const uint32_t rows = (uint32_t)envs * 2u;  // bytes per element column
  const uint32_t region_b = rows * (uint32_t)(L.pitch1 > L.pitch3 ? L.pitch1 : L.pitch3);
  const uint32_t x2 = rows * (uint32_t)L.pitch2;
  budget = region_b < budget ? budget - region_b : 0u;
  if (budget < x2) budget = x2;
  int kc_max = ((int)(budget / rows) - 8) / 16 * 16;
  if (kc_max < 16) kc_max = 16;
  if (kc_max > kPolicyMaxChunk) kc_max = kPolicyMaxChunk;
  const int kpad = 16 * d.KS1;
  L.n_chunks = (kpad + kc_max - 1) / kc_max;
  L.KC = ((kpad + L.n_chunks - 1) / L.n_chunks + 15) / 16 * 16;
  L.pitch_in = L.KC + 8;
  const uint32_t chunk = rows * (uint32_t)L.pitch_in;
  L.off_b = chunk > x2 ? chunk : x2;
  L.total = L.off_b + region_b;
  return L;
}

struct PolicyParams {
  PolicyDims d;
  PolicyLds lds;
  uint64_t seed;
  int64_t env_base, B;
  const uint4* hdr;          // the handle's [B] {tile, turn, misc, episode}
  const float* features;     // [B][F]
  int8_t* actions;           // [B]
  float* probs;              // [B][A] or null
  float* value;              // [B] or null
  const uint16_t* w;         // packed bf16 image (PolicyDims::w*)
  const float* b;            // packed biases (PolicyDims::b*)
  float inv_tau;             // the action rule (wab_policy_set_action_rule): 1 / temperature,
  int32_t act_mode;          //   kActSample or kActGreedy
};

// A set of the policy's ten tensors (wab_policy_weights' fields, in its order): torch Linear
// layout, device.  Kernels name the field they mean; no device code indexes a set.
template <class P>
struct PolicyTensors {
  P w1, b1, w2, b2, w3, b3, wa, ba, wv, bv;
};

struct PolicyPackParams {
  PolicyDims d;
  PolicyTensors<const float*> src;
  uint16_t* w;
  float* b;
};

// the kernels (wab_policy.hip), launched from wab_capi_policy.hip
__global__ void wab_policy_pack(PolicyPackParams p);
template <bool TWO>
__global__ void wab_policy_kernel(PolicyParams p);

}  // namespace wab
