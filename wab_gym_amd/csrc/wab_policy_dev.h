// wab_policy_dev.h — the device policy's building blocks, shared by wab_policy_kernel
// (wab_policy.hip) and the policy build of the multi-step small kernel (wab_step_small.hip,
// wab_rollout_policy): the bf16 rounding, the fragment loads, the MFMA passes, the layer
// epilogue and the head / softmax / draw tail.  Both kernels compute through these, so they
// agree bit for bit: an MFMA column depends only on its own env's operand, whatever the number
// MT of 32-env tiles a workgroup takes a weight tile through.
#pragma once

#include <hip/hip_runtime.h>

#include "wab_policy.h"
#include "wab_device.h"

namespace wab {

typedef __bf16 pol_bf16x8 __attribute__((ext_vector_type(8)));
typedef float pol_f32x16 __attribute__((ext_vector_type(16)));

// float32 -> bf16 bits, round to nearest even (NaN -> the quiet NaN 0x7FC0, as torch does)
__host__ __device__ inline uint32_t pol_bf16(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
  u += 0x7FFFu + ((u >> 16) & 1u);
  return u >> 16;
}

__device__ __forceinline__ pol_bf16x8 pol_frag(uint4 v) { return __builtin_bit_cast(pol_bf16x8, v); }

// A tile's weight fragments of one pass (at most kPolicyMaxKs k-steps: KC <= 256, widths <= 256)
// are all requested at once, before the work that precedes their use (layer 1: the chunk's
// feature loads; later layers: the barrier), so that their L2 latency is not paid per k-step:
// four k-steps of MFMAs are ~0.2 us, less than one L2 round trip.  wfrag points at this lane's
// 16 bytes of the first fragment (fragments 64 uint4 apart).
constexpr int kPolicyMaxKs = 16;
__device__ __forceinline__ void pol_load_frags(uint4 (&wf)[kPolicyMaxKs], const uint4* __restrict__ wfrag, int nks) {
#pragma unroll
  for (int i = 0; i < kPolicyMaxKs; ++i) {
    wf[i] = make_uint4(0u, 0u, 0u, 0u);
    if (i < nks) wf[i] = wfrag[(size_t)i * 64u];  // (uniform)
  }
}

// acc[mt] += W(tile, the pass's nks k-steps) * X(32-env tile mt): x points at this lane's 16 bytes
// of k-step 0 of env tile 0 (row r = lane & 31, column 8 (lane >> 5)); env tiles are 32 * pitch
// elements apart
template <int MT>
__device__ __forceinline__ void pol_mma(pol_f32x16 (&acc)[MT], const uint4 (&wf)[kPolicyMaxKs], int nks,
                                        const uint16_t* x, int pitch) {
#pragma unroll
  for (int i = 0; i < kPolicyMaxKs; ++i) {
    if (i < nks) {  // (uniform)
      pol_bf16x8 b[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        b[mt] = pol_frag(*reinterpret_cast<const uint4*>(x + (size_t)(mt * 32) * (size_t)pitch + (size_t)(i * 16)));
      const pol_bf16x8 a = pol_frag(wf[i]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[mt], acc[mt], 0, 0, 0);
    }
  }
}

// bias, leaky_relu (and the clamp after layer 3), bf16, into the next layer's LDS image: register
// group g of a lane holds units 32 tile + 8 g + 4 (lane >> 5) + 0..3 of env 32 mt + (lane & 31)
template <bool CLAMP, int MT>
__device__ __forceinline__ void pol_store(const pol_f32x16 (&acc)[MT], const float* __restrict__ bias, int tile,
                                          uint16_t* xn, int pitch, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int n = 32 * tile + 8 * g + 4 * h;
    const float4 bv = *reinterpret_cast<const float4*>(bias + n);
    const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      uint32_t o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = acc[mt][4 * g + i] + bb[i];
        v = v >= 0.0f ? v : 0.01f * v;
        if (CLAMP) v = fminf(fmaxf(v, -4.0f), 4.0f);
        o[i] = pol_bf16(v);
      }
      uint2 w;
      w.x = o[0] | (o[1] << 16);
      w.y = o[2] | (o[3] << 16);
      *reinterpret_cast<uint2*>(xn + (size_t)(mt * 32 + r) * (size_t)pitch + (size_t)n) = w;
    }
  }
}

template <int MT>
__device__ __forceinline__ void pol_zero(pol_f32x16 (&acc)[MT]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.0f;
}

// a hidden layer past the first: wave w takes tiles w and w + 4 through all MT env tiles; wf holds
// tile w's fragments, requested by the caller before the barrier
template <bool CLAMP, int MT>
__device__ __forceinline__ void pol_layer(uint4 (&wf)[kPolicyMaxKs], const uint4* __restrict__ wimg,
                                          const float* __restrict__ bias, int NT, int KS, const uint16_t* xin,
                                          int pitch_in, uint16_t* xout, int pitch_out, int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
  for (int t = wave; t < NT; t += 4) {
    if (t != wave) pol_load_frags(wf, wimg + (size_t)t * (size_t)KS * 64u + (size_t)lane, KS);
    pol_f32x16 acc[MT];
    pol_zero(acc);
    pol_mma(acc, wf, KS, xin + (size_t)r * (size_t)pitch_in + 8 * h, pitch_in);
    pol_store<CLAMP>(acc, bias, t, xout, pitch_out, lane);
  }
}

// the head tile (rows 0..7 action logits, row 8 the value) on this lane's env column: x points at
// the lane's 16 bytes of k-step 0 of its env's X3 row
__device__ __forceinline__ pol_f32x16 pol_head_mma(const uint4 (&wf)[kPolicyMaxKs], int nks, const uint16_t* x) {
  pol_f32x16 acc = {};
#pragma unroll
  for (int i = 0; i < kPolicyMaxKs; ++i) {
    if (i < nks) {  // (uniform)
      const pol_bf16x8 b = pol_frag(*reinterpret_cast<const uint4*>(x + (size_t)(i * 16)));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pol_frag(wf[i]), b, acc, 0, 0, 0);
    }
  }
  return acc;
}

// The tail on the head tile's accumulator: softmax, value and the keyed draw of env column
// r = lane & 31, finished by the lanes 0..31 for which `sampler` holds (every lane of the wave
// must call: lane (r, 0) takes rows 4..7 from lane (r, 1)).  `env` is the env's index in the
// handle (the row of actions / value / probs), env_base + env its global id; episode and turn
// are the env's current ones.  Returns the action (of a sampler lane; -1 otherwise).
__device__ __forceinline__ int pol_sample(const pol_f32x16& acc, int lane, bool sampler, const float* __restrict__ bh,
                                          int A, uint64_t seed, int64_t env_base, int64_t env, uint32_t episode,
                                          uint32_t turn, int8_t* actions, float* probs, float* value) {
  // lane (r, h) holds rows 4 h + 0..3 in registers 0..3 and rows 8 + 4 h + 0..3 in registers 4..7
  // of env column r
  float lg[kPolicyMaxActions];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lg[i] = acc[i];
    lg[4 + i] = __shfl(acc[i], (lane + 32) & 63, 64);
  }
  if (!sampler) return -1;
  const float val = acc[4] + bh[kPolicyMaxActions];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kPolicyMaxActions; ++k) {
    lg[k] = lg[k] + bh[k];
    if (k < A) m = fmaxf(m, lg[k]);
  }
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < kPolicyMaxActions; ++k) {
    lg[k] = k < A ? expf(lg[k] - m) : 0.0f;
    if (k < A) s = s + lg[k];
  }
  const float inv = 1.0f / s;
  // the keyed draw (oracle/keyed_rng.py): site 11, the env's episode and turn, tile (0, 0), k = 0
  const uint64_t ek = episode_key(seed, (uint64_t)(env_base + env), (uint64_t)episode);
  const uint64_t U = draw_U(0u, make_ts(SITE_POLICY, 0u, (int32_t)turn), (uint32_t)ek, (uint32_t)(ek >> 32));
  const double u = (double)U * 0x1p-53;
  double c = 0.0;
  int a = 0;
#pragma unroll
  for (int k = 0; k < kPolicyMaxActions; ++k) {
    const float pk = lg[k] * inv;
    if (k < A) {
      if (probs) probs[(size_t)env * (size_t)A + (size_t)k] = pk;
      c = c + (double)pk;
      if (k < A - 1 && c <= u) a += 1;
    }
  }
  actions[env] = (int8_t)a;
  if (value) value[env] = val;
  return a;
}

}  // namespace wab
