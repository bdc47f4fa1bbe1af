// wab_policy_dev.h — the device policy's forward pass, stated once for its three users:
// wab_policy_kernel (wab_policy.hip), the policy build of the multi-step small kernel
// (wab_step_small.hip, wab_rollout_policy) and wab_policy_bwd_kernel (wab_policy_grad.hip): the
// bf16 rounding, the row staging, the fragment loads, the layer-1 chunk loop, the tile pass of
// the later layers, the layer epilogue and the head / softmax / draw tail.  A kernel adds only
// what is its own, as callables: how it stages a chunk, its barrier, what else it does with a
// finished element.  All three compute through these, so they agree bit for bit: an MFMA column
// depends only on its own env's operand, whatever the number MT of 32-env tiles a workgroup
// takes a weight tile through.
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

template <int MT>
__device__ __forceinline__ void pol_zero(pol_f32x16 (&acc)[MT]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[mt][i] = 0.0f;
}

// bias, leaky_relu (and the clamp after layer 3), bf16, into the next layer's LDS image: register
// group g of a lane holds units 32 tile + 8 g + 4 (lane >> 5) + 0..3 of env 32 mt + (lane & 31).
// hook(g, mt, i, unit, row, z >= 0, inside the clamp, the bf16 bits) sees every element once
// (the gradient kernel's masks and workspace column)
template <bool CLAMP, int MT, class Hook>
__device__ __forceinline__ void pol_store(const pol_f32x16 (&acc)[MT], const float* __restrict__ bias, int tile,
                                          uint16_t* xn, int pitch, int lane, Hook hook) {
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
        const bool pos = v >= 0.0f;
        v = pos ? v : 0.01f * v;
        const bool inside = !CLAMP || (v >= -4.0f && v <= 4.0f);
        if (CLAMP) v = fminf(fmaxf(v, -4.0f), 4.0f);
        o[i] = pol_bf16(v);
        hook(g, mt, i, n + i, mt * 32 + r, pos, inside, o[i]);
      }
      uint2 w;
      w.x = o[0] | (o[1] << 16);
      w.y = o[2] | (o[3] << 16);
      *reinterpret_cast<uint2*>(xn + (size_t)(mt * 32 + r) * (size_t)pitch + (size_t)n) = w;
    }
  }
}

template <bool CLAMP, int MT>
__device__ __forceinline__ void pol_store(const pol_f32x16 (&acc)[MT], const float* __restrict__ bias, int tile,
                                          uint16_t* xn, int pitch, int lane) {
  pol_store<CLAMP>(acc, bias, tile, xn, pitch, lane, [](int, int, int, int, int, bool, bool, uint32_t) {});
}

// Columns [k0, k0 + kn) of ROWS float32 rows of F columns (n_env of them inside the batch) as bf16
// into x[ROWS][pitch]: wave w takes rows w, w + 4, ..., a lane one column of 16 rows at a time,
// the 16 loads issued together (addresses clamped into the batch, so none is conditional; rows
// past the batch and the pad columns are stored as zeros).  each(e, k, v, inside) sees every
// element after its store, with whether it is inside the array.
// src(j, e) is where tile row e = wave + 4 j starts, in floats from `rows`: the overload below
// takes the rows as they lie; a caller with an index hands in its own (wave-uniform: it depends on
// the wave and j alone).
template <int ROWS, class Src, class Each>
__device__ __forceinline__ void pol_stage_rows(const float* __restrict__ rows, int F, int n_env, int k0, int kn,
                                               uint16_t* x, int pitch, int wave, int lane, Src src, Each each) {
  for (int kl = lane; kl < kn; kl += 64) {
    const int k = k0 + kl;
    const bool kin = k < F;
    const float* col = rows + (size_t)(kin ? k : F - 1);
    constexpr int kRows = 16;  // (32 in flight measured the same: 55.9-56.2 against 55.8-56.0 us)
    for (int eb = 0; eb < ROWS / 4; eb += kRows) {
      float v[kRows];
#pragma unroll
      for (int i = 0; i < kRows; ++i) {
        const int e = wave + 4 * (eb + i);
        v[i] = col[src(eb + i, e)];
      }
#pragma unroll
      for (int i = 0; i < kRows; ++i) {
        const int e = wave + 4 * (eb + i);
        const bool in = kin && e < n_env;
        x[(size_t)e * (size_t)pitch + (size_t)kl] = (uint16_t)(in ? pol_bf16(v[i]) : 0u);
        each(e, k, v[i], in);
      }
    }
  }
}

template <int ROWS, class Each>
__device__ __forceinline__ void pol_stage_rows(const float* __restrict__ rows, int F, int n_env, int k0, int kn,
                                               uint16_t* x, int pitch, int wave, int lane, Each each) {
  pol_stage_rows<ROWS>(rows, F, n_env, k0, kn, x, pitch, wave, lane,
                       [=](int, int e) { return (size_t)(e < n_env ? e : n_env - 1) * (size_t)F; }, each);
}

// Layer 1: the input in chunks of L.KC columns through the LDS image x (region A); wave w keeps
// tiles w and (TWO) w + 4 of all MT env tiles in accumulators across the chunks (k-steps
// ascending).  Per chunk: the chunk's fragments requested, barrier() once the last chunk's rows
// have been read, stage(k0, kn) writes the chunk's kn columns (a multiple of 16) as bf16 rows,
// barrier(), the MFMAs.  store(acc, tile, j) takes each finished tile (j = 0: w, 1: w + 4).
template <int MT, bool TWO, class Stage, class Barrier, class Store>
__device__ __forceinline__ void pol_layer1(const PolicyDims& d, const PolicyLds& L, const uint4* __restrict__ wimg,
                                           const uint16_t* x, int wave, int lane, Stage stage, Barrier barrier,
                                           Store store) {
  pol_f32x16 acc0[MT], acc1[MT];
  pol_zero(acc0);
  if (TWO) pol_zero(acc1);
  const int KC = L.KC, pitch_in = L.pitch_in;
  const int kpad = 16 * d.KS1;
  uint4 wf[kPolicyMaxKs];
  const uint4* const w1t = wimg + (d.w1 >> 3) + (size_t)wave * (size_t)d.KS1 * 64u + (size_t)lane;
  for (int c = 0; c < L.n_chunks; ++c) {
    const int k0 = c * KC;
    const int kn = kpad - k0 < KC ? kpad - k0 : KC;
    const int ks0 = k0 >> 4, nks = kn >> 4;
    if (wave < d.NT1) pol_load_frags(wf, w1t + (size_t)ks0 * 64u, nks);
    if (c > 0) barrier();
    stage(k0, kn);
    barrier();
    const uint16_t* xl = x + (size_t)(lane & 31) * (size_t)pitch_in + 8 * (lane >> 5);
    if (wave < d.NT1) pol_mma(acc0, wf, nks, xl, pitch_in);
    if (TWO && wave + 4 < d.NT1) {
      pol_load_frags(wf, w1t + ((size_t)4 * (size_t)d.KS1 + (size_t)ks0) * 64u, nks);
      pol_mma(acc1, wf, nks, xl, pitch_in);
    }
  }
  if (wave < d.NT1) store(acc0, wave, 0);
  if (TWO && wave + 4 < d.NT1) store(acc1, wave + 4, 1);
}

// A layer past the first, forward or backward: wave w takes tiles w and w + 4 (of NT, KS k-steps
// each, fragments from wimg) through all MT env tiles of xin and hands each accumulator to
// store(acc, tile, j).  EARLY (act, rollout): wf holds tile w's fragments, requested by the
// caller before the barrier, and the tiles are a loop.  Otherwise (the gradient kernel) every
// tile's fragments are loaded here, after the barrier, and the two tiles are unrolled, so that j
// is a constant where the store picks its mask registers.
template <int MT, bool EARLY, class Store>
__device__ __forceinline__ void pol_layer(uint4 (&wf)[kPolicyMaxKs], const uint4* __restrict__ wimg, int NT, int KS,
                                          const uint16_t* xin, int pitch_in, int wave, int lane, Store store) {
  const uint16_t* const x = xin + (size_t)(lane & 31) * (size_t)pitch_in + 8 * (lane >> 5);
  const auto tile = [&](int t, int j, bool load) {
    if (load) pol_load_frags(wf, wimg + (size_t)t * (size_t)KS * 64u + (size_t)lane, KS);
    pol_f32x16 acc[MT];
    pol_zero(acc);
    pol_mma(acc, wf, KS, x, pitch_in);
    store(acc, t, j);
  };
  if constexpr (EARLY) {
    for (int t = wave; t < NT; t += 4) tile(t, (t - wave) >> 2, t != wave);
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (wave + 4 * j < NT) tile(wave + 4 * j, j, true);
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

// The softmax and the value of env column r = lane & 31 from the head tile's accumulator (every
// lane of the wave must call: lane (r, 0) takes rows 4..7 from lane (r, 1), and only lanes 0..31
// hold a whole column): z_k = logit_k - max, e_k = expf(z_k) (0 for k >= A), s their sum over
// k = 0, 1, ... in order, inv = 1 / s; p_k = e_k * inv.
// SCALED (the act and rollout heads, under the policy's action rule): logit_k is first replaced by
// fl32((logit_k + bias_k) * inv_tau), one rounding of its own, inv_tau = 1 / temperature from the
// host (1.0f leaves every bit).  The gradient and evaluate kernels take the unscaled form.
struct PolSoftmax {
  float val, z[kPolicyMaxActions], e[kPolicyMaxActions], s, inv;
};
template <bool SCALED>
__device__ __forceinline__ PolSoftmax pol_softmax_of(const pol_f32x16& acc, int lane, const float* __restrict__ bh, int A,
                                                     float inv_tau) {
  // lane (r, h) holds rows 4 h + 0..3 in registers 0..3 and rows 8 + 4 h + 0..3 in registers 4..7
  // of env column r
  PolSoftmax q;
  float lg[kPolicyMaxActions];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lg[i] = acc[i];
    lg[4 + i] = __shfl(acc[i], (lane + 32) & 63, 64);
  }
  q.val = acc[4] + bh[kPolicyMaxActions];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kPolicyMaxActions; ++k) {
    lg[k] = lg[k] + bh[k];
    if constexpr (SCALED) lg[k] = __fmul_rn(lg[k], inv_tau);
    if (k < A) m = fmaxf(m, lg[k]);
  }
  q.s = 0.0f;
#pragma unroll
  for (int k = 0; k < kPolicyMaxActions; ++k) {
    q.z[k] = lg[k] - m;
    q.e[k] = k < A ? expf(q.z[k]) : 0.0f;
    if (k < A) q.s = q.s + q.e[k];
  }
  q.inv = 1.0f / q.s;
  return q;
}
__device__ __forceinline__ PolSoftmax pol_softmax(const pol_f32x16& acc, int lane, const float* __restrict__ bh, int A) {
  return pol_softmax_of<false>(acc, lane, bh, A, 1.0f);
}

// The tail on the head tile's accumulator: softmax (of the logits scaled by inv_tau), value and
// the action of env column r = lane & 31 under the policy's action rule (`mode`, uniform: the
// keyed draw, or kActGreedy, the first maximum of the probabilities as written, no draw made),
// finished by the lanes 0..31 for which `sampler` holds (every lane of the wave
// must call).  `env` is the env's index in the handle (the row of actions / value / probs),
// env_base + env its global id; episode and turn are the env's current ones.  Returns the action
// (of a sampler lane; -1 otherwise).
__device__ __forceinline__ int pol_sample(const pol_f32x16& acc, int lane, bool sampler, const float* __restrict__ bh,
                                          int A, float inv_tau, int mode, uint64_t seed, int64_t env_base, int64_t env,
                                          uint32_t episode, uint32_t turn, int8_t* actions, float* probs,
                                          float* value) {
  const PolSoftmax q = pol_softmax_of<true>(acc, lane, bh, A, inv_tau);
  if (!sampler) return -1;
  const bool greedy = mode == kActGreedy;
  double u = 0.0;
  if (!greedy) {
    // the keyed draw (oracle/keyed_rng.py): site 11, the env's episode and turn, tile (0, 0), k = 0
    const uint64_t ek = episode_key(seed, (uint64_t)(env_base + env), (uint64_t)episode);
    const uint64_t U = draw_U(0u, make_ts(SITE_POLICY, 0u, (int32_t)turn), (uint32_t)ek, (uint32_t)(ek >> 32));
    u = (double)U * 0x1p-53;
  }
  double c = 0.0;
  float best = 0.0f;
  int a = 0;
#pragma unroll
  for (int k = 0; k < kPolicyMaxActions; ++k) {
    const float pk = q.e[k] * q.inv;
    if (k < A) {
      if (probs) probs[(size_t)env * (size_t)A + (size_t)k] = pk;
      if (greedy) {
        // ties to the lowest index; a NaN never compares greater, so a row of NaNs gives 0
        if (k == 0) best = pk;
        else if (pk > best) { best = pk; a = k; }
      } else {
        c = c + (double)pk;
        if (k < A - 1 && c <= u) a += 1;
      }
    }
  }
  actions[env] = (int8_t)a;
  if (value) value[env] = q.val;
  return a;
}

}  // namespace wab
