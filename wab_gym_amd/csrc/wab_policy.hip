// wab_policy.hip — the actor-critic policy of actor_critic.py:54-97 for inference, with the
// action sampled in the same launch (wab_policy_act), and the weight pack kernel
// (wab_policy_load).  gfx950.
//
// Network: three Linear + leaky_relu(0.01) layers, clamp(-4, 4) after the third, a softmax
// action head and a one-unit value head; F >= 1 inputs, widths h1, h2, h3 in 1..256, A = 2..8
// actions, all runtime (zero padding to the MFMA tile).
//
// Numeric contract (wab_gym_amd/policy_reference.py reference_forward states the same in torch):
//   * every matmul operand is bf16, rounded to nearest even: the input features, the weights
//     (once, by the pack kernel) and the hidden activations after bias, leaky_relu and clamp;
//   * products are accumulated in fp32 by v_mfma_f32_32x32x16_bf16 (the order of the sum is the
//     instruction's; k-steps of 16 in ascending order);
//   * bias add, leaky_relu (x >= 0 ? x : 0.01f * x), clamp, the softmax (max-subtracted, expf,
//     the sum over k = 0, 1, ... in order, one divide 1 / sum, p_k = e_k * that) and the value
//     are fp32; features that are 0 or 1 (wab_step_features) are exact in bf16;
//   * the reference's + U(0, 1) / 100 input noise (actor_critic.py:189) is not reproduced.
// Sampling: u = U * 2^-53, U the 53-bit keyed draw of (seed, global env id, the env's current
// episode, site 11, the env's current turn, x = 0, y = 0, k = 0), episode and turn read from the
// handle's state; action = #{k < A - 1 : c_k <= u}, c_k the running sum in double, k = 0, 1, ...,
// of the fp32 probabilities written out: an exact function of probs and u.
// Action rule (wab_policy_set_action_rule; PolicyParams::inv_tau, act_mode): the logits, bias
// included, are first multiplied by inv_tau = 1.0f / temperature, rounded once (1.0f: no bit
// changes); kActGreedy takes the first maximum of the probabilities written out in place of the
// draw (ties to the lowest index, a row of NaNs gives 0).
//
// Shape: a workgroup of four waves takes 128 envs.  The input features are staged in LDS as
// bf16 in chunks of KC columns (PolicyLds), each wave loading rows with one dword per lane
// (rows are 4-byte aligned only; consecutive lanes read consecutive columns).  In the hidden
// layers the waves split the 32-unit output tiles (tile t on wave t & 3) and each takes all four
// 32-env tiles through it, so every weight fragment (one coalesced 16-byte load per lane from
// the packed image, L2-resident) is read once per 128 envs; a pass's fragments are all requested
// before the feature loads or the barrier that precede their use (pol_load_frags).  Units are the MFMA's rows and envs
// its columns: a lane then holds four consecutive units of one env per register group, which it
// stores to the next layer's LDS image as one 8-byte word.  The heads are one tile; each wave
// takes it for its own 32 envs and lanes 0..31 finish the softmax and the draw.
#include <hip/hip_runtime.h>

#include "wab_policy_dev.h"

namespace wab {

// ------------------------------------------------------------------------ weight pack
__device__ __forceinline__ void pack_layer(const float* __restrict__ W, int N, int K, int KS,
                                           uint16_t* __restrict__ dst, uint32_t i) {
  // i indexes the layer's image: ((nt * KS + ks) * 64 + lane) * 8 + j
  const uint32_t j = i & 7u, lane = (i >> 3) & 63u, f = i >> 9;
  const int nt = (int)(f / (uint32_t)KS), ks = (int)(f % (uint32_t)KS);
  const int n = 32 * nt + (int)(lane & 31u), k = 16 * ks + 8 * (int)(lane >> 5) + (int)j;
  dst[i] = (uint16_t)((n < N && k < K) ? pol_bf16(W[(size_t)n * (size_t)K + (size_t)k]) : 0u);
}

__global__ __launch_bounds__(256) void wab_policy_pack(PolicyPackParams p) {
  const PolicyDims& d = p.d;
  const uint32_t stride = gridDim.x * 256u;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < d.w_total; i += stride) {
    if (i < d.w2) pack_layer(p.src.w1, d.h1, d.F, d.KS1, p.w + d.w1, i - d.w1);
    else if (i < d.w3) pack_layer(p.src.w2, d.h2, d.h1, d.KS2, p.w + d.w2, i - d.w2);
    else if (i < d.wh) pack_layer(p.src.w3, d.h3, d.h2, d.KS3, p.w + d.w3, i - d.w3);
    else {
      // the head tile: rows 0 .. A-1 of the action head, row 8 the value head
      const uint32_t e = i - d.wh, j = e & 7u, lane = (e >> 3) & 63u, ks = e >> 9;
      const int n = (int)(lane & 31u), k = 16 * (int)ks + 8 * (int)(lane >> 5) + (int)j;
      float v = 0.0f;
      if (k < d.h3) {
        if (n < d.A) v = p.src.wa[(size_t)n * (size_t)d.h3 + (size_t)k];
        else if (n == kPolicyMaxActions) v = p.src.wv[k];
      }
      p.w[i] = (uint16_t)pol_bf16(v);
    }
  }
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < d.b_total; i += stride) {
    float v = 0.0f;
    if (i < d.b2) { if ((int)(i - d.b1) < d.h1) v = p.src.b1[i - d.b1]; }
    else if (i < d.b3) { if ((int)(i - d.b2) < d.h2) v = p.src.b2[i - d.b2]; }
    else if (i < d.bh) { if ((int)(i - d.b3) < d.h3) v = p.src.b3[i - d.b3]; }
    else {
      const int n = (int)(i - d.bh);
      if (n < d.A) v = p.src.ba[n];
      else if (n == kPolicyMaxActions) v = p.src.bv[0];
    }
    p.b[i] = v;
  }
}

// ------------------------------------------------------------------------ forward + sample
// TWO: h1 > 128, a wave holds two layer-1 tiles across the chunks (64 more accumulator registers:
// that instance takes one wave per SIMD's registers, the common one stays at two)
template <bool TWO>
__global__ __launch_bounds__(256, TWO ? 1 : 2) void wab_policy_kernel(PolicyParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pol_smem[];
  uint16_t* const regA = reinterpret_cast<uint16_t*>(pol_smem);
  uint16_t* const regB = reinterpret_cast<uint16_t*>(pol_smem + p.lds.off_b);
  const PolicyDims& d = p.d;
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int64_t env0 = (int64_t)blockIdx.x * kPolicyEnvs;
  const int n_env = (int)(p.B - env0 < kPolicyEnvs ? p.B - env0 : kPolicyEnvs);
  const uint4* const wimg = reinterpret_cast<const uint4*>(p.w);

  // the sampling lane's env header, asked for early (lanes 0..31 of wave w: env 32 w + lane)
  const int my_env = 32 * wave + r;
  const bool sampler = h == 0 && my_env < n_env;
  uint4 hdr = make_uint4(0u, 0u, 0u, 0u);
  if (sampler) hdr = p.hdr[env0 + my_env];

  // ---- layer 1: chunks of KC input columns through region A -> X1 (region B)
  pol_layer1<4, TWO>(
      d, p.lds, wimg, regA, wave, lane,
      [&](int k0, int kn) {
        pol_stage_rows<kPolicyEnvs>(p.features + (size_t)env0 * (size_t)d.F, d.F, n_env, k0, kn, regA, p.lds.pitch_in,
                                    wave, lane, [](int, int, float, bool) {});
      },
      [] { __syncthreads(); },
      [&](const pol_f32x16(&acc)[4], int t, int) { pol_store<false>(acc, p.b + d.b1, t, regB, p.lds.pitch1, lane); });
  uint4 wf[kPolicyMaxKs];
  const uint4* const w2 = wimg + (d.w2 >> 3), * const w3 = wimg + (d.w3 >> 3);
  if (wave < d.NT2) pol_load_frags(wf, w2 + (size_t)wave * (size_t)d.KS2 * 64u + (size_t)lane, d.KS2);
  __syncthreads();  // X1 complete; region A free

  // ---- layer 2: X1 (region B) -> X2 (region A); layer 3: X2 -> X3 (region B), clamped
  pol_layer<4, true>(wf, w2, d.NT2, d.KS2, regB, p.lds.pitch1, wave, lane, [&](const pol_f32x16(&acc)[4], int t, int) {
    pol_store<false>(acc, p.b + d.b2, t, regA, p.lds.pitch2, lane);
  });
  if (wave < d.NT3) pol_load_frags(wf, w3 + (size_t)wave * (size_t)d.KS3 * 64u + (size_t)lane, d.KS3);
  __syncthreads();
  pol_layer<4, true>(wf, w3, d.NT3, d.KS3, regA, p.lds.pitch2, wave, lane, [&](const pol_f32x16(&acc)[4], int t, int) {
    pol_store<true>(acc, p.b + d.b3, t, regB, p.lds.pitch3, lane);
  });
  pol_load_frags(wf, wimg + (d.wh >> 3) + (size_t)lane, d.KS4);
  __syncthreads();

  // ---- heads: one tile (rows 0..7 action logits, row 8 the value), wave w on envs 32 w ..
  const pol_f32x16 acc = pol_head_mma(wf, d.KS4, regB + (size_t)(32 * wave + r) * (size_t)p.lds.pitch3 + 8 * h);
  pol_sample(acc, lane, sampler, p.b + d.bh, d.A, p.inv_tau, p.act_mode, p.seed, p.env_base, env0 + my_env, hdr.w, hdr.y,
             p.actions, p.probs, p.value);
}

template __global__ void wab_policy_kernel<false>(PolicyParams p);
template __global__ void wab_policy_kernel<true>(PolicyParams p);

}  // namespace wab
