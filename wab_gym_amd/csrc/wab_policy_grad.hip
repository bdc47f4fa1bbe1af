// wab_policy_grad.hip — finish_episode()'s loss and loss.backward() of actor_critic.py:148-165
// for the device policy: the loss terms and the gradients of the ten parameter tensors over N
// stored rows (features, action, weight, value target).  gfx950.
//
// Numeric contract (wab_gym_amd/policy_reference.py reference_loss_and_grad states the same in torch):
//   * forward: wab_policy_act's, through the same pol_* functions (wab_policy_dev.h): the layer-1
//     chunk loop, the tile passes, pol_store (the epilogue below is a hook on it) and pol_softmax,
//     so x_l, the value and the probabilities have wab_policy_act's bits;
//   * head, fp32, per row: p = the forward's probabilities, log p_k = (logit_k - max) - logf(sum),
//     H = -sum_k p_k log p_k, g_logit_k = weight (p_k - [k = a]) + entropy_coef p_k (log p_k + H),
//     g_v = value_coef l'(v - target), l smooth_l1 (beta 1) or 0.5 d^2;
//   * backward, straight-through: D_l = bf16(G_l); dW_l = D_l^T x_{l-1} and db_l = D_l^T 1 by
//     v_mfma_f32_32x32x16_bf16 with the rows as the k dimension (16 rows per instruction, row
//     blocks of 128 in ascending order per slab); dx_{l-1} = D_l bf16(W_l) by the same instruction
//     from a transposed image of the packed weights; G_{l-1} = dx_{l-1} * (z >= 0 ? 1 : 0.01f),
//     and 0 where layer 3's leaky_relu left [-4, 4];
//   * sums over rows: row block b belongs to slab b % slabs, whatever the chunking; the reducer
//     adds the slabs in ascending order in fp32 and multiplies by `scale` once.  The loss terms
//     are summed in double (lanes by a fixed shuffle tree, waves, blocks and slabs in order).
// No float atomics; every sum has one order, so results are bitwise reproducible.
// wab_policy_grad_ppo (reference_ppo_loss_and_grad; include/wab.h) is the same with the head's
// weight replaced by the clipped surrogate's r A or 0, g_v by 0 where the value loss is clipped,
// and four more sums; wab_policy_evaluate is the forward and the head's row outputs alone.  Both
// are instances of wab_policy_bwd_kernel (MODE), so logp, value and entropy have the same bits.
//
// wab_policy_bwd_kernel: one workgroup per 128 rows, wab_policy_kernel's plan (the rows' features
// staged as bf16 chunks, the waves splitting the 32-unit tiles).  A lane keeps the leaky_relu and
// clamp masks of the units it produced as bits in registers: the backward pass's accumulators
// have the forward's layout (units the MFMA's rows, envs its columns), so the same lane applies
// them.  x_1..x_3 and D_1..D_4 go to the chunk's workspace unit-major (wab_policy_grad.h).
// wab_policy_wgrad_kernel: one wave per (up to 4 output tiles x one 32-column tile, slab).
// wab_policy_grad_reduce_kernel: slabs -> the ten torch-layout tensors and the four loss scalars.
#include <hip/hip_runtime.h>

#include "wab_policy_dev.h"
#include "wab_policy_grad.h"

namespace wab {

// ------------------------------------------------------------------------ transposed image
__device__ __forceinline__ uint16_t grad_wt_elem(const GradPackParams& p, int img, uint32_t i) {
  const PolicyDims& d = p.g.d;
  const uint32_t j = i & 7u, lane = (i >> 3) & 63u, f = i >> 9;
  const int KT = img == 1 ? p.g.KT1 : (img == 2 ? p.g.KT2 : p.g.KT3);
  const int nt = (int)(f / (uint32_t)KT), ks = (int)(f % (uint32_t)KT);
  const int n = 32 * nt + (int)(lane & 31u);                      // unit of layer img
  const int k = 16 * ks + 8 * (int)(lane >> 5) + (int)j;          // unit of layer img + 1
  // element (k, n) of the forward image of layer img + 1: tile k / 32, k-step n / 16
  const int KSf = img == 1 ? d.KS2 : (img == 2 ? d.KS3 : d.KS4);
  const int NTf = img == 1 ? d.NT2 : (img == 2 ? d.NT3 : 1);
  const uint32_t base = img == 1 ? d.w2 : (img == 2 ? d.w3 : d.wh);
  if (n >= 16 * KSf || k >= 32 * NTf) return 0;
  const uint32_t lanef = (uint32_t)(k & 31) + 32u * (uint32_t)((n & 15) >> 3);
  return p.w[base + (((uint32_t)(k >> 5) * (uint32_t)KSf + (uint32_t)(n >> 4)) * 64u + lanef) * 8u + (uint32_t)(n & 7)];
}

__global__ __launch_bounds__(256) void wab_policy_grad_pack(GradPackParams p) {
  const GradPlan& g = p.g;
  const uint32_t stride = gridDim.x * 256u;
  if (blockIdx.x == 0 && threadIdx.x < 2u) p.bad[threadIdx.x] = 0u;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < g.wt_total; i += stride) {
    if (i < g.wt2) p.wt[i] = grad_wt_elem(p, 1, i - g.wt1);
    else if (i < g.wt3) p.wt[i] = grad_wt_elem(p, 2, i - g.wt2);
    else p.wt[i] = grad_wt_elem(p, 3, i - g.wt3);
  }
}

// ------------------------------------------------------------------------ epilogues
// pol_store with the workspace column and the masks as its hook: bit (g & 1) * 16 + 4 mt + i of
// sb[g >> 1] is z >= 0, of cb the same for -4 <= leaky_relu(z) <= 4.  Rows past n_env go to the
// workspace as zeros.
template <bool CLAMP>
__device__ __forceinline__ void grad_fwd_store(const pol_f32x16 (&acc)[4], const float* __restrict__ bias, int tile,
                                               uint16_t* xn, int pitch, int lane, int n_env, uint16_t* wsx,
                                               int64_t cr, uint32_t (&sb)[2], uint32_t (&cb)[2]) {
  sb[0] = sb[1] = 0u;
  cb[0] = cb[1] = 0u;
  pol_store<CLAMP>(acc, bias, tile, xn, pitch, lane,
                   [&](int g, int mt, int i, int unit, int row, bool pos, bool inside, uint32_t bits) {
                     const uint32_t bit = 1u << ((g & 1) * 16 + 4 * mt + i);
                     if (pos) sb[g >> 1] |= bit;
                     if (CLAMP && inside) cb[g >> 1] |= bit;
                     wsx[(size_t)unit * (size_t)cr + (size_t)row] = (uint16_t)(row < n_env ? bits : 0u);
                   });
}

// D = bf16(dx * slope * clamp mask) of the tile's units into the LDS image the next backward
// layer reads (TO_LDS) and the workspace
template <bool CLAMP, bool TO_LDS>
__device__ __forceinline__ void grad_bwd_store(const pol_f32x16 (&acc)[4], int tile, uint16_t* dn, int pitch, int lane,
                                               uint16_t* wsd, int64_t cr, const uint32_t (&sb)[2],
                                               const uint32_t (&cb)[2]) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int n = 32 * tile + 8 * g + 4 * h;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      uint32_t o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t bit = 1u << ((g & 1) * 16 + 4 * mt + i);
        float v = acc[mt][4 * g + i];
        v = (sb[g >> 1] & bit) ? v : 0.01f * v;
        if (CLAMP) v = (cb[g >> 1] & bit) ? v : 0.0f;
        o[i] = pol_bf16(v);
        wsd[(size_t)(n + i) * (size_t)cr + (size_t)(mt * 32 + r)] = (uint16_t)o[i];
      }
      if (TO_LDS) {
        uint2 w;
        w.x = o[0] | (o[1] << 16);
        w.y = o[2] | (o[3] << 16);
        *reinterpret_cast<uint2*>(dn + (size_t)(mt * 32 + r) * (size_t)pitch + (size_t)n) = w;
      }
    }
  }
}

__device__ __forceinline__ double grad_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// the configured value loss of one difference and its derivative
__device__ __forceinline__ float grad_value_loss(float dl, bool mse, float& dv) {
  const float ad = fabsf(dl);
  const bool quad = mse || ad < 1.0f;
  dv = quad ? dl : (dl > 0.0f ? 1.0f : -1.0f);
  return quad ? 0.5f * dl * dl : ad - 0.5f;
}

// ------------------------------------------------------------------------ rows through an index
// The source row of an index (wab_policy_*_gather): clamped into [0, M) before anything is loaded
// through it.  A row whose index was outside is left out as a bad-action row is, and counted in
// bad[1] by the head.
__device__ __forceinline__ int64_t grad_src_row(int32_t idx, int64_t M) {
  const int64_t i = idx;
  return i < 0 ? 0 : (i < M ? i : M - 1);
}

// lane j's 64-bit value, the same in every lane (j wave-uniform)
__device__ __forceinline__ size_t grad_lane_u64(size_t v, int j) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
  return (size_t)lo | ((size_t)hi << 32);
}

// ------------------------------------------------------------------------ forward, head, backward chain
// MODE (wab_policy_grad.h): kGradModePpo changes the head's weight, value gradient and sums alone;
// kGradModeEval ends after the head's row outputs and touches no workspace but the bad counts.
// GATHER: row i of the call is row rows[i] of the source (features and the head's per-row inputs);
// the blocks, the workspace, the sums and the row outputs are those of rows 0 .. N - 1 all the
// same, so the results are the bits of the plain instance on gathered copies.
// Columns [k0, k0 + kn) of the block's 128 rows as bf16 0x0000 / 0x3F80 into x[128][pitch] from
// packed rows (include/wab.h, WAB_HAS_PACKED_FEATURES; PACKED instances).  k0 is a multiple of 16
// and kn at most 256, 240 where k0 is in the middle of a dword, so the chunk lies within the eight
// dwords from k0 >> 5: thread t takes four of them (half t & 1) of row t >> 1, one 16-byte load
// where they start on a 16-byte boundary of the row, and expands each byte inside the chunk to one
// 16-byte LDS store.  `row` is the thread's source row (null: past the batch, stored as zeros);
// columns from F on are zero whatever the row's pad bits hold.
__device__ __forceinline__ void grad_stage_packed(const uint32_t* __restrict__ row, int F, int P, int k0, int kn,
                                                  uint16_t* x, int pitch, int tid) {
  const int e = tid >> 1;
  const int dw = (k0 >> 5) + 4 * (tid & 1);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (row) {
    if ((dw & 3) == 0 && dw + 4 <= P) {
      const uint4 v = *reinterpret_cast<const uint4*>(row + dw);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (dw + i < P) w[i] = row[dw + i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int k = 32 * (dw + i) + 8 * b;
      if (k < k0 || k >= k0 + kn) continue;
      uint32_t bits = (w[i] >> (8 * b)) & 0xFFu;
      bits = k >= F ? 0u : (F - k >= 8 ? bits : bits & ((1u << (F - k)) - 1u));
      uint4 v;  // bf16 1.0 = 0x3F80
      v.x = ((bits & 1u) ? 0x3F80u : 0u) | ((bits & 2u) ? 0x3F800000u : 0u);
      v.y = ((bits & 4u) ? 0x3F80u : 0u) | ((bits & 8u) ? 0x3F800000u : 0u);
      v.z = ((bits & 16u) ? 0x3F80u : 0u) | ((bits & 32u) ? 0x3F800000u : 0u);
      v.w = ((bits & 64u) ? 0x3F80u : 0u) | ((bits & 128u) ? 0x3F800000u : 0u);
      *reinterpret_cast<uint4*>(x + (size_t)e * (size_t)pitch + (size_t)(k - k0)) = v;
    }
  }
}

template <bool TWO, int MODE, bool GATHER, bool PACKED>
__global__ __launch_bounds__(256, TWO ? 1 : 2) void wab_policy_bwd_kernel(GradBwdParams p) {
  constexpr bool PPO = MODE == kGradModePpo, EVAL = MODE == kGradModeEval;
  constexpr int TERMS = PPO ? kGradPpoTerms : kGradLossTerms;
  extern __shared__ __attribute__((aligned(16))) unsigned char grad_smem[];
  uint16_t* const regA = reinterpret_cast<uint16_t*>(grad_smem);
  uint16_t* const regB = reinterpret_cast<uint16_t*>(grad_smem + p.g.lds.off_b);
  uint16_t* const regC = regA;  // D_4, once X_2 has been read
  const GradPlan& g = p.g;
  const PolicyDims& d = g.d;
  const PolicyLds& L = g.lds;
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int64_t env0 = p.row0 + (int64_t)blockIdx.x * kGradRows;  // (global row; < N by the grid)
  const int n_env = (int)(p.N - env0 < kGradRows ? p.N - env0 : kGradRows);
  const int64_t cr = p.chunk_rows;
  uint16_t* const ws = p.ws + (size_t)blockIdx.x * kGradRows;  // this block's rows of every unit
  const uint4* const wimg = reinterpret_cast<const uint4*>(p.w);
  const uint4* const wtimg = reinterpret_cast<const uint4*>(p.wt);

  uint32_t s1[2][2] = {}, s2[2][2] = {}, s3[2][2] = {}, c3[2][2] = {}, cx[2] = {};

  // GATHER: lane (j, .) of wave w keeps where tile row w + 4 j (the rows the wave stages; past the
  // batch, the batch's last) starts in the source, one index load per row and launch; the staging
  // reads it lane to scalar, once per 16 loads
  [[maybe_unused]] size_t src_off = 0;
  if constexpr (GATHER && !PACKED) {
    const int e = wave + 4 * r;
    src_off = (size_t)grad_src_row(p.rows[env0 + (e < n_env ? e : n_env - 1)], p.M) * (size_t)d.F;
  }
  // PACKED: thread t stages row t >> 1 of the block (grad_stage_packed): its packed source row, one
  // index load per thread and launch
  [[maybe_unused]] const uint32_t* bits_row = nullptr;
  if constexpr (PACKED) {
    const int e = (int)(threadIdx.x >> 1);
    if (e < n_env) {
      int64_t src = env0 + e;
      if constexpr (GATHER) src = grad_src_row(p.rows[src], p.M);
      bits_row = p.bits + (size_t)src * (size_t)p.P;
    }
  }

  // ---- layer 1: chunks of KC input columns through region A -> X1 (region B)
  pol_layer1<4, TWO>(
      d, L, wimg, regA, wave, lane,
      [&](int k0, int kn) {
        if constexpr (PACKED)
          grad_stage_packed(bits_row, d.F, p.P, k0, kn, regA, L.pitch_in, (int)threadIdx.x);
        else if constexpr (GATHER)
          pol_stage_rows<kGradRows>(p.features, d.F, n_env, k0, kn, regA, L.pitch_in, wave, lane,
                                    [&](int j, int) { return grad_lane_u64(src_off, j); },
                                    [](int, int, float, bool) {});
        else
          pol_stage_rows<kGradRows>(p.features + (size_t)env0 * (size_t)d.F, d.F, n_env, k0, kn, regA, L.pitch_in,
                                    wave, lane, [](int, int, float, bool) {});
      },
      [] { __syncthreads(); },
      [&](const pol_f32x16(&acc)[4], int t, int j) {
        if constexpr (EVAL)
          pol_store<false>(acc, p.b + d.b1, t, regB, L.pitch1, lane);
        else
          grad_fwd_store<false>(acc, p.b + d.b1, t, regB, L.pitch1, lane, n_env, ws + (size_t)g.u_x[1] * (size_t)cr, cr,
                                s1[j], cx);
      });
  __syncthreads();  // X1 complete; region A free

  // ---- layer 2: X1 (region B) -> X2 (region A); layer 3: X2 -> X3 (region B), clamped
  uint4 wf[kPolicyMaxKs];
  pol_layer<4, false>(wf, wimg + (d.w2 >> 3), d.NT2, d.KS2, regB, L.pitch1, wave, lane,
                      [&](const pol_f32x16(&acc)[4], int t, int j) {
                        if constexpr (EVAL)
                          pol_store<false>(acc, p.b + d.b2, t, regA, L.pitch2, lane);
                        else
                          grad_fwd_store<false>(acc, p.b + d.b2, t, regA, L.pitch2, lane, n_env,
                                                ws + (size_t)g.u_x[2] * (size_t)cr, cr, s2[j], cx);
                      });
  __syncthreads();
  pol_layer<4, false>(wf, wimg + (d.w3 >> 3), d.NT3, d.KS3, regA, L.pitch2, wave, lane,
                      [&](const pol_f32x16(&acc)[4], int t, int j) {
                        if constexpr (EVAL)
                          pol_store<true>(acc, p.b + d.b3, t, regB, L.pitch3, lane);
                        else
                          grad_fwd_store<true>(acc, p.b + d.b3, t, regB, L.pitch3, lane, n_env,
                                               ws + (size_t)g.u_x[3] * (size_t)cr, cr, s3[j], c3[j]);
                      });
  pol_load_frags(wf, wimg + (d.wh >> 3) + (size_t)lane, d.KS4);
  __syncthreads();

  // ---- heads: wave w on rows 32 w .., lanes 0..31 finish
  {
    const pol_f32x16 acc = pol_head_mma(wf, d.KS4, regB + (size_t)(32 * wave + r) * (size_t)L.pitch3 + 8 * h);
    const int A = d.A;
    const PolSoftmax q = pol_softmax(acc, lane, p.b + d.bh, A);
    const int my = 32 * wave + r;
    const int64_t row = env0 + my;
    const bool live = h == 0 && my < n_env;
    double part[TERMS] = {};
    if (h == 0) {
      const float val = q.val;
      float z[kPolicyMaxActions], pk[kPolicyMaxActions], gk[kPolicyMaxActions];
      const float ls = logf(q.s);
      float H = 0.0f;
#pragma unroll
      for (int k = 0; k < kPolicyMaxActions; ++k) {
        pk[k] = q.e[k] * q.inv;
        z[k] = q.z[k] - ls;  // log p_k
        if (k < A) H = H - pk[k] * z[k];
      }
      int a = 0;
      float wgt = 0.0f, tgt = 0.0f, olp = 0.0f, ov = 0.0f;
      // the row the head's inputs are read at: the call's row, or (GATHER) its source row
      int64_t in = row;
      [[maybe_unused]] bool bad_row = false;
      if constexpr (GATHER) {
        if (live) {
          const int32_t idx = p.rows[row];
          bad_row = idx < 0 || (int64_t)idx >= p.M;
          in = grad_src_row(idx, p.M);
        }
      }
      if (live) {
        if (!EVAL || p.actions) a = (int)p.actions[in];
        if (!EVAL) {
          wgt = p.weight[in];
          tgt = p.target[in];
        }
        if (PPO) {
          olp = p.old_logp[in];
          if (p.value_clip > 0.0f) ov = p.old_value[in];
        }
      }
      if constexpr (GATHER) a = bad_row ? -1 : a;  // (from here on a bad-action row)
      const bool bad = a < 0 || a >= A;
      const bool use = live && !bad;
      if constexpr (GATHER) {
        if (live && bad) atomicAdd(bad_row ? p.bad + 1 : p.bad, 1u);
      } else {
        if (live && bad) atomicAdd(p.bad, 1u);
      }
      float la = 0.0f;
      if constexpr (EVAL) {
        // (a chain of selects on `a` alone is turned into an indexed load from a scratch copy of z)
        uint32_t za = 0u;
#pragma unroll
        for (int k = 0; k < kPolicyMaxActions; ++k) za |= k == a ? __builtin_bit_cast(uint32_t, z[k]) : 0u;
        la = __builtin_bit_cast(float, za);
        if (live) {
          if (p.logp) p.logp[row] = bad ? 0.0f : la;
          if (p.value) p.value[row] = val;
          if (p.entropy) p.entropy[row] = H;
        }
      } else {
        // the clipped surrogate (include/wab.h): r = exp(clamp(logp - old_logp)), the weight r A or,
        // where the clip holds the row, 0
        float weff = wgt, lpol = 0.0f, rr = 0.0f, dlt = 0.0f;
        bool clipped = false;
        if constexpr (PPO) {
#pragma unroll
          for (int k = 0; k < kPolicyMaxActions; ++k)
            if (k == a) la = z[k];
          dlt = la - olp;
          dlt = dlt < -30.0f ? -30.0f : (dlt > 30.0f ? 30.0f : dlt);
          rr = expf(dlt);
          const float lo = 1.0f - p.clip, hi = 1.0f + p.clip;
          clipped = (wgt > 0.0f && rr > hi) || (wgt < 0.0f && rr < lo);
          const float ra = rr * wgt;
          weff = clipped ? 0.0f : ra;
          lpol = clipped ? -(wgt * (wgt > 0.0f ? hi : lo)) : -ra;
        }
#pragma unroll
        for (int k = 0; k < kPolicyMaxActions; ++k) {
          if (k == a) la = z[k];
          const float g1 = weff * (pk[k] - (k == a ? 1.0f : 0.0f));
          const float g2 = p.entropy_coef * (pk[k] * (z[k] + H));
          gk[k] = (use && k < A) ? g1 + g2 : 0.0f;
        }
        float dv;
        float lv = grad_value_loss(val - tgt, p.mse != 0, dv);
        bool vclipped = false;
        if constexpr (PPO) {
          const float u = val - ov, c = p.value_clip;
          if (c > 0.0f && !(fabsf(u) <= c)) {
            float dv2;
            const float l2 = grad_value_loss((ov + (u > 0.0f ? c : -c)) - tgt, p.mse != 0, dv2);
            vclipped = l2 > lv;
            lv = vclipped ? l2 : lv;
          }
        }
        const float gv = (use && !vclipped) ? p.value_coef * dv : 0.0f;
        if (use) {
          part[0] = PPO ? (double)lpol : (double)(-(wgt * la));
          part[1] = (double)lv;
          part[2] = (double)H;
          if constexpr (PPO) {
            part[3] = clipped ? 1.0 : 0.0;
            part[4] = expm1((double)dlt) - (double)dlt;  // Schulman's k3, from the fp32 d
            part[5] = vclipped ? 1.0 : 0.0;
            part[6] = (double)rr;
          }
        }
        if (live) {
          if (p.logp) p.logp[row] = bad ? 0.0f : la;
          if (p.value) p.value[row] = val;
          if (p.entropy) p.entropy[row] = H;
          if (PPO && p.ratio) p.ratio[row] = bad ? 0.0f : rr;
        }
        // D_4's row: [g_logit (8) | g_v | 0 x 7] as bf16, to region C and the workspace
        uint32_t o[kGradHeadUnits];
#pragma unroll
        for (int k = 0; k < kGradHeadUnits; ++k)
          o[k] = k < kPolicyMaxActions ? pol_bf16(gk[k < kPolicyMaxActions ? k : 0])
                                       : (k == kPolicyMaxActions ? pol_bf16(gv) : 0u);
        uint4 q0, q1;
        q0.x = o[0] | (o[1] << 16); q0.y = o[2] | (o[3] << 16); q0.z = o[4] | (o[5] << 16); q0.w = o[6] | (o[7] << 16);
        q1.x = o[8] | (o[9] << 16); q1.y = o[10] | (o[11] << 16); q1.z = o[12] | (o[13] << 16); q1.w = o[14] | (o[15] << 16);
        uint4* const drow = reinterpret_cast<uint4*>(regC + (size_t)my * (size_t)g.pitch4);
        drow[0] = q0;
        drow[1] = q1;
        uint16_t* const wsd = ws + (size_t)g.u_d[4] * (size_t)cr + (size_t)my;
#pragma unroll
        for (int k = 0; k < kGradHeadUnits; ++k) wsd[(size_t)k * (size_t)cr] = (uint16_t)o[k];
      }
    }
    if constexpr (!EVAL) {
#pragma unroll
      for (int j = 0; j < TERMS; ++j) {
        const double v = grad_wave_sum(part[j]);
        if (lane == 0) p.part[((size_t)blockIdx.x * 4u + (size_t)wave) * (size_t)kGradTermPitch + (size_t)j] = v;
      }
    }
  }
  if constexpr (EVAL) return;  // forward and head alone
  __syncthreads();  // D_4 complete

  // ---- dx_3 = D_4 . [Wa; Wv] -> D_3 (region B); dx_2 = D_3 . W_3 -> D_2 (region A); dx_1 -> D_1
  pol_layer<4, false>(wf, wtimg + (g.wt3 >> 3), d.NT3, g.KT3, regC, g.pitch4, wave, lane,
                      [&](const pol_f32x16(&acc)[4], int t, int j) {
                        grad_bwd_store<true, true>(acc, t, regB, L.pitch3, lane, ws + (size_t)g.u_d[3] * (size_t)cr, cr,
                                                   s3[j], c3[j]);
                      });
  __syncthreads();
  pol_layer<4, false>(wf, wtimg + (g.wt2 >> 3), d.NT2, g.KT2, regB, L.pitch3, wave, lane,
                      [&](const pol_f32x16(&acc)[4], int t, int j) {
                        grad_bwd_store<false, true>(acc, t, regA, L.pitch2, lane, ws + (size_t)g.u_d[2] * (size_t)cr, cr,
                                                    s2[j], cx);
                      });
  __syncthreads();
  pol_layer<4, false>(wf, wtimg + (g.wt1 >> 3), d.NT1, g.KT1, regA, L.pitch2, wave, lane,
                      [&](const pol_f32x16(&acc)[4], int t, int j) {
                        grad_bwd_store<false, false>(acc, t, nullptr, 0, lane, ws + (size_t)g.u_d[1] * (size_t)cr, cr,
                                                     s1[j], cx);
                      });
}

template __global__ void wab_policy_bwd_kernel<false, kGradModeGrad, false>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModeGrad, false>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<false, kGradModePpo, false>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModePpo, false>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<false, kGradModeEval, false>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModeEval, false>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<false, kGradModeGrad, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModeGrad, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<false, kGradModePpo, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModePpo, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<false, kGradModeEval, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModeEval, true>(GradBwdParams p);
// (PACKED: the rows' features are packed bits, wab_policy_*_packed)
template __global__ void wab_policy_bwd_kernel<false, kGradModeGrad, false, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModeGrad, false, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<false, kGradModePpo, false, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModePpo, false, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<false, kGradModeEval, false, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModeEval, false, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<false, kGradModeGrad, true, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModeGrad, true, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<false, kGradModePpo, true, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModePpo, true, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<false, kGradModeEval, true, true>(GradBwdParams p);
template __global__ void wab_policy_bwd_kernel<true, kGradModeEval, true, true>(GradBwdParams p);

// ------------------------------------------------------------------------ dW, db
// the slab's row blocks of this chunk, ascending: acc[i] += D_l[rows, tile i]^T . [X_{l-1} | 1][rows, tile kt]
// (GATHER, on the FEAT path alone: a lane's eight feature rows are the source rows of its eight rows)
// (PACKED, on the FEAT path alone: lane r of tile kt takes bit r of dword kt of each of its eight
// packed rows, one dword load per row at the same address in the 32 lanes, and builds the operand
// words the float loads round to: 0x3F80 where the bit is set)
template <bool FEAT, bool GATHER, bool PACKED = false>
__device__ __forceinline__ void grad_wgrad_blocks(const GradWgradParams& p, int K, int n_d, int u_d, int u_x, int grp,
                                                  int kt, int tiles, int slab, int lane,
                                                  pol_f32x16 (&acc)[kGradTiles]) {
  const GradPlan& g = p.g;
  const int r = lane & 31, h = lane >> 5;
  const size_t cr = (size_t)p.chunk_rows;
  const int64_t S = g.slabs;
  const int64_t B0 = p.row0 / kGradRows;
  const int c = 32 * kt + r;
  const bool c_in = c < K, c_one = c == K;
  const uint16_t* const xcol = p.ws + (size_t)(u_x + (c_in && !FEAT ? c : 0)) * cr;
  const float* const fcol = p.features + (size_t)(c_in ? c : 0);
  const uint16_t* dcol[kGradTiles];
  bool a_ok[kGradTiles];
#pragma unroll
  for (int i = 0; i < kGradTiles; ++i) {
    const int m = 32 * (kGradTiles * grp + i) + r;
    a_ok[i] = m < n_d;
    dcol[i] = p.ws + (size_t)(u_d + (a_ok[i] ? m : 0)) * cr;
  }
  // operands outside the arrays as masks (a select between whole vectors goes through scratch):
  // a column past K_in is 0, column K_in the bf16 ones; an output unit past the array is 0
  const uint32_t b_and = c_in ? 0xFFFFFFFFu : 0u, b_or = c_one ? 0x3F803F80u : 0u;
  uint32_t a_and[kGradTiles];
#pragma unroll
  for (int i = 0; i < kGradTiles; ++i) a_and[i] = a_ok[i] ? 0xFFFFFFFFu : 0u;
  for (int64_t b = B0 + ((int64_t)slab - B0 % S + S) % S; b < B0 + p.n_blocks; b += S) {
    const size_t rb = (size_t)(b - B0) * kGradRows;
    // GATHER: the block's 128 source rows, one index load per row and block: lane l holds those of
    // rows l and 64 + l (a row past N clamped to N - 1 first, then its index into the source); a
    // k-step's eight come from there lane to lane, so no feature load waits for an index load
    [[maybe_unused]] int32_t src_lo = 0, src_hi = 0;
    if constexpr (FEAT && GATHER) {
      const int64_t r0 = p.row0 + (int64_t)rb + lane, r1 = r0 + 64;
      src_lo = (int32_t)grad_src_row(p.rows[r0 < p.N ? r0 : p.N - 1], p.M);
      src_hi = (int32_t)grad_src_row(p.rows[r1 < p.N ? r1 : p.N - 1], p.M);
    }
#pragma unroll 4
    for (int ks = 0; ks < kGradRows / 16; ++ks) {
      const size_t rc = rb + (size_t)(16 * ks + 8 * h);
      uint4 bv;
      if constexpr (FEAT && PACKED) {
        // (a tile past the row's dwords, the ones column's at F a multiple of 128, is masked below)
        const uint32_t* const bcol = p.bits + (size_t)(kt < p.P ? kt : p.P - 1);
        uint32_t o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int64_t row = p.row0 + (int64_t)rc + j;
          row = row < p.N ? row : p.N - 1;  // (rows past N have D = 0)
          if constexpr (GATHER) row = __shfl(ks < 4 ? src_lo : src_hi, (16 * ks + 8 * h + j) & 63, 64);
          o[j] = ((bcol[(size_t)row * (size_t)p.P] >> r) & 1u) ? 0x3F80u : 0u;
        }
        bv.x = o[0] | (o[1] << 16);
        bv.y = o[2] | (o[3] << 16);
        bv.z = o[4] | (o[5] << 16);
        bv.w = o[6] | (o[7] << 16);
      } else if (FEAT) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int64_t row = p.row0 + (int64_t)rc + j;
          row = row < p.N ? row : p.N - 1;  // (rows past N have D = 0)
          if constexpr (GATHER) row = __shfl(ks < 4 ? src_lo : src_hi, (16 * ks + 8 * h + j) & 63, 64);
          v[j] = fcol[(size_t)row * (size_t)K];
        }
        bv.x = pol_bf16(v[0]) | (pol_bf16(v[1]) << 16);
        bv.y = pol_bf16(v[2]) | (pol_bf16(v[3]) << 16);
        bv.z = pol_bf16(v[4]) | (pol_bf16(v[5]) << 16);
        bv.w = pol_bf16(v[6]) | (pol_bf16(v[7]) << 16);
      } else {
        bv = *reinterpret_cast<const uint4*>(xcol + rc);
      }
      bv.x = (bv.x & b_and) | b_or; bv.y = (bv.y & b_and) | b_or;
      bv.z = (bv.z & b_and) | b_or; bv.w = (bv.w & b_and) | b_or;
#pragma unroll
      for (int i = 0; i < kGradTiles; ++i) {
        if (i < tiles) {  // (uniform)
          uint4 av = *reinterpret_cast<const uint4*>(dcol[i] + rc);
          av.x &= a_and[i]; av.y &= a_and[i]; av.z &= a_and[i]; av.w &= a_and[i];
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pol_frag(av), pol_frag(bv), acc[i], 0, 0, 0);
        }
      }
    }
  }
}

template <bool GATHER, bool PACKED>
__global__ __launch_bounds__(64) void wab_policy_wgrad_kernel(GradWgradParams p) {
  const GradPlan& g = p.g;
  const int lane = (int)threadIdx.x, task = (int)blockIdx.x, slab = (int)blockIdx.y;
  const int64_t S = g.slabs;
  const int64_t B0 = p.row0 / kGradRows;
  if (task == g.n_tasks) {
    // the loss terms of the slab's row blocks, ascending, waves in order
    if (lane < p.n_terms) {
      double* const dst = p.loss + (size_t)slab * (size_t)kGradTermPitch + (size_t)lane;
      double v = p.first ? 0.0 : *dst;
      for (int64_t b = B0 + ((int64_t)slab - B0 % S + S) % S; b < B0 + p.n_blocks; b += S)
        for (int w = 0; w < 4; ++w) v = v + p.part[((size_t)(b - B0) * 4u + (size_t)w) * (size_t)kGradTermPitch + (size_t)lane];
      *dst = v;
    }
    return;
  }
  // the task's layer and its constants (static indices: the plan stays in scalar registers)
  int layer = 1, t0 = 0, K = g.k_in[1], n_d = g.n_d[1], u_d = g.u_d[1], u_x = 0, kts = g.ktiles[1];
#pragma unroll
  for (int l = 2; l <= 4; ++l)
    if (task >= g.task0[l]) {
      layer = l; t0 = g.task0[l]; K = g.k_in[l]; n_d = g.n_d[l]; u_d = g.u_d[l]; u_x = g.u_x[l - 1]; kts = g.ktiles[l];
    }
  const int local = task - t0;
  const int grp = local / kts, kt = local % kts;
  const int all = layer < 4 ? n_d / 32 : 1;
  const int tiles = all - kGradTiles * grp < kGradTiles ? all - kGradTiles * grp : kGradTiles;
  float* const sl = p.slab + ((size_t)slab * (size_t)g.n_tasks + (size_t)task) * (size_t)(kGradTiles * 1024) + (size_t)lane;
  pol_f32x16 acc[kGradTiles];
  pol_zero(acc);
  if (!p.first) {
#pragma unroll
    for (int i = 0; i < kGradTiles; ++i)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][q] = sl[(size_t)((i * 16 + q) * 64)];
  }
  if (layer == 1) grad_wgrad_blocks<true, GATHER, PACKED>(p, K, n_d, u_d, u_x, grp, kt, tiles, slab, lane, acc);
  else grad_wgrad_blocks<false, false>(p, K, n_d, u_d, u_x, grp, kt, tiles, slab, lane, acc);
#pragma unroll
  for (int i = 0; i < kGradTiles; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) sl[(size_t)((i * 16 + q) * 64)] = acc[i][q];
}

template __global__ void wab_policy_wgrad_kernel<false>(GradWgradParams p);
template __global__ void wab_policy_wgrad_kernel<true>(GradWgradParams p);
template __global__ void wab_policy_wgrad_kernel<false, true>(GradWgradParams p);
template __global__ void wab_policy_wgrad_kernel<true, true>(GradWgradParams p);

// ------------------------------------------------------------------------ slabs -> gradients
__global__ __launch_bounds__(256) void wab_policy_grad_reduce_kernel(GradReduceParams p) {
  const GradPlan& g = p.g;
  const PolicyDims& d = g.d;
  const int64_t n1 = (int64_t)d.h1 * (d.F + 1), n2 = (int64_t)d.h2 * (d.h1 + 1), n3 = (int64_t)d.h3 * (d.h2 + 1);
  const int64_t n4 = (int64_t)(d.A + 1) * (d.h3 + 1);
  const int64_t total = n1 + n2 + n3 + n4;
  const size_t slab_stride = (size_t)g.n_tasks * (size_t)(kGradTiles * 1024);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    int layer;
    int64_t o = e;
    if (o < n1) layer = 1;
    else if ((o -= n1) < n2) layer = 2;
    else if ((o -= n2) < n3) layer = 3;
    else { o -= n3; layer = 4; }
    const int K = layer == 1 ? d.F : (layer == 2 ? d.h1 : (layer == 3 ? d.h2 : d.h3));
    const int t0 = layer == 1 ? g.task0[1] : (layer == 2 ? g.task0[2] : (layer == 3 ? g.task0[3] : g.task0[4]));
    const int kts = layer == 1 ? g.ktiles[1] : (layer == 2 ? g.ktiles[2] : (layer == 3 ? g.ktiles[3] : g.ktiles[4]));
    const int n = (int)(o / (K + 1)), k = (int)(o % (K + 1));
    // the MFMA row of the unit: the value head is row 8 of the head tile
    const int nm = (layer == 4 && n == d.A) ? kPolicyMaxActions : n;
    const int tile = nm >> 5, m = nm & 31;
    const int task = t0 + (tile / kGradTiles) * kts + (k >> 5);
    const int q = 4 * (m >> 3) + (m & 3), ln = (k & 31) + 32 * ((m >> 2) & 1);
    const size_t idx = ((size_t)task * kGradTiles + (size_t)(tile % kGradTiles)) * 1024u + (size_t)(q * 64 + ln);
    float v = 0.0f;
    if (!p.empty)
      for (int s = 0; s < g.slabs; ++s) v = v + p.slab[(size_t)s * slab_stride + idx];
    v = v * p.scale;
    float* dst;
    if (layer == 1) dst = k < K ? p.out.w1 + (size_t)n * (size_t)K + k : p.out.b1 + n;
    else if (layer == 2) dst = k < K ? p.out.w2 + (size_t)n * (size_t)K + k : p.out.b2 + n;
    else if (layer == 3) dst = k < K ? p.out.w3 + (size_t)n * (size_t)K + k : p.out.b3 + n;
    else if (n < d.A) dst = k < K ? p.out.wa + (size_t)n * (size_t)K + k : p.out.ba + n;
    else dst = k < K ? p.out.wv + k : p.out.bv;
    *dst = p.accumulate ? *dst + v : v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && p.loss_out) {
    double l[3] = {0.0, 0.0, 0.0};
    if (!p.empty)
      for (int s = 0; s < g.slabs; ++s)
        for (int j = 0; j < 3; ++j) l[j] = l[j] + p.loss[(size_t)s * (size_t)kGradTermPitch + (size_t)j];
    const double tot = (double)p.scale * (l[0] + (double)p.value_coef * l[1] - (double)p.entropy_coef * l[2]);
    const float out[4] = {(float)l[0], (float)l[1], (float)l[2], (float)tot};
    for (int j = 0; j < 4; ++j) p.loss_out[j] = p.accumulate ? p.loss_out[j] + out[j] : out[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && p.ppo_out) {
    // the clipped surrogate's diagnostics, never scaled
    for (int j = 0; j < kGradPpoTerms - kGradLossTerms; ++j) {
      double v = 0.0;
      if (!p.empty)
        for (int s = 0; s < g.slabs; ++s) v = v + p.loss[(size_t)s * (size_t)kGradTermPitch + (size_t)(kGradLossTerms + j)];
      p.ppo_out[j] = p.accumulate ? p.ppo_out[j] + (float)v : (float)v;
    }
  }
}

}  // namespace wab
