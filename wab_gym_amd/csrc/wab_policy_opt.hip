// wab_policy_opt.hip — optimizer.step() of actor_critic.py:104, :165 for the device policy: Adam
// (or AdamW) with a global-norm clip and a skip on a non-finite gradient, writing the fp32
// parameter, both moments and the packed bf16 image wab_policy_act reads (wab_policy_adam_step).
// gfx950.
//
// Numeric contract (include/wab.h states it in full; reference_adam_step of
// wab_gym_amd/policy_reference.py is the same in numpy; the library is built with -ffp-contract=off):
//   * S = the adjacent-pair tree sum of (double)g_i * (double)g_i over the flat order, zero-padded
//     to a power of two; norm = sqrt(S); a non-finite S skips the step;
//   * c = (float)min(1, max_grad_norm / (norm + 1e-6)) or 1; bias corrections from the running
//     products beta^step kept in the state, in double; a = (float)(lr / (1 - b1p)),
//     r2 = sqrtf((float)(1 - b2p));
//   * per element in fp32: g = g c (+ wd p), m = b1 m + (1 - b1) g, v = b2 v + ((1 - b2) g) g,
//     p = p - a (m / (sqrtf(v) / r2 + eps)); the image element is pol_bf16(p).
//
// Shape: the work is latency-bound (the reference net moves about 3 MB), so it is three launches
// with nothing shared between workgroups inside a launch:
//   1. wab_adam_norm_kernel: a workgroup of 256 threads sums one 1024-element segment of the flat
//      order, a subtree of the pair tree (four elements per thread, an xor butterfly in the wave,
//      the four waves through LDS), into one double of the workspace.  More than 1024 segments
//      (in_features beyond ~4000) take wab_adam_mid_kernel, the same over the partials;
//   2. wab_adam_update_kernel, indexed by the packed image as wab_policy_pack is: every workgroup
//      first finishes the tree over the (at most 1024) partials itself and reads the state, then
//      one thread per image element does the Adam arithmetic and stores the parameter, the moments
//      and the bf16 element; padding is never written; the biases take a second loop;
//   3. wab_adam_finish_kernel, one workgroup: the same tree once more, then the new state.  The
//      update launch reads the state every workgroup of it needs unchanged, so the state is written
//      by the launch after it.
// No atomics; every sum has one order, which depends on the shape alone.
#include <hip/hip_runtime.h>

#include "wab_policy_dev.h"
#include "wab_policy_opt.h"

namespace wab {

namespace {

// ((a + b) + (c + d)) of thread t's four consecutive values, then the pair tree over the 256
// threads: the sum of a 1024-value subtree, in every thread.  lds: four doubles, used once.
__device__ __forceinline__ double adam_block_sum(double a, double b, double c, double d, double* lds) {
  double s = (a + b) + (c + d);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s = s + __shfl_xor(s, m);  // (x + y == y + x bit for bit: both lanes of a pair agree)
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__device__ __forceinline__ double adam_partial(const double* __restrict__ part, uint32_t n, uint32_t i) {
  return i < n ? part[i] : 0.0;
}

// the tree over the last level's partials (n <= 1024)
__device__ __forceinline__ double adam_total(const double* __restrict__ part, uint32_t n, double* lds) {
  const uint32_t i = 4u * threadIdx.x;
  return adam_block_sum(adam_partial(part, n, i), adam_partial(part, n, i + 1u), adam_partial(part, n, i + 2u),
                        adam_partial(part, n, i + 3u), lds);
}

// What one call derives from S, the constants and the state before it.
struct AdamScalars {
  double b1p, b2p;  // the new beta powers
  float norm, c, a, r2;
  bool skip;
};

__device__ __forceinline__ AdamScalars adam_scalars(double S, const AdamConsts& k, const AdamState& st) {
  AdamScalars r;
  const double norm = sqrt(S);
  r.norm = (float)norm;
  r.skip = !__builtin_isfinite(S);
  r.c = 1.0f;
  if (k.max_grad_norm > 0.0) {
    const double q = k.max_grad_norm / (norm + 1e-6);
    r.c = (float)(q < 1.0 ? q : 1.0);  // (a NaN norm gives 1)
  }
  r.b1p = (st.step == 0 ? 1.0 : st.beta1_pow) * k.beta1;
  r.b2p = (st.step == 0 ? 1.0 : st.beta2_pow) * k.beta2;
  r.a = (float)(k.lr / (1.0 - r.b1p));
  r.r2 = sqrtf((float)(1.0 - r.b2p));
  return r;
}

struct AdamStep {
  AdamConsts k;
  float c, a, r2;
};

// one element: reads g[e], updates p[e], m[e], v[e]; returns the new parameter
__device__ __forceinline__ float adam_element(const AdamStep& s, const float* __restrict__ g, float* __restrict__ p,
                                              float* __restrict__ m, float* __restrict__ v, size_t e) {
  float gi = g[e] * s.c;
  float pe = p[e];
  if (s.k.decay == 1) gi = gi + s.k.wdf * pe;
  if (s.k.decay == 2) pe = pe * s.k.decayf;
  const float me = s.k.b1f * m[e] + s.k.omb1 * gi;
  const float ve = s.k.b2f * v[e] + (s.k.omb2 * gi) * gi;
  const float den = sqrtf(ve) / s.r2 + s.k.epsf;
  pe = pe - s.a * (me / den);
  p[e] = pe;
  m[e] = me;
  v[e] = ve;
  return pe;
}

// element i of a hidden layer's image, ((nt * KS + ks) * 64 + lane) * 8 + j (pack_layer's index)
__device__ __forceinline__ void adam_layer(const AdamStep& s, const float* __restrict__ g, float* __restrict__ W,
                                           float* __restrict__ M, float* __restrict__ V, int N, int K, int KS,
                                           uint16_t* __restrict__ dst, uint32_t i) {
  const uint32_t j = i & 7u, lane = (i >> 3) & 63u, f = i >> 9;
  const int nt = (int)(f / (uint32_t)KS), ks = (int)(f % (uint32_t)KS);
  const int n = 32 * nt + (int)(lane & 31u), k = 16 * ks + 8 * (int)(lane >> 5) + (int)j;
  if (n < N && k < K) dst[i] = (uint16_t)pol_bf16(adam_element(s, g, W, M, V, (size_t)n * (size_t)K + (size_t)k));
}

}  // namespace

// ------------------------------------------------------------------------ the norm's partials
__global__ __launch_bounds__(256) void wab_adam_norm_kernel(AdamNormParams p) {
  __shared__ double lds[4];
  const uint32_t P = p.flat.off[kAdamTensors];
  const uint32_t i0 = blockIdx.x * (uint32_t)kAdamSegment + 4u * threadIdx.x;
  double q[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t i = i0 + (uint32_t)e;
    q[e] = 0.0;
    if (i < P) {
      const float* base = p.flat.g[0];
      uint32_t first = 0;
#pragma unroll
      for (int t = 1; t < kAdamTensors; ++t)
        if (i >= p.flat.off[t]) {
          base = p.flat.g[t];
          first = p.flat.off[t];
        }
      const double g = (double)base[i - first];
      q[e] = g * g;
    }
  }
  const double s = adam_block_sum(q[0], q[1], q[2], q[3], lds);
  if (threadIdx.x == 0) p.part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void wab_adam_mid_kernel(AdamMidParams p) {
  __shared__ double lds[4];
  const uint32_t i = blockIdx.x * (uint32_t)kAdamSegment + 4u * threadIdx.x;
  const double s = adam_block_sum(adam_partial(p.in, p.n_in, i), adam_partial(p.in, p.n_in, i + 1u),
                                  adam_partial(p.in, p.n_in, i + 2u), adam_partial(p.in, p.n_in, i + 3u), lds);
  if (threadIdx.x == 0) p.out[blockIdx.x] = s;
}

// ------------------------------------------------------------------------ the update
__global__ __launch_bounds__(256) void wab_adam_update_kernel(AdamUpdateParams p) {
  __shared__ double lds[4];
  __shared__ float sc[4];
  const double S = adam_total(p.part, p.n_part, lds);
  if (threadIdx.x == 0) {
    const AdamScalars r = adam_scalars(S, p.c, *p.state);
    sc[0] = r.c;
    sc[1] = r.a;
    sc[2] = r.r2;
    sc[3] = r.skip ? 1.0f : 0.0f;
  }
  __syncthreads();
  if (sc[3] != 0.0f) return;  // a non-finite gradient: nothing changes (uniform)
  AdamStep s;
  s.k = p.c;
  s.c = sc[0];
  s.a = sc[1];
  s.r2 = sc[2];
  const PolicyDims& d = p.d;
  const uint32_t stride = gridDim.x * 256u;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < d.w_total; i += stride) {
    if (i < d.w2) adam_layer(s, p.g.w1, p.p.w1, p.m.w1, p.v.w1, d.h1, d.F, d.KS1, p.w + d.w1, i - d.w1);
    else if (i < d.w3) adam_layer(s, p.g.w2, p.p.w2, p.m.w2, p.v.w2, d.h2, d.h1, d.KS2, p.w + d.w2, i - d.w2);
    else if (i < d.wh) adam_layer(s, p.g.w3, p.p.w3, p.m.w3, p.v.w3, d.h3, d.h2, d.KS3, p.w + d.w3, i - d.w3);
    else {
      // the head tile: rows 0 .. A-1 of the action head, row 8 the value head
      const uint32_t e = i - d.wh, j = e & 7u, lane = (e >> 3) & 63u, ks = e >> 9;
      const int n = (int)(lane & 31u), k = 16 * (int)ks + 8 * (int)(lane >> 5) + (int)j;
      if (k < d.h3) {
        if (n < d.A) p.w[i] = (uint16_t)pol_bf16(adam_element(s, p.g.wa, p.p.wa, p.m.wa, p.v.wa, (size_t)n * (size_t)d.h3 + (size_t)k));
        else if (n == kPolicyMaxActions) p.w[i] = (uint16_t)pol_bf16(adam_element(s, p.g.wv, p.p.wv, p.m.wv, p.v.wv, (size_t)k));
      }
    }
  }
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < d.b_total; i += stride) {
    if (i < d.b2) { if ((int)(i - d.b1) < d.h1) p.b[i] = adam_element(s, p.g.b1, p.p.b1, p.m.b1, p.v.b1, i - d.b1); }
    else if (i < d.b3) { if ((int)(i - d.b2) < d.h2) p.b[i] = adam_element(s, p.g.b2, p.p.b2, p.m.b2, p.v.b2, i - d.b2); }
    else if (i < d.bh) { if ((int)(i - d.b3) < d.h3) p.b[i] = adam_element(s, p.g.b3, p.p.b3, p.m.b3, p.v.b3, i - d.b3); }
    else {
      const int n = (int)(i - d.bh);
      if (n < d.A) p.b[i] = adam_element(s, p.g.ba, p.p.ba, p.m.ba, p.v.ba, (size_t)n);
      else if (n == kPolicyMaxActions) p.b[i] = adam_element(s, p.g.bv, p.p.bv, p.m.bv, p.v.bv, 0);
    }
  }
}

// ------------------------------------------------------------------------ the new state
__global__ __launch_bounds__(256) void wab_adam_finish_kernel(AdamFinishParams p) {
  __shared__ double lds[4];
  const double S = adam_total(p.part, p.n_part, lds);
  if (threadIdx.x != 0) return;
  const AdamScalars r = adam_scalars(S, p.c, *p.state);
  p.state->grad_norm = r.norm;
  p.state->clip_scale = r.c;
  if (r.skip) {
    p.state->skipped += 1;
    return;
  }
  p.state->step += 1;
  p.state->beta1_pow = r.b1p;
  p.state->beta2_pow = r.b2p;
}

}  // namespace wab
