// wab_advantage.hip — advantages of a [T][B] rollout segment (wab_gae) and the whole-batch
// normalisation of a tensor (wab_whiten), include/wab.h.
//
// wab_gae: generalised advantage estimation, the reverse twin of the returns scan
// (wab_returns_kernel, wab_features.hip) with one more input column, on the same exact-reward
// table.  Numeric contract (normative; restated in include/wab.h and DESIGN.md).  Per env b, in
// float64, in this order, with no contraction (-ffp-contract=off):
//
//   gl = gamma * lambda                       (one double multiply, on the host)
//   A = 0.0;  vnext = last_value ? (double)last_value[b] : 0.0
//   for t = T-1 .. 0:
//       v = (double)value[t][b]
//       r = the step's exact double reward (the handle's table, as wab_discounted_returns_exact
//           maps it; h == NULL: (double)reward)
//       d = done[t][b] != 0                   (any nonzero byte)
//       delta = (r + (d ? 0.0 : gamma * vnext)) - v
//       A     = delta + (d ? 0.0 : gl * A)
//       advantage[t][b] = (float)A;  target[t][b] = (float)(A + v)
//       vnext = v
//
// The two selects are part of the contract (a -0.0 reward plus the selected 0.0 is +0.0); NaN and
// infinities propagate as the arithmetic says, up to the next done.
//
// wab_whiten: (x - mean) / (std + eps) over all n elements, std unbiased, in float64, the sums
// in an order that depends on n alone: per-workgroup partial sums in the caller's workspace and a
// combining pass that every workgroup of the next kernel repeats for itself, no atomics.
#include <hip/hip_runtime.h>

#include "wab_device.h"
#include "wab_advantage.h"

namespace wab {

// One chain per env, B innermost, VEC consecutive envs per thread.  As in wab_returns_kernel
// each thread first issues the loads of a whole chunk of kGaeChunk steps, of all three inputs
// and every one unconditional, then runs the chain over the registers.  A chunk holds
// kGaeChunk * (2 VEC + 1) registers (reward, value, the done bytes): 96 at VEC 1, 160 at VEC 2;
// VEC 4 would need 288, past the 256 a wave can address, so there is no such instance.
// `tab` holds the NE rewards whose float32 is not their double (inexact_rewards, wab_capi.hip).
template <int VEC, int NE>
__global__ __launch_bounds__(64) void wab_gae_kernel(const float* __restrict__ reward,
                                                     const uint8_t* __restrict__ done,
                                                     const float* __restrict__ value,
                                                     const float* __restrict__ last_value, int32_t T, int64_t B,
                                                     double gamma, double gl, float* __restrict__ advantage,
                                                     float* __restrict__ target, RewardTable tab) {
  const int64_t b = ((int64_t)blockIdx.x * 64 + threadIdx.x) * VEC;
  if (b >= B) return;
  uint32_t tkey[NE > 0 ? NE : 1];
  double tval[NE > 0 ? NE : 1];
#pragma unroll
  for (int k = 0; k < NE; ++k) {  // (registers, as in wab_returns_kernel)
    tkey[k] = tab.f32[k];
    tval[k] = tab.f64[k];
    opaque(tkey[k]);
    opaque(tval[k]);
  }
  double A[VEC], vnext[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    A[v] = 0.0;
    vnext[v] = last_value ? (double)last_value[b + v] : 0.0;
  }
  for (int32_t hi = T - 1; hi >= 0; hi -= kGaeChunk) {
    const int n = hi + 1 < kGaeChunk ? hi + 1 : kGaeChunk;  // steps hi, hi-1, .., hi-n+1
    float rf[kGaeChunk][VEC], vf[kGaeChunk][VEC];
    uint32_t dn[kGaeChunk];
    // (a step past the segment's start re-reads step 0, unused)
#pragma unroll
    for (int j = 0; j < kGaeChunk; ++j) {
      const int64_t i = (int64_t)(hi - j > 0 ? hi - j : 0) * B + b;
      if constexpr (VEC == 2) {
        const float2 r2 = *reinterpret_cast<const float2*>(reward + i);
        const float2 v2 = *reinterpret_cast<const float2*>(value + i);
        rf[j][0] = r2.x; rf[j][1] = r2.y;
        vf[j][0] = v2.x; vf[j][1] = v2.y;
        dn[j] = *reinterpret_cast<const uint16_t*>(done + i);
      } else {
        rf[j][0] = reward[i];
        vf[j][0] = value[i];
        dn[j] = done[i];
      }
    }
#pragma unroll
    for (int j = 0; j < kGaeChunk; ++j) {
      if (j < n) {
        float oa[VEC], ot[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const double val = (double)vf[j][v];
          double r = (double)rf[j][v];
#pragma unroll
          for (int k = 0; k < NE; ++k)
            if (__float_as_uint(rf[j][v]) == tkey[k]) r = tval[k];
          const bool d = ((dn[j] >> (8 * v)) & 0xFFu) != 0;
          const double gv = gamma * vnext[v];
          const double ga = gl * A[v];
          const double delta = (r + (d ? 0.0 : gv)) - val;
          A[v] = delta + (d ? 0.0 : ga);
          oa[v] = (float)A[v];
          ot[v] = (float)(A[v] + val);
          vnext[v] = val;
        }
        const int64_t i = (int64_t)(hi - j) * B + b;
        if constexpr (VEC == 2) {
          if (advantage) *reinterpret_cast<float2*>(advantage + i) = make_float2(oa[0], oa[1]);
          if (target) *reinterpret_cast<float2*>(target + i) = make_float2(ot[0], ot[1]);
        } else {
          if (advantage) advantage[i] = oa[0];
          if (target) target[i] = ot[0];
        }
      }
    }
  }
}

#define WAB_GAE_INSTANCE(V, N)                                                                                  \
  template __global__ void wab_gae_kernel<V, N>(const float* __restrict__, const uint8_t* __restrict__,        \
                                                const float* __restrict__, const float* __restrict__, int32_t, \
                                                int64_t, double, double, float* __restrict__,                  \
                                                float* __restrict__, RewardTable);
WAB_GAE_INSTANCE(1, 0) WAB_GAE_INSTANCE(1, 1) WAB_GAE_INSTANCE(1, 2) WAB_GAE_INSTANCE(1, 3)
WAB_GAE_INSTANCE(1, 4) WAB_GAE_INSTANCE(1, 8)
WAB_GAE_INSTANCE(2, 0) WAB_GAE_INSTANCE(2, 1) WAB_GAE_INSTANCE(2, 2) WAB_GAE_INSTANCE(2, 3)
WAB_GAE_INSTANCE(2, 4) WAB_GAE_INSTANCE(2, 8)
#undef WAB_GAE_INSTANCE

namespace {

// The workgroup's sum of v, the same value in every thread: each wave by the shuffle tree, then
// the four wave sums in wave order.  `sh` holds 4 doubles.
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();  // (the last call's readers are done with sh)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// the sum of the G partial sums: thread i adds entries i, i + 256, ... in order, then block_sum
__device__ __forceinline__ double combine(const double* part, int G, double* sh) {
  double c = 0.0;
  for (int i = threadIdx.x; i < G; i += kWhitenThreads) c += part[i];
  return block_sum(c, sh);
}

// f(x[i]) summed over the workgroup's tiles: a thread adds its element of each of a tile's
// kWhitenPerThread rows in row order, tile after tile (the loads of a tile issued together, one
// past n re-reading x[n - 1], unused)
template <typename F>
__device__ __forceinline__ double tiles_sum(const float* x, int64_t n, F f) {
  double acc = 0.0;
  for (int64_t tile = blockIdx.x; tile * kWhitenTile < n; tile += gridDim.x) {
    const int64_t base = tile * kWhitenTile + threadIdx.x;
    float xv[kWhitenPerThread];
#pragma unroll
    for (int j = 0; j < kWhitenPerThread; ++j) {
      const int64_t i = base + (int64_t)j * kWhitenThreads;
      xv[j] = x[i < n ? i : n - 1];
    }
#pragma unroll
    for (int j = 0; j < kWhitenPerThread; ++j)
      if (base + (int64_t)j * kWhitenThreads < n) acc += f((double)xv[j]);
  }
  return acc;
}

}  // namespace

// 1. psum[g] = the sum of x over workgroup g's tiles
__global__ __launch_bounds__(kWhitenThreads) void wab_whiten_sum_kernel(const float* x, int64_t n, double* psum) {
  __shared__ double sh[4];
  const double s = block_sum(tiles_sum(x, n, [](double v) { return v; }), sh);
  if (threadIdx.x == 0) psum[blockIdx.x] = s;
}

// 2. mean from psum (every workgroup the same adds), pss[g] = the sum of (x - mean)^2
__global__ __launch_bounds__(kWhitenThreads) void wab_whiten_dev_kernel(const float* x, int64_t n,
                                                                       const double* psum, double* pss) {
  __shared__ double sh[4];
  const double mean = combine(psum, (int)gridDim.x, sh) / (double)n;
  const double s = block_sum(tiles_sum(x, n, [mean](double v) {
                               const double dev = v - mean;
                               return dev * dev;
                             }), sh);
  if (threadIdx.x == 0) pss[blockIdx.x] = s;
}

// 3. out = float32((x - mean) / (sqrt(var) + eps)); n = 1: 0 / 0 = NaN, as torch.std of one
// element.  out may be x: a thread reads the elements it writes, a tile at a time, before it
// writes them.
__global__ __launch_bounds__(kWhitenThreads) void wab_whiten_out_kernel(const float* x, int64_t n, double eps,
                                                                       const double* psum, const double* pss,
                                                                       float* out) {
  __shared__ double sh[4];
  const double mean = combine(psum, (int)gridDim.x, sh) / (double)n;
  const double var = combine(pss, (int)gridDim.x, sh) / (double)(n - 1);
  const double denom = sqrt(var) + eps;
  for (int64_t tile = blockIdx.x; tile * kWhitenTile < n; tile += gridDim.x) {
    const int64_t base = tile * kWhitenTile + threadIdx.x;
    float xv[kWhitenPerThread];
#pragma unroll
    for (int j = 0; j < kWhitenPerThread; ++j) {
      const int64_t i = base + (int64_t)j * kWhitenThreads;
      xv[j] = x[i < n ? i : n - 1];
    }
#pragma unroll
    for (int j = 0; j < kWhitenPerThread; ++j) {
      const int64_t i = base + (int64_t)j * kWhitenThreads;
      if (i < n) out[i] = (float)(((double)xv[j] - mean) / denom);
    }
  }
}

}  // namespace wab
