// wab_advantage.h — constants of the advantage kernels (wab_advantage.hip), shared with the host
// side in wab_capi_segment.hip.
#pragma once

#include <stdint.h>

#include "wab_params.h"

namespace wab {

// steps whose loads the GAE scan issues before it runs its chain over them (as kReturnsChunk)
constexpr int kGaeChunk = 32;

// wab_whiten: a workgroup of kWhitenThreads threads sums tiles of kWhitenTile elements (16 per
// thread), tile g, g + G, g + 2 G, ... for workgroup g of G = min(ceil(n / kWhitenTile),
// kWhitenMaxGroups); the workspace holds two arrays of kWhitenMaxGroups doubles (the partial sums
// of x, then of the squared deviations)
constexpr int kWhitenThreads = 256;
constexpr int kWhitenPerThread = 16;
constexpr int kWhitenTile = kWhitenThreads * kWhitenPerThread;
constexpr int kWhitenMaxGroups = 1024;
constexpr int64_t kWhitenMaxN = (int64_t)1 << 40;

// the kernels (wab_advantage.hip), launched from wab_capi_segment.hip
template <int VEC, int NE>
__global__ void wab_gae_kernel(const float* __restrict__ reward, const uint8_t* __restrict__ done,
                               const float* __restrict__ value, const float* __restrict__ last_value, int32_t T,
                               int64_t B, double gamma, double gl, float* __restrict__ advantage,
                               float* __restrict__ target, RewardTable tab);
__global__ void wab_whiten_sum_kernel(const float* x, int64_t n, double* psum);
__global__ void wab_whiten_dev_kernel(const float* x, int64_t n, const double* psum, double* pss);
__global__ void wab_whiten_out_kernel(const float* x, int64_t n, double eps, const double* psum, const double* pss,
                                      float* out);

}  // namespace wab
