// wab_capi_segment.hip — the C-ABI's post-processing of a rollout segment ([T][B] reward, done,
// value): discounted returns, GAE, episode statistics, return normalisation and whitening.
//
// As in wab_capi.hip, nothing here allocates, copies to the host or synchronises.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "wab_host.h"
#include "wab_episodes.h"
#include "wab_advantage.h"

using namespace wab_host;

namespace {

// "no handle": an empty reward table (every float32 reward stands for itself)
wab::RewardTable no_rewards() {
  wab::RewardTable none;
  std::memset(&none, 0, sizeof(none));
  return none;
}

// the device a call without a handle runs on: the current one
hipError_t device_of(const wab_handle* h, int* device) {
  *device = h ? h->device : 0;
  return h ? hipSuccess : hipGetDevice(device);
}

// f(std::integral_constant<int, NE>) for the kernel instance that holds ne inexact rewards
// (inexact_rewards: 0..4, or 8)
template <typename F>
void dispatch_ne(int ne, F&& f) {
  switch (ne) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{});
  }
}
template <int V>
using vec_c = std::integral_constant<int, V>;

// the discounted-return scan: VEC envs per thread, the widest whose grid still gives each of
// the 1024 SIMDs a 64-thread wave and whose rows stay aligned; the reward table reduced to the
// entries whose float32 is not the double itself (the others convert exactly)
// The choice is made here alone, on the host, and launches nothing: launch_returns runs what
// this returns and wab_debug_returns_plan reports it.
struct ReturnsPlan {
  int vec, ne;               // the instance wab_returns_kernel<vec, ne>
  wab::RewardTable inexact;  // its table: the inexact entries, padded to ne
};

// the entries of `tab` whose float32 is not the double itself, and the NE instance that holds
// them (0..4, or 8), padded to it with copies of entry 0 (same key, same value)
wab::RewardTable inexact_rewards(const wab::RewardTable& tab, int* ne) {
  wab::RewardTable inexact = no_rewards();
  for (int k = 0; k < tab.n; ++k) {
    float f;
    std::memcpy(&f, &tab.f32[k], 4);
    if ((double)f != tab.f64[k]) {
      inexact.f32[inexact.n] = tab.f32[k];
      inexact.f64[inexact.n] = tab.f64[k];
      inexact.n++;
    }
  }
  *ne = inexact.n <= 4 ? inexact.n : 8;
  for (int k = inexact.n; k < *ne; ++k) {
    inexact.f32[k] = inexact.f32[0];
    inexact.f64[k] = inexact.f64[0];
  }
  return inexact;
}

ReturnsPlan returns_plan(const float* reward, const uint8_t* done, const float* returns, int64_t B,
                         const wab::RewardTable& tab) {
  ReturnsPlan plan;
  plan.inexact = inexact_rewards(tab, &plan.ne);
  const auto fits = [&](int v) {
    const uintptr_t a = 4u * (uintptr_t)v - 1u;
    return B % v == 0 && B / v >= 64 * 1024 && ((uintptr_t)reward & a) == 0 && ((uintptr_t)returns & a) == 0 &&
           ((uintptr_t)done & (uintptr_t)(v - 1)) == 0;
  };
  plan.vec = fits(4) ? 4 : fits(2) ? 2 : 1;
  return plan;
}

int launch_returns(const float* reward, const uint8_t* done, int32_t T, int64_t B, double gamma,
                   const float* bootstrap, float* returns, const wab::RewardTable& tab, void* stream) {
  const ReturnsPlan plan = returns_plan(reward, done, returns, B, tab);
  const int vec = plan.vec;
  const wab::RewardTable& inexact = plan.inexact;
  const dim3 grid((unsigned)((B / vec + 63) / 64));
  hipStream_t s = (hipStream_t)stream;
  dispatch_ne(plan.ne, [&](auto n) {
    const auto run = [&](auto v) {
      hipLaunchKernelGGL((wab::wab_returns_kernel<decltype(v)::value, decltype(n)::value>), grid, dim3(64), 0, s,
                         reward, done, T, B, gamma, bootstrap, returns, inexact);
    };
    if (vec == 4) run(vec_c<4>{});
    else if (vec == 2) run(vec_c<2>{});
    else run(vec_c<1>{});
  });
  HIP_TRY(hipGetLastError());
  return WAB_OK;
}

// the GAE scan (wab_gae_kernel<vec, ne>, wab_advantage.hip): 2 envs per thread where B is even,
// B / 2 still gives each of the 1024 SIMDs a 64-thread wave, every float row is 8-byte aligned
// and done 2-byte aligned, else 1 (there is no VEC 4: a chunk's registers would not fit); the
// table as in returns_plan.  launch_gae runs what this returns, wab_debug_gae_plan reports it.
ReturnsPlan gae_plan(const float* reward, const uint8_t* done, const float* value, const float* advantage,
                     const float* target, int64_t B, const wab::RewardTable& tab) {
  ReturnsPlan plan;
  plan.inexact = inexact_rewards(tab, &plan.ne);
  const uintptr_t rows = (uintptr_t)reward | (uintptr_t)value | (uintptr_t)advantage | (uintptr_t)target;  // (NULL: 0)
  plan.vec = B % 2 == 0 && B / 2 >= 64 * 1024 && (rows & 7u) == 0 && ((uintptr_t)done & 1u) == 0 ? 2 : 1;
  return plan;
}

int launch_gae(const float* reward, const uint8_t* done, const float* value, const float* last_value, int32_t T,
               int64_t B, double gamma, double lambda, float* advantage, float* target, const wab::RewardTable& tab,
               void* stream) {
  const ReturnsPlan plan = gae_plan(reward, done, value, advantage, target, B, tab);
  const int vec = plan.vec;
  const wab::RewardTable& inexact = plan.inexact;
  const double gl = gamma * lambda;
  const dim3 grid((unsigned)((B / vec + 63) / 64));
  hipStream_t s = (hipStream_t)stream;
  dispatch_ne(plan.ne, [&](auto n) {
    const auto run = [&](auto v) {
      hipLaunchKernelGGL((wab::wab_gae_kernel<decltype(v)::value, decltype(n)::value>), grid, dim3(64), 0, s, reward,
                         done, value, last_value, T, B, gamma, gl, advantage, target, inexact);
    };
    if (vec == 2) run(vec_c<2>{});
    else run(vec_c<1>{});
  });
  HIP_TRY(hipGetLastError());
  return WAB_OK;
}

// [a, a + na) and [b, b + nb) share a byte (a NULL range shares none)
bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return a && b && na && nb && pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" {

int wab_discounted_returns(const float* reward, const uint8_t* done, int32_t T, int64_t B, double gamma,
                           const float* bootstrap, float* returns, void* stream) {
  g_err.clear();
  if (!reward || !done || !returns || T < 0 || B < 0)
    return fail(WAB_E_INVALID, "wab_discounted_returns: bad argument");
  if (T == 0 || B == 0) return WAB_OK;
  return launch_returns(reward, done, T, B, gamma, bootstrap, returns, no_rewards(), stream);
}

int wab_discounted_returns_exact(const wab_handle* h, const float* reward, const uint8_t* done, int32_t T,
                                 int64_t B, double gamma, const float* bootstrap, float* returns, void* stream) {
  g_err.clear();
  if (!h || !reward || !done || !returns || T < 0 || B < 0)
    return fail(WAB_E_INVALID, "wab_discounted_returns_exact: bad argument");
  if (h->rewards.n < 0)
    return fail(WAB_E_INVALID, "wab_discounted_returns_exact: two of the options' rewards round to the same "
                               "float32; the double rewards are not recoverable");
  if (T == 0 || B == 0) return WAB_OK;
  DeviceGuard guard(h->device);
  return launch_returns(reward, done, T, B, gamma, bootstrap, returns, h->rewards, stream);
}

namespace {
// the count table of wab_episode_stats_update (wab_episodes.h): W waves per step, N entries,
// n_tiles tiles; false where the table is larger than a grid can cover
bool episode_table(int32_t T, int64_t B, int64_t* W, int64_t* N, int64_t* n_tiles) {
  *W = (B + 63) / 64;
  *N = (int64_t)T * *W;
  *n_tiles = (*N + wab::kEpTile - 1) / wab::kEpTile;
  return *n_tiles <= 0x7FFFFFFF;
}
}  // namespace

int64_t wab_episode_stats_workspace(int32_t T, int64_t B) {
  g_err.clear();
  int64_t W, N, n_tiles;
  if (T < 0 || B < 1 || B > 0x7FFFFFFF || !episode_table(T, B, &W, &N, &n_tiles))
    return fail(WAB_E_INVALID, "wab_episode_stats_workspace: T >= 0, 1 <= B < 2^31 and T * ceil(B / 64) < 2^39");
  return n_tiles * 8 + N * 4;  // tile_off i64 [n_tiles], then local u32 [N]
}

int wab_episode_stats_update(const wab_handle* h, const float* reward, const uint8_t* done, int32_t T, int64_t B,
                             double* ret, int64_t* length, double* ep_return, int32_t* ep_length, int32_t* ep_env,
                             int32_t* ep_step, int64_t capacity, int64_t* count, void* workspace, void* stream) {
  g_err.clear();
  wab::EpisodeParams q;
  std::memset(&q, 0, sizeof(q));
  if (T < 0 || B < 1 || B > 0x7FFFFFFF || !episode_table(T, B, &q.W, &q.N, &q.n_tiles))
    return fail(WAB_E_INVALID, "wab_episode_stats_update: T >= 0, 1 <= B < 2^31 and T * ceil(B / 64) < 2^39");
  if (!ret || !length || !count || capacity < 0 || (T > 0 && (!reward || !done)))
    return fail(WAB_E_INVALID, "wab_episode_stats_update: bad argument");
  if (capacity > 0 && (!ep_return || !ep_length || !ep_env || !ep_step))
    return fail(WAB_E_INVALID, "wab_episode_stats_update: the record arrays may be NULL with capacity 0 only");
  if (T > 0 && (!workspace || ((uintptr_t)workspace & 7u) != 0))
    return fail(WAB_E_INVALID, "wab_episode_stats_update: workspace must be 8-byte aligned and hold "
                               "wab_episode_stats_workspace(T, B) bytes");
  if (h && h->rewards.n < 0)
    return fail(WAB_E_INVALID, "wab_episode_stats_update: two of the options' rewards round to the same "
                               "float32; the double rewards are not recoverable");
  int ne = 0;
  if (h) q.tab = inexact_rewards(h->rewards, &ne);
  q.reward = reward;
  q.done = done;
  q.T = T;
  q.B = B;
  q.ret = ret;
  q.length = length;
  q.ep_return = ep_return;
  q.ep_length = ep_length;
  q.ep_env = ep_env;
  q.ep_step = ep_step;
  q.capacity = capacity;
  q.count = count;
  q.tile_off = static_cast<int64_t*>(workspace);
  q.local = reinterpret_cast<uint32_t*>(q.tile_off + q.n_tiles);
  int device = 0;
  HIP_TRY(device_of(h, &device));
  DeviceGuard guard(device);
  hipStream_t s = (hipStream_t)stream;
  if (T > 0) hipLaunchKernelGGL(wab::wab_episode_count_kernel, dim3((unsigned)q.n_tiles), dim3(256), 0, s, q);
  hipLaunchKernelGGL(wab::wab_episode_scan_kernel, dim3(1), dim3(256), 0, s, q);  // (T = 0: count = {0, 0})
  if (T > 0)
    dispatch_ne(ne, [&](auto n) {
      hipLaunchKernelGGL((wab::wab_episode_walk_kernel<decltype(n)::value>), dim3((unsigned)q.W), dim3(64), 0, s, q);
    });
  HIP_TRY(hipGetLastError());
  return WAB_OK;
}

int wab_normalize_episode_returns(const float* returns, const uint8_t* done, int32_t T, int64_t B, double eps,
                                  float* out, void* stream) {
  g_err.clear();
  if (!returns || !done || !out || T < 0 || B < 0)
    return fail(WAB_E_INVALID, "wab_normalize_episode_returns: bad argument");
  if (T == 0 || B == 0) return WAB_OK;
  if ((B + 63) / 64 > 0x7FFFFFFF) return fail(WAB_E_INVALID, "wab_normalize_episode_returns: B too large");
  const dim3 grid((unsigned)((B + 63) / 64));
  if (T <= wab::kNormLdsSteps)  // the wave's columns in LDS, T x 64 floats
    hipLaunchKernelGGL(wab::wab_normalize_lds_kernel, grid, dim3(64), (size_t)T * 256u, (hipStream_t)stream, returns,
                       done, T, B, eps, out);
  else
    hipLaunchKernelGGL(wab::wab_normalize_kernel, grid, dim3(64), 0, (hipStream_t)stream, returns, done, T, B, eps,
                       out);
  HIP_TRY(hipGetLastError());
  return WAB_OK;
}

int wab_gae(const wab_handle* h, const float* reward, const uint8_t* done, const float* value,
            const float* last_value, int32_t T, int64_t B, double gamma, double lambda, float* advantage,
            float* target, void* stream) {
  g_err.clear();
  if (!reward || !done || !value || (!advantage && !target) || T < 0 || B < 0)
    return fail(WAB_E_INVALID, "wab_gae: bad argument (reward, done, value and one of advantage, target are "
                               "required; T >= 0, B >= 0)");
  if (h && h->rewards.n < 0)
    return fail(WAB_E_INVALID, "wab_gae: two of the options' rewards round to the same float32; the double rewards "
                               "are not recoverable");
  if (T == 0 || B == 0) return WAB_OK;
  if ((B + 63) / 64 > 0x7FFFFFFF || (uint64_t)B > (~(uint64_t)0 >> 3) / (uint64_t)T)
    return fail(WAB_E_INVALID, "wab_gae: B too large");
  {
    const uint64_t n = (uint64_t)T * (uint64_t)B;
    const void* in[4] = {reward, done, value, last_value};
    const uint64_t in_bytes[4] = {4 * n, n, 4 * n, 4 * (uint64_t)B};
    for (const float* o : {advantage, target})
      for (int k = 0; k < 4; ++k)
        if (ranges_overlap(o, 4 * n, in[k], in_bytes[k]))
          return fail(WAB_E_INVALID, "wab_gae: an output overlaps an input (the scan reads value[t] again as step "
                                     "t - 1's next value)");
    if (ranges_overlap(advantage, 4 * n, target, 4 * n))
      return fail(WAB_E_INVALID, "wab_gae: advantage and target overlap");
  }
  int device = 0;
  HIP_TRY(device_of(h, &device));
  DeviceGuard guard(device);
  return launch_gae(reward, done, value, last_value, T, B, gamma, lambda, advantage, target,
                    h ? h->rewards : no_rewards(), stream);
}

int64_t wab_whiten_workspace(int64_t n) {
  g_err.clear();
  if (n < 0 || n > wab::kWhitenMaxN) return fail(WAB_E_INVALID, "wab_whiten_workspace: 0 <= n <= 2^40");
  return 2 * (int64_t)wab::kWhitenMaxGroups * 8;  // the partial sums of x, then of the squared deviations
}

int wab_whiten(const float* x, int64_t n, double eps, float* out, void* workspace, void* stream) {
  g_err.clear();
  if (n < 0 || n > wab::kWhitenMaxN) return fail(WAB_E_INVALID, "wab_whiten: 0 <= n <= 2^40");
  if (n == 0) return WAB_OK;
  if (!x || !out || !workspace || ((uintptr_t)workspace & 7u) != 0)
    return fail(WAB_E_INVALID, "wab_whiten: x, out and an 8-byte aligned workspace of wab_whiten_workspace(n) bytes "
                               "are required");
  if (out != x && ranges_overlap(x, 4 * (uint64_t)n, out, 4 * (uint64_t)n))
    return fail(WAB_E_INVALID, "wab_whiten: out must be x itself or not overlap it");
  const int64_t tiles = (n + wab::kWhitenTile - 1) / wab::kWhitenTile;
  const dim3 grid((unsigned)std::min<int64_t>(tiles, wab::kWhitenMaxGroups)), block(wab::kWhitenThreads);
  double* psum = static_cast<double*>(workspace);
  double* pss = psum + wab::kWhitenMaxGroups;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(wab::wab_whiten_sum_kernel, grid, block, 0, s, x, n, psum);
  hipLaunchKernelGGL(wab::wab_whiten_dev_kernel, grid, block, 0, s, x, n, (const double*)psum, pss);
  hipLaunchKernelGGL(wab::wab_whiten_out_kernel, grid, block, 0, s, x, n, eps, (const double*)psum, (const double*)pss,
                     out);
  HIP_TRY(hipGetLastError());
  return WAB_OK;
}

int wab_debug_returns_plan(const wab_handle* h, const float* reward, const uint8_t* done, const float* returns,
                           int64_t B, int32_t out[2]) {
  g_err.clear();
  if (!reward || !done || !returns || B < 0 || !out) return fail(WAB_E_INVALID, "wab_debug_returns_plan: bad argument");
  if (h && h->rewards.n < 0)
    return fail(WAB_E_INVALID, "wab_debug_returns_plan: two of the options' rewards round to the same float32; "
                               "wab_discounted_returns_exact refuses this handle");
  const ReturnsPlan plan = returns_plan(reward, done, returns, B, h ? h->rewards : no_rewards());
  out[0] = plan.vec;
  out[1] = plan.ne;
  return WAB_OK;
}

int wab_debug_gae_plan(const wab_handle* h, const float* reward, const uint8_t* done, const float* value,
                       const float* advantage, const float* target, int64_t B, int32_t out[2]) {
  g_err.clear();
  if (!reward || !done || !value || (!advantage && !target) || B < 0 || !out)
    return fail(WAB_E_INVALID, "wab_debug_gae_plan: bad argument");
  if (h && h->rewards.n < 0)
    return fail(WAB_E_INVALID, "wab_debug_gae_plan: two of the options' rewards round to the same float32; wab_gae "
                               "refuses this handle");
  const ReturnsPlan plan = gae_plan(reward, done, value, advantage, target, B, h ? h->rewards : no_rewards());
  out[0] = plan.vec;
  out[1] = plan.ne;
  return WAB_OK;
}

}  // extern "C"
