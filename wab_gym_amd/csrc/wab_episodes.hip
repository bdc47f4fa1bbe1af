// wab_episodes.hip — per-episode statistics and normalisation of a [T][B] rollout segment
// (wab_episode_stats_update / wab_normalize_episode_returns, include/wab.h).
//
// Episode accounting is the forward twin of the returns scan (wab_features.hip): one chain per
// env, walking t = 0..T-1, adding each step's exact double reward to the env's running return
// and closing an episode at every done.  The finished episodes leave compacted, in ascending
// (step, env) order, without atomics:
//   1. wab_episode_count_kernel reads `done` only.  The count table has one entry per (step,
//      wave of 64 envs), row-major, which is the order of the bytes of `done` itself; a
//      workgroup takes kEpTile consecutive entries, counts each with one ballot, scans its tile
//      and writes every entry's exclusive offset within the tile and the tile's sum.
//   2. wab_episode_scan_kernel (one workgroup) scans the tile sums in place and writes
//      count = {finished, min(finished, capacity)}.
//   3. wab_episode_walk_kernel runs the chains, a wave per 64 envs: it issues the loads of
//      kEpChunk steps, then walks them; a done lane writes its record at
//      tile offset + entry offset + its rank among the wave's done lanes (the same ballot).
// Every record has one writer and one place, so the output does not depend on scheduling.
//
// Normalisation (wab_normalize_kernel) is one chain per env too: per segment a sum, a sum of
// squared deviations and the division, each sequential in step order in float64 without
// contraction (-ffp-contract=off), re-reading the segment for the second and third pass.
#include <hip/hip_runtime.h>

#include "wab_device.h"
#include "wab_episodes.h"

namespace wab {

namespace {

// inclusive scan over the wave's 64 lanes
template <typename V>
__device__ __forceinline__ V wave_inclusive(V v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

}  // namespace

__global__ __launch_bounds__(256) void wab_episode_count_kernel(EpisodeParams p) {
  __shared__ uint32_t wsum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // a wave counts 64 consecutive entries, lane j keeping entry e0 + j's count
  const int64_t e0 = (int64_t)blockIdx.x * kEpTile + wv * 64;
  // (step, wave) of the entry being read, advanced entry by entry (wave-uniform)
  int64_t t = e0 / p.W, w = e0 % p.W;
  uint32_t d[64];
  uint64_t live = 0;
  // all 64 loads go out before the first ballot waits for one; each is unconditional (an entry
  // past the table or an env past B reads done[0], masked by its `live` bit)
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    const int64_t b = w * 64 + lane;
    const bool ok = e0 + j < p.N && b < p.B;
    d[j] = p.done[ok ? t * p.B + b : 0];
    live |= (uint64_t)ok << j;
    if (++w == p.W) {
      w = 0;
      ++t;
    }
  }
  uint32_t mine = 0;
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    const uint64_t m = __ballot(((live >> j) & 1u) != 0 && d[j] != 0);
    if (lane == j) mine = (uint32_t)__popcll(m);
  }
  const uint32_t inc = wave_inclusive(mine, lane);
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t off = 0, total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < wv) off += wsum[k];
    total += wsum[k];
  }
  if (e0 + lane < p.N) p.local[e0 + lane] = off + inc - mine;
  if (threadIdx.x == 0) p.tile_off[blockIdx.x] = (int64_t)total;
}

__global__ __launch_bounds__(256) void wab_episode_scan_kernel(EpisodeParams p) {
  __shared__ int64_t wsum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < p.n_tiles; c0 += 256) {
    const int64_t i = c0 + threadIdx.x;
    const int64_t v = i < p.n_tiles ? p.tile_off[i] : 0;
    const int64_t inc = wave_inclusive((long long)v, lane);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int64_t off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < wv) off += wsum[k];
      total += wsum[k];
    }
    if (i < p.n_tiles) p.tile_off[i] = carry + off + inc - v;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    p.count[0] = carry;
    p.count[1] = carry < p.capacity ? carry : p.capacity;
  }
}

template <int NE>
__global__ __launch_bounds__(64) void wab_episode_walk_kernel(EpisodeParams p) {
  const int lane = threadIdx.x;
  const int64_t w = blockIdx.x;
  const int64_t b = w * 64 + lane;
  // a lane past B walks env B - 1 again and writes nothing: the ballots need whole waves
  const bool active = b < p.B;
  const int64_t bb = active ? b : p.B - 1;
  uint32_t tkey[NE > 0 ? NE : 1];
  double tval[NE > 0 ? NE : 1];
#pragma unroll
  for (int k = 0; k < NE; ++k) {  // (registers, as in wab_returns_kernel)
    tkey[k] = p.tab.f32[k];
    tval[k] = p.tab.f64[k];
    opaque(tkey[k]);
    opaque(tval[k]);
  }
  double ret = p.ret[bb];
  int64_t len = p.length[bb];
  for (int64_t lo = 0; lo < p.T; lo += kEpChunk) {
    const int n = p.T - lo < kEpChunk ? (int)(p.T - lo) : kEpChunk;
    float rf[kEpChunk];
    uint32_t dn[kEpChunk];
    // unconditional loads (a step past the segment's end re-reads step T - 1, unused)
#pragma unroll
    for (int j = 0; j < kEpChunk; ++j) {
      const int64_t i = (lo + j < p.T ? lo + j : p.T - 1) * p.B + bb;
      rf[j] = p.reward[i];
      dn[j] = p.done[i];
    }
    // lane j holds where the records of step lo + j of this wave start
    int64_t base_j;
    {
      const int64_t tj = lo + (lane & (kEpChunk - 1));
      const int64_t e = (tj < p.T ? tj : p.T - 1) * p.W + w;
      base_j = p.tile_off[e >> kEpTileShift] + (int64_t)p.local[e];
    }
#pragma unroll
    for (int j = 0; j < kEpChunk; ++j) {
      if (j < n) {
        // the step's exact double reward when the table has it, else the float32 as given
        double r = (double)rf[j];
#pragma unroll
        for (int k = 0; k < NE; ++k)
          if (__float_as_uint(rf[j]) == tkey[k]) r = tval[k];
        ret += r;
        len += 1;
        const bool d = active && dn[j] != 0;
        const uint64_t m = __ballot(d);
        if (m != 0) {  // (wave-uniform)
          const uint32_t blo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base_j, j);
          const uint32_t bhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)base_j >> 32), j);
          if (d) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                            __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            const int64_t idx = (int64_t)(((uint64_t)bhi << 32) | blo) + (int64_t)rank;
            if (idx < p.capacity) {
              p.ep_return[idx] = ret;
              p.ep_length[idx] = (int32_t)len;
              p.ep_env[idx] = (int32_t)b;
              p.ep_step[idx] = (int32_t)(lo + j);
            }
            ret = 0.0;
            len = 0;
          }
        }
      }
    }
  }
  if (active) {
    p.ret[b] = ret;
    p.length[b] = len;
  }
}

template __global__ void wab_episode_walk_kernel<0>(EpisodeParams);
template __global__ void wab_episode_walk_kernel<1>(EpisodeParams);
template __global__ void wab_episode_walk_kernel<2>(EpisodeParams);
template __global__ void wab_episode_walk_kernel<3>(EpisodeParams);
template __global__ void wab_episode_walk_kernel<4>(EpisodeParams);
template __global__ void wab_episode_walk_kernel<8>(EpisodeParams);

// (R - mean) / (std + eps) per episode segment of each env's column (actor_critic.py:145-146,
// torch.std unbiased).  A thread walks its column segment by segment; each of the three passes
// over a segment loads kNormAhead steps before it uses them (a step past the segment re-reads
// an earlier one, unused), so a pass waits once per kNormAhead steps, not once per step.
// `out` may be `x` itself: a segment is read for the last time before its first element is written.
__global__ __launch_bounds__(64) void wab_normalize_kernel(const float* x, const uint8_t* done, int32_t T_,
                                                           int64_t B, double eps, float* out) {
  const int64_t T = T_;
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int64_t s = 0;
  while (s < T) {
    // pass 1: the segment's last step e (its done, or T - 1) and its sum
    double sum = 0.0;
    int64_t e = s;
    bool open = true;
    for (int64_t t0 = s; open; t0 += kNormAhead) {
      float xv[kNormAhead];
      uint32_t dv[kNormAhead];
#pragma unroll
      for (int j = 0; j < kNormAhead; ++j) {
        const int64_t i = (t0 + j < T ? t0 + j : T - 1) * B + b;
        xv[j] = x[i];
        dv[j] = done[i];
      }
#pragma unroll
      for (int j = 0; j < kNormAhead; ++j) {
        if (open) {
          sum += (double)xv[j];
          if (dv[j] != 0 || t0 + j >= T - 1) {
            open = false;
            e = t0 + j;
          }
        }
      }
    }
    const int64_t n = e - s + 1;
    const double mean = sum / (double)n;
    // pass 2: the squared deviations, in step order
    double ss = 0.0;
    for (int64_t t0 = s; t0 <= e; t0 += kNormAhead) {
      float xv[kNormAhead];
#pragma unroll
      for (int j = 0; j < kNormAhead; ++j) xv[j] = x[(t0 + j <= e ? t0 + j : e) * B + b];
#pragma unroll
      for (int j = 0; j < kNormAhead; ++j) {
        if (t0 + j <= e) {
          const double dev = (double)xv[j] - mean;
          ss += dev * dev;
        }
      }
    }
    // (n = 1: 0 / 0 = NaN, as torch.std of one element)
    const double denom = sqrt(ss / (double)(n - 1)) + eps;
    // pass 3
    for (int64_t t0 = s; t0 <= e; t0 += kNormAhead) {
      float xv[kNormAhead];
#pragma unroll
      for (int j = 0; j < kNormAhead; ++j) xv[j] = x[(t0 + j <= e ? t0 + j : e) * B + b];
#pragma unroll
      for (int j = 0; j < kNormAhead; ++j)
        if (t0 + j <= e) out[(t0 + j) * B + b] = (float)(((double)xv[j] - mean) / denom);
    }
    s = e + 1;
  }
}

// The same for segments of at most kNormLdsSteps steps: the wave first brings its 64 columns into
// LDS (loads of 32 steps issued together, as in the walk) and each lane's dones into a bit mask,
// then every lane runs the three passes of its segments out of its own LDS column.  A segment's
// end comes from the mask, so no pass waits for memory to learn its length.  The arithmetic and
// its order are wab_normalize_kernel's: the two give the same bits.
__global__ __launch_bounds__(64) void wab_normalize_lds_kernel(const float* x, const uint8_t* done, int32_t T,
                                                               int64_t B, double eps, float* out) {
  extern __shared__ float col[];  // [T][64]; a lane reads only what it wrote: no barrier
  const int lane = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * 64 + lane;
  const int64_t bb = b < B ? b : B - 1;
  uint64_t mask[kNormLdsSteps / 64] = {};
#pragma unroll
  for (int t0 = 0; t0 < kNormLdsSteps; t0 += 32) {
    if (t0 < T) {  // (wave-uniform)
      float xv[32];
      uint32_t dv[32];
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        const int64_t i = (int64_t)(t0 + j < T ? t0 + j : T - 1) * B + bb;
        xv[j] = x[i];
        dv[j] = done[i];
      }
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        if (t0 + j < T) {
          col[(t0 + j) * 64 + lane] = xv[j];
          if (dv[j] != 0) mask[(t0 + j) >> 6] |= 1ull << ((t0 + j) & 63);
        }
      }
    }
  }
  if (b >= B) return;
  int s = 0;
  while (s < T) {
    // the segment's last step: the first done at or after s, or T - 1
    int e = T - 1;
#pragma unroll
    for (int k = kNormLdsSteps / 64 - 1; k >= 0; --k) {
      const uint64_t m = k > (s >> 6) ? mask[k] : k == (s >> 6) ? mask[k] >> (s & 63) << (s & 63) : 0;
      if (m != 0) e = k * 64 + __builtin_ctzll(m);
    }
    const int n = e - s + 1;
    // (unrolled so that the LDS reads of four steps, and in the last pass their divisions, overlap;
    // the adds keep their order)
    double sum = 0.0;
#pragma unroll 4
    for (int t = s; t <= e; ++t) sum += (double)col[t * 64 + lane];
    const double mean = sum / (double)n;
    double ss = 0.0;
#pragma unroll 4
    for (int t = s; t <= e; ++t) {
      const double dev = (double)col[t * 64 + lane] - mean;
      ss += dev * dev;
    }
    const double denom = sqrt(ss / (double)(n - 1)) + eps;
#pragma unroll 4
    for (int t = s; t <= e; ++t) out[(int64_t)t * B + b] = (float)(((double)col[t * 64 + lane] - mean) / denom);
    s = e + 1;
  }
}

}  // namespace wab
