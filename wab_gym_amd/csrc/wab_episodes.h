// wab_episodes.h — parameters of the episode accounting and normalisation kernels
// (wab_episodes.hip), shared with the host side in wab_capi_segment.hip.
#pragma once

#include <stdint.h>

#include "wab_params.h"

namespace wab {

// The count table of a [T][B] segment has one entry per (step, wave of 64 envs), row-major:
// entry t * W + w counts the dones of envs [64 w, 64 w + 64) at step t.  The count kernel scans
// it in tiles of kEpTile entries (4 waves x 64 entries), the scan kernel scans the tile sums.
constexpr int kEpTile = 256;
constexpr int kEpTileShift = 8;
// steps whose loads the walk issues before it runs its chain over them (as kReturnsChunk)
constexpr int kEpChunk = 32;
// steps the normalisation loads ahead in each of its three passes over a segment
constexpr int kNormAhead = 8;
// segments of at most this many steps are normalised out of LDS (wab_normalize_lds_kernel)
constexpr int kNormLdsSteps = 128;

struct EpisodeParams {
  const float* reward;   // [T][B]
  const uint8_t* done;   // [T][B]
  int32_t T;
  int64_t B;
  int64_t W;             // waves per step, ceil(B / 64)
  int64_t N;             // count-table entries, T * W
  int64_t n_tiles;       // ceil(N / kEpTile)
  double* ret;           // [B] running return, in and out
  int64_t* length;       // [B] running length, in and out
  double* ep_return;     // [capacity] records, ascending (step, env); NULL with capacity 0
  int32_t* ep_length;
  int32_t* ep_env;
  int32_t* ep_step;
  int64_t capacity;
  int64_t* count;        // {finished, written}
  int64_t* tile_off;     // workspace: [n_tiles] tile sums, scanned in place to exclusive offsets
  uint32_t* local;       // workspace: [N] exclusive offset of each entry within its tile
  RewardTable tab;       // the inexact rewards, padded to the kernel's NE (wab_returns_kernel)
};

// the kernels (wab_episodes.hip), launched from wab_capi_segment.hip
__global__ void wab_episode_count_kernel(EpisodeParams p);
__global__ void wab_episode_scan_kernel(EpisodeParams p);
template <int NE>
__global__ void wab_episode_walk_kernel(EpisodeParams p);
__global__ void wab_normalize_kernel(const float* x, const uint8_t* done, int32_t T, int64_t B, double eps, float* out);
__global__ void wab_normalize_lds_kernel(const float* x, const uint8_t* done, int32_t T, int64_t B, double eps,
                                         float* out);

}  // namespace wab
