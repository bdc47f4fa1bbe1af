// wab_advantage.h — constants of the advantage kernels (wab_advantage.hip), shared with the host
// side in wab_capi.hip.
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

}  // namespace wab
