// wab_snapshot.hip — env state to fixed-size records and back (wab_snapshot_save /
// wab_snapshot_restore, include/wab.h).
//
// The handle keeps its state as arrays with the env innermost (wab_params.h: hdr, food,
// wolves [slots][B], eaten_xy / eaten_rem [cap][B], bushmap); a snapshot is env-major: one
// record of rw dwords per env (SnapLayout), so that any env range is one contiguous slice.
// Both directions are a transposition through LDS, one workgroup per 64 envs:
//   state side   lane = env: consecutive lanes read or write consecutive elements of a row;
//   record side  16-byte units, consecutive lanes consecutive units of the group's records
//                (64 records are one contiguous block of 64 * rw dwords).
// In LDS an env's record starts at a pitch of snap_pitch(rw) dwords.  When 64 records exceed the
// LDS the host gives the launch (wab_capi.hip snapshot_params: 40 KB) the group goes in passes of
// 32 or 16 envs.
//
// The record is canonical: wolf slots >= n_wolves, log entries >= n_eaten, bitmap bits >= W*H
// and the padding are written as 0, and the wide kernel's bitmap (one dword per row, bit j of
// row i) is converted to the bit i*H + j order of the other two kernels.  Neither kernel
// allocates, synchronises the host or uses atomics: each output element has one writer.
#include <hip/hip_runtime.h>

#include "wab_params.h"

namespace wab {

namespace {

constexpr uint32_t kRowPitch = 33;  // LDS dwords per env of the wide kernel's 32 bitmap rows

__device__ __forceinline__ uint32_t low_bits(int n) { return n >= 32 ? ~0u : ((1u << n) - 1u); }

}  // namespace

// state -> records
__global__ __launch_bounds__(256) void wab_snapshot_pack(SnapParams p) {
  extern __shared__ uint32_t lds[];
  const SnapLayout L = snap_layout(p.slots, p.cap, p.WHW);
  const uint32_t pitch = snap_pitch(L.rw), U = L.rw / 4u;
  const uint32_t E = 1u << p.lg_envs, lg = (uint32_t)p.lg_envs, tid = threadIdx.x;
  uint32_t* rec = lds;
  uint32_t* rows = lds + E * pitch;  // wide only
  const int64_t rest = p.n - (int64_t)blockIdx.x * kEnvsPerBlock;
  const uint32_t nb = rest < kEnvsPerBlock ? (uint32_t)rest : (uint32_t)kEnvsPerBlock;
  const uint32_t last_mask = (p.WH & 31) ? low_bits(p.WH & 31) : ~0u;

  for (uint32_t sub = 0; sub < nb; sub += E) {
    const uint32_t ne = nb - sub < E ? nb - sub : E;
    const int64_t r0 = (int64_t)blockIdx.x * kEnvsPerBlock + sub;  // first record of the pass
    const int64_t g0 = p.env0 + r0;                                // its env in the handle
    // header and food; the wide kernel's bitmap rows (env-major: 32 consecutive dwords per env)
    for (uint32_t e = tid; e < ne; e += 256) {
      *reinterpret_cast<uint4*>(&rec[e * pitch]) = p.hdr[g0 + e];
      *reinterpret_cast<uint2*>(&rec[e * pitch + 4u]) = reinterpret_cast<const uint2*>(p.food)[g0 + e];
    }
    if (p.wide) {
      const uint32_t hmask = low_bits(p.H);
      for (uint32_t it = tid; it < ne * 32u; it += 256) {
        const uint32_t e = it >> 5, i = it & 31u;
        rows[e * kRowPitch + i] = i < (uint32_t)p.W ? p.bushmap[(size_t)(g0 + e) * 32u + i] & hmask : 0u;
      }
    }
    __syncthreads();
    // wolf tiles, slot k of env e: item k * E + e
    for (uint32_t it = tid; it < (uint32_t)p.slots << lg; it += 256) {
      const uint32_t e = it & (E - 1u), k = it >> lg;
      if (e >= ne) continue;
      const uint32_t nw = misc_nw(rec[e * pitch + 2u]);
      rec[e * pitch + L.wolf + k] = k < nw ? p.wolves[(int64_t)k * p.B + g0 + e] : 0u;
    }
    // eaten-tile log: the tiles, then the berries left, four entries to a dword
    for (uint32_t it = tid; it < (uint32_t)p.cap << lg; it += 256) {
      const uint32_t e = it & (E - 1u), k = it >> lg;
      if (e >= ne) continue;
      const uint32_t nl = misc_ne(rec[e * pitch + 2u]);
      rec[e * pitch + L.exy + k] = k < nl ? p.eaten_xy[(int64_t)k * p.B + g0 + e] : 0u;
    }
    for (uint32_t it = tid; it < (L.bm - L.erem) << lg; it += 256) {
      const uint32_t e = it & (E - 1u), k = it >> lg;
      if (e >= ne) continue;
      const uint32_t nl = misc_ne(rec[e * pitch + 2u]);
      uint32_t v = 0;
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t row = 4u * k + j;
        if (row < nl && row < (uint32_t)p.cap) v |= (uint32_t)p.eaten_rem[(int64_t)row * p.B + g0 + e] << (8u * j);
      }
      rec[e * pitch + L.erem + k] = v;
    }
    // bush bitmap (bit i*H + j) and the zero padding behind it
    for (uint32_t it = tid; it < (L.rw - L.bm) << lg; it += 256) {
      const uint32_t e = it & (E - 1u), k = it >> lg;
      if (e >= ne) continue;
      uint32_t v = 0;
      if (k < (uint32_t)p.WHW) {
        if (p.wide) {  // bits [32k, 32k + 32) come from the rows i with [i*H, i*H + H) in that range
          const int lo = 32 * (int)k;
          for (int i = lo / p.H; i < p.W && i * p.H < lo + 32; ++i) {
            const uint32_t r = rows[e * kRowPitch + (uint32_t)i];
            const int off = i * p.H - lo;  // in (-H, 32)
            v |= off >= 0 ? r << off : r >> -off;
          }
        } else {
          v = p.bushmap[(int64_t)k * p.B + g0 + e];
          if (k == (uint32_t)p.WHW - 1u) v &= last_mask;
        }
      }
      rec[e * pitch + L.bm + k] = v;
    }
    __syncthreads();
    // records: unit u of env e is unit e * U + u of the pass's block of records
    uint4* out = p.records + (size_t)r0 * U;
    for (uint32_t it = tid; it < ne * U; it += 256) {
      const uint32_t e = it / U, u = it - e * U;
      out[it] = *reinterpret_cast<const uint4*>(&rec[e * pitch + 4u * u]);
    }
    __syncthreads();  // (the next pass rewrites the LDS)
  }
}

// records -> state, for the envs with mask[env] != 0 (or all of [env0, env0 + n))
__global__ __launch_bounds__(256) void wab_snapshot_unpack(SnapParams p) {
  extern __shared__ uint32_t lds[];
  const SnapLayout L = snap_layout(p.slots, p.cap, p.WHW);
  const uint32_t pitch = snap_pitch(L.rw), U = L.rw / 4u;
  const uint32_t E = 1u << p.lg_envs, lg = (uint32_t)p.lg_envs, tid = threadIdx.x;
  uint32_t* rec = lds;
  const int64_t rest = p.n - (int64_t)blockIdx.x * kEnvsPerBlock;
  const uint32_t nb = rest < kEnvsPerBlock ? (uint32_t)rest : (uint32_t)kEnvsPerBlock;

  for (uint32_t sub = 0; sub < nb; sub += E) {
    const uint32_t ne = nb - sub < E ? nb - sub : E;
    const int64_t r0 = (int64_t)blockIdx.x * kEnvsPerBlock + sub;
    const int64_t g0 = p.env0 + r0;
    const uint4* in = p.records + (size_t)r0 * U;
    for (uint32_t it = tid; it < ne * U; it += 256) {
      const uint32_t e = it / U, u = it - e * U;
      *reinterpret_cast<uint4*>(&rec[e * pitch + 4u * u]) = in[it];
    }
    __syncthreads();
    const auto taken = [&](uint32_t e) { return e < ne && (!p.mask || p.mask[g0 + e] != 0); };
    for (uint32_t e = tid; e < ne; e += 256) {
      if (!taken(e)) continue;
      p.hdr[g0 + e] = *reinterpret_cast<const uint4*>(&rec[e * pitch]);
      reinterpret_cast<uint2*>(p.food)[g0 + e] = *reinterpret_cast<const uint2*>(&rec[e * pitch + 4u]);
    }
    for (uint32_t it = tid; it < (uint32_t)p.slots << lg; it += 256) {
      const uint32_t e = it & (E - 1u), k = it >> lg;
      if (taken(e)) p.wolves[(int64_t)k * p.B + g0 + e] = rec[e * pitch + L.wolf + k];
    }
    for (uint32_t it = tid; it < (uint32_t)p.cap << lg; it += 256) {
      const uint32_t e = it & (E - 1u), k = it >> lg;
      if (!taken(e)) continue;
      p.eaten_xy[(int64_t)k * p.B + g0 + e] = rec[e * pitch + L.exy + k];
      p.eaten_rem[(int64_t)k * p.B + g0 + e] = (uint8_t)(rec[e * pitch + L.erem + (k >> 2)] >> (8u * (k & 3u)));
    }
    if (p.wide) {  // row i = bits [i*H, i*H + H); rows >= W of the env's 32 are written as 0
      const uint32_t hmask = low_bits(p.H);
      for (uint32_t it = tid; it < ne * 32u; it += 256) {
        const uint32_t e = it >> 5, i = it & 31u;
        if (!taken(e)) continue;
        uint32_t v = 0;
        if (i < (uint32_t)p.W) {
          const uint32_t bit = i * (uint32_t)p.H, w = bit >> 5, s = bit & 31u;
          v = rec[e * pitch + L.bm + w] >> s;
          if (s != 0 && w + 1u < (uint32_t)p.WHW) v |= rec[e * pitch + L.bm + w + 1u] << (32u - s);
          v &= hmask;
        }
        p.bushmap[(size_t)(g0 + e) * 32u + i] = v;
      }
    } else {
      for (uint32_t it = tid; it < (uint32_t)p.WHW << lg; it += 256) {
        const uint32_t e = it & (E - 1u), k = it >> lg;
        if (taken(e)) p.bushmap[(int64_t)k * p.B + g0 + e] = rec[e * pitch + L.bm + k];
      }
    }
    __syncthreads();
  }
}

}  // namespace wab
