// wab_host.h — what the host-side files of the library (wab_capi*.hip, the host part of
// wab_torus.hip) share: the handle and policy objects, the error string, and the helpers more
// than one of them uses.  Internal: everything but the two C structs is in a namespace of hidden
// visibility, so nothing here adds to the library's exports.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/wab.h"
#include "wab_params.h"

struct wab_handle {
  wab::Params p;
  int device = 0;
  int slots = 8;
  int n_blocks = 0;
  size_t lds_bytes = 0;
  int step_kernel = 0;         // KERNEL_BLOCK / KERNEL_SMALL / KERNEL_WIDE
  size_t small_lds_bytes = 0;  // LDS of the small-view kernel
  size_t small_feat_lds_bytes = 0;  // ... with the fused featurizer (wab_step_features), 0: not fusable
  bool reset_done = false;
  std::vector<void*> allocs;
  uint8_t* scratch_planes = nullptr;  // wab_step_features without planes, not fusable (lazy)
  float* bounce_rows = nullptr;       // wab_rollout_policy's 2 T launches: two [B][F] feature rows (lazy)
  size_t lds_max = 0;                 // the device's LDS limit per workgroup (wab_rollout_policy_fused)
  // egocentric observation (allocated by the first wab_egocentric call)
  uint4* ego_path = nullptr;
  uint32_t* ego_diamond = nullptr;
  int ego_cap = 0, ego_n_diamond = 0;
  bool small_g11 = false;    // the small kernel's 11x11 specialisation (geometry_11)
  bool small_rules = false;  // ... with the default options' rules as constants too (default_rules)
  wab::RewardTable rewards;  // exact doubles of the rewards a step returns (n = 0: ambiguous)
  size_t wide_lds_bytes = 0;  // LDS per workgroup of the wide kernel (see wab_create)
  size_t wide_roll_lds_bytes = 0;  // ... of its multi-step build (wab_rollout_wide)
  int32_t obs_placement = WAB_OBS_SAME_BUFFER;  // wab_set_obs_placement: which wide per-step build
  uint64_t rollout_launches = 0, rollout_step_calls = 0;  // wab_counters' host tallies
  uint64_t snapshot_hash = 0;  // wab_snapshot_hash of the options the handle was created with
};

// wab_policy_*: the packed weights of one network on one device (wab_policy.h)
struct wab_policy {
  int device = 0;
  size_t lds_max = 0;  // the device's LDS limit per workgroup
  wab::PolicyDims dims;
  wab::PolicyLds lds;
  uint16_t* w = nullptr;  // bf16 image, dims.w_total elements
  float* b = nullptr;     // padded biases, dims.b_total floats
  bool loaded = false;
  // wab_policy_set_action_rule: host state only, read as kernel arguments by every act and
  // rollout enqueued afterwards (inv_tau = 1.0f / rule.temperature in float32, checked there)
  wab_action_rule rule = {WAB_ACT_SAMPLE, 1.0f};
  float inv_tau = 1.0f;
};

namespace wab_host __attribute__((visibility("hidden"))) {

using wab::Params;

extern thread_local std::string g_err;  // wab_last_error (wab_capi.hip)

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// (`fail` is the including file's: wab_torus.hip keeps its own error string)
#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess)                                                          \
      return fail(WAB_E_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_)); \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

inline bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; }

// The per-kernel maximum of dynamic LDS, on `device`: raised to `bytes` when that is above both
// the 64 KB every kernel has and whatever an earlier call set for this (device, kernel); never
// lowered, since handles that share an instance launch with the largest of their sizes.
hipError_t raise_lds(int device, const void* kernel, size_t bytes);

// One launch of a kernel whose only parameter is the block `p`, through the pointer the
// family's selection function returned (the same pointer raise_lds got); workgroups of 256.
template <typename P>
inline void launch_params(const void* kernel, unsigned blocks, size_t lds, hipStream_t stream, const P& p) {
  void* args[] = {const_cast<P*>(&p)};
  (void)hipLaunchKernel(kernel, dim3(blocks), dim3(256), args, lds, stream);  // (the caller reads hipGetLastError)
}

// Which step kernel a handle runs (wab_create).
enum { KERNEL_BLOCK = 0, KERNEL_SMALL = 1, KERNEL_WIDE = 2 };

// The small-view kernel's instance wab_step_small<slots, g11 ? 11 : 0, feat, roll, rules, policy>
// (wab_capi.hip): the one place that names them.  rules and policy (and with it packed, the policy
// build that stores packed rows) exist for 8 slots at 11x11 only.
const void* small_kernel(int slots, bool g11, bool rules, bool feat, bool roll, bool policy, bool packed = false);
inline const void* small_kernel(const wab_handle* h, bool feat, bool roll, bool policy = false, bool packed = false) {
  return small_kernel(h->slots, h->small_g11, h->small_rules, feat, roll, policy, packed);
}

// where a step's observation, and its actions and results, go
inline void bind_obs(Params& p, const wab_obs* o) {
  p.planes = o->planes;
  p.food_turns = o->food_turns;
  p.role = o->role;
  p.status = o->status;
}
inline void bind_step(Params& p, const int8_t* actions, float* reward, uint8_t* done) {
  p.actions = actions;
  p.reward = reward;
  p.done = done;
}

// Step t of an obs_seq for the per-step fallback loops.  A slice of planes that is not 16-byte
// aligned (B * OB % 16 != 0) is written through a handle-owned buffer (allocated by the first such
// call) and copied to its place on the stream by obs_slice_done.  Without planes: the scalars only.
struct ObsSlice {
  wab_obs o;               // what the step writes
  uint8_t* dst = nullptr;  // where its planes belong
};
int obs_slice(wab_handle* h, const wab_obs* obs_seq, int32_t t, const char* what, ObsSlice* s);
int obs_slice_done(wab_handle* h, const ObsSlice& s, void* stream);

}  // namespace wab_host
