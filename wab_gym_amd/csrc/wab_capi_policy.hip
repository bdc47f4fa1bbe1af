// wab_capi_policy.hip — the C-ABI's device policy: create, load, act (wab_policy.hip), loss and
// parameter gradients (wab_policy_grad.hip), the optimizer step (wab_policy_opt.hip) and the
// closed-loop rollout wab_rollout_policy (the POLICY instances of wab_step_small.hip, or act and
// step in turns).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>

#include "wab_host.h"
#include "wab_policy_grad.h"
#include "wab_policy_opt.h"

using namespace wab_host;

namespace {

// a handle-owned pair of [B][F] feature rows (16-byte aligned), allocated by the first call that needs it
float* bounce_rows(wab_handle* h, size_t row_floats) {
  if (!h->bounce_rows) {
    DeviceGuard guard(h->device);
    void* ptr = nullptr;
    if (hipMalloc(&ptr, std::max<size_t>(16, 2u * ((row_floats + 3u) & ~(size_t)3u) * 4u)) != hipSuccess) return nullptr;
    h->allocs.push_back(ptr);
    h->bounce_rows = static_cast<float*>(ptr);
  }
  return h->bounce_rows;
}

// which instance of wab_policy_kernel and wab_policy_bwd_kernel a net takes: <true> for h1 > 128,
// two layer-1 tiles per wave
bool policy_two_tiles(const wab::PolicyDims& d) { return d.NT1 > 4; }
const void* policy_kernel(const wab::PolicyDims& d) {
  return policy_two_tiles(d) ? reinterpret_cast<const void*>(&wab::wab_policy_kernel<true>)
                             : reinterpret_cast<const void*>(&wab::wab_policy_kernel<false>);
}
template <int MODE, bool GATHER, bool PACKED>
const void* policy_bwd_instance(bool two) {
  return two ? reinterpret_cast<const void*>(&wab::wab_policy_bwd_kernel<true, MODE, GATHER, PACKED>)
             : reinterpret_cast<const void*>(&wab::wab_policy_bwd_kernel<false, MODE, GATHER, PACKED>);
}
template <bool GATHER, bool PACKED>
const void* policy_bwd_mode(bool two, int mode) {
  return mode == wab::kGradModePpo    ? policy_bwd_instance<wab::kGradModePpo, GATHER, PACKED>(two)
         : mode == wab::kGradModeEval ? policy_bwd_instance<wab::kGradModeEval, GATHER, PACKED>(two)
                                      : policy_bwd_instance<wab::kGradModeGrad, GATHER, PACKED>(two);
}
// (gather: the rows come through an index, wab_policy_*_gather; packed: the features are packed
// bits, wab_policy_*_packed)
const void* policy_bwd_kernel(const wab::PolicyDims& d, int mode, bool gather, bool packed) {
  const bool two = policy_two_tiles(d);
  if (packed) return gather ? policy_bwd_mode<true, true>(two, mode) : policy_bwd_mode<false, true>(two, mode);
  return gather ? policy_bwd_mode<true, false>(two, mode) : policy_bwd_mode<false, false>(two, mode);
}
const void* policy_wgrad_kernel(bool gather, bool packed) {
  if (packed)
    return gather ? reinterpret_cast<const void*>(&wab::wab_policy_wgrad_kernel<true, true>)
                  : reinterpret_cast<const void*>(&wab::wab_policy_wgrad_kernel<false, true>);
  return gather ? reinterpret_cast<const void*>(&wab::wab_policy_wgrad_kernel<true>)
                : reinterpret_cast<const void*>(&wab::wab_policy_wgrad_kernel<false>);
}

// wab_policy_weights as the kernels' set of the ten tensors; P = float* for a set a kernel writes
// (the public struct is const float* throughout: this is the one const_cast)
template <class P>
wab::PolicyTensors<P> tensor_set(const wab_policy_weights& w) {
  const auto c = [](const float* x) { return const_cast<P>(x); };
  return {c(w.w1), c(w.b1), c(w.w2), c(w.b2), c(w.w3), c(w.b3), c(w.wa), c(w.ba), c(w.wv), c(w.bv)};
}

// The check of a set: every pointer set, every pointer 4-byte aligned.  `first`: the first fault in
// the tensors' order (a pointer's NULL before its alignment); `any_null`: a NULL anywhere in the set.
enum SetFault { SET_OK, SET_NULL, SET_MISALIGNED };
struct SetCheck {
  SetFault first;
  bool any_null;
};
SetCheck check_set(const wab_policy_weights& w) {
  SetCheck r = {SET_OK, false};
  for (const float* q : {w.w1, w.b1, w.w2, w.b2, w.w3, w.b3, w.wa, w.ba, w.wv, w.bv}) {
    const SetFault f = !q ? SET_NULL : (reinterpret_cast<uintptr_t>(q) & 3u) != 0 ? SET_MISALIGNED : SET_OK;
    if (r.first == SET_OK) r.first = f;
    r.any_null = r.any_null || !q;
  }
  return r;
}

// What a call on a handle and a policy together needs of the pair: always the same device; with
// PAIR_RUNS the options' action count, loaded weights and a reset handle (the policy is to run on
// the handle's envs); with PAIR_FEATURES the handle's feature rows as the policy's input.
enum : unsigned { PAIR_RUNS = 1, PAIR_FEATURES = 2 };
int check_pair(const wab_handle* h, const wab_policy* p, const char* what, unsigned checks) {
  const std::string w = std::string(what) + ": ";
  if (p->device != h->device)
    return fail(WAB_E_INVALID, w + "the policy is on device " + std::to_string(p->device) + ", the handle on device " +
                                   std::to_string(h->device));
  if ((checks & PAIR_RUNS) && p->dims.A != h->p.n_actions)
    return fail(WAB_E_INVALID, w + "the policy has " + std::to_string(p->dims.A) + " actions, the handle's options " +
                                   std::to_string(h->p.n_actions));
  if (checks & PAIR_FEATURES) {
    const int F = wab_feature_dim(h);
    if (F < 0) return fail(WAB_E_INVALID, w + "the wrapper cannot index this viewport");
    if (p->dims.F != F)
      return fail(WAB_E_INVALID, w + "the policy takes " + std::to_string(p->dims.F) +
                                     " features, the handle's rows have " + std::to_string(F));
  }
  if ((checks & PAIR_RUNS) && !p->loaded) return fail(WAB_E_STATE, w + "call wab_policy_load first");
  if ((checks & PAIR_RUNS) && !h->reset_done)
    return fail(WAB_E_STATE, w + "call wab_reset first (no env has an episode yet)");
  return WAB_OK;
}

// Whether (h, p) takes the one-launch path, and its LDS for T steps (returns scanned in the
// launch or not).  The answer does not depend on T: the limit is tested with the longest
// in-launch returns scan's reward codes.
bool roll_policy_plan(const wab_handle* h, const wab_policy* p, int32_t T, bool fused_returns, wab::RollPolicy* out,
                      std::string* why) {
  const auto no = [&](const char* msg) {
    if (why) *why = msg;
    return false;
  };
  if (h->step_kernel != KERNEL_SMALL || !h->small_g11 || h->slots != 8 || !h->small_feat_lds_bytes)
    return no("the one-launch kernel is built for the 11x11 small-view kernel with 8 wolf slots and the fused "
              "featurizer");
  const int F = wab_feature_dim(h);
  if (F < 0 || p->dims.F != F) return no("the policy's in_features is not the handle's feature length");
  if (((size_t)h->p.B * (size_t)F) % 4u != 0) return no("batch * feature_dim is not a multiple of 4");
  Params q = h->p;
  q.features = reinterpret_cast<float*>(16);  // (layout only)
  q.returns = reinterpret_cast<float*>(16);
  q.n_steps = wab::kMaxFusedReturnSteps;
  const wab::RollPolicy rp = wab::roll_policy_lds(p->dims, wab::small_layout(q).total * 4u);
  if (rp.reg_a + rp.lds.total > h->lds_max)
    return no("the kernel's LDS exceeds the device's limit per workgroup");
  if (out) {
    q.n_steps = T;
    if (!fused_returns) q.returns = nullptr;
    *out = wab::roll_policy_lds(p->dims, wab::small_layout(q).total * 4u);
  }
  return true;
}

}  // namespace

extern "C" {

int wab_policy_create(const wab_policy_shape* shape, int device, wab_policy** out) {
  g_err.clear();
  if (!shape || !out) return fail(WAB_E_INVALID, "wab_policy_create: NULL argument");
  *out = nullptr;
  if (shape->in_features < 1) return fail(WAB_E_INVALID, "wab_policy_create: in_features must be >= 1");
  const int32_t hs[3] = {shape->h1, shape->h2, shape->h3};
  for (int i = 0; i < 3; ++i)
    if (hs[i] < 1 || hs[i] > wab::kPolicyMaxWidth)
      return fail(WAB_E_INVALID, "wab_policy_create: h" + std::to_string(i + 1) + " = " + std::to_string(hs[i]) +
                                     " outside [1, 256]");
  if (shape->n_actions < 2 || shape->n_actions > wab::kPolicyMaxActions)
    return fail(WAB_E_INVALID, "wab_policy_create: n_actions must be in [2, 8]");
  if (shape->in_features > (1 << 20)) return fail(WAB_E_INVALID, "wab_policy_create: in_features above 2^20");
  int n_dev = 0;
  HIP_TRY(hipGetDeviceCount(&n_dev));
  if (device < 0 || device >= n_dev) return fail(WAB_E_INVALID, "wab_policy_create: no such device");
  wab_policy* p = new (std::nothrow) wab_policy();
  if (!p) return fail(WAB_E_NOMEM, "wab_policy_create: out of host memory");
  p->device = device;
  p->dims = wab::policy_dims(shape->in_features, shape->h1, shape->h2, shape->h3, shape->n_actions);
  p->lds = wab::policy_lds(p->dims, wab::kPolicyEnvs, wab::kPolicyLdsBudget);
  DeviceGuard guard(device);
  // the kernel's dynamic LDS can exceed the 64 KB default (the attribute is a maximum per device
  // and kernel, so it is set to the device's limit, whatever other policies on the device need)
  int lds_max = 0;
  hipError_t e = hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
  if (e == hipSuccess && (size_t)lds_max < p->lds.total) {
    delete p;
    return fail(WAB_E_INVALID, "wab_policy_create: the device's LDS is smaller than the kernel needs");
  }
  p->lds_max = (size_t)lds_max;
  if (e == hipSuccess) e = raise_lds(device, policy_kernel(p->dims), p->lds_max);
  // the same for wab_rollout_policy's one-launch instances on this device (both: which one a
  // handle takes depends on its options)
  for (bool rules : {false, true})
    for (bool packed : {false, true})
      if (e == hipSuccess) e = raise_lds(device, small_kernel(8, true, rules, true, true, true, packed), p->lds_max);
  void *w = nullptr, *b = nullptr;
  if (e == hipSuccess) e = hipMalloc(&w, (size_t)p->dims.w_total * 2u);
  if (e == hipSuccess) e = hipMalloc(&b, (size_t)p->dims.b_total * 4u);
  if (e != hipSuccess) {
    if (w) (void)hipFree(w);
    delete p;
    return fail(e == hipErrorOutOfMemory ? WAB_E_NOMEM : WAB_E_HIP,
                std::string("wab_policy_create: ") + hipGetErrorString(e));
  }
  p->w = static_cast<uint16_t*>(w);
  p->b = static_cast<float*>(b);
  *out = p;
  return WAB_OK;
}

int wab_policy_destroy(wab_policy* p) {
  if (!p) return WAB_OK;
  {
    DeviceGuard guard(p->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(p->w);
    (void)hipFree(p->b);
  }
  delete p;
  return WAB_OK;
}

int wab_policy_load(wab_policy* p, const wab_policy_weights* wts, void* stream) {
  g_err.clear();
  if (!p || !wts) return fail(WAB_E_INVALID, "wab_policy_load: NULL argument");
  if (check_set(*wts).any_null)
    return fail(WAB_E_INVALID, "wab_policy_load: every weight and bias pointer must be set");
  wab::PolicyPackParams pp;
  pp.d = p->dims;
  pp.src = tensor_set<const float*>(*wts);
  pp.w = p->w;
  pp.b = p->b;
  DeviceGuard guard(p->device);
  const unsigned blocks = (unsigned)std::min<uint32_t>((p->dims.w_total + 255u) / 256u, 1024u);
  hipLaunchKernelGGL(wab::wab_policy_pack, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pp);
  HIP_TRY(hipGetLastError());
  p->loaded = true;
  return WAB_OK;
}

int wab_policy_act(wab_handle* h, wab_policy* p, const float* features, int8_t* actions, float* probs,
                   float* value, void* stream) {
  g_err.clear();
  if (!h || !p || !features || !actions) return fail(WAB_E_INVALID, "wab_policy_act: NULL argument");
  if (int rc = check_pair(h, p, "wab_policy_act", PAIR_RUNS)) return rc;
  if ((reinterpret_cast<uintptr_t>(features) & 3u) != 0 || (probs && (reinterpret_cast<uintptr_t>(probs) & 3u) != 0) ||
      (value && (reinterpret_cast<uintptr_t>(value) & 3u) != 0))
    return fail(WAB_E_INVALID, "wab_policy_act: features, probs and value must be 4-byte aligned");
  if (h->p.B == 0) return WAB_OK;
  wab::PolicyParams pp;
  pp.d = p->dims;
  pp.lds = p->lds;
  pp.seed = h->p.seed;
  pp.env_base = h->p.env_base;
  pp.B = h->p.B;
  pp.hdr = h->p.hdr;
  pp.features = features;
  pp.actions = actions;
  pp.probs = probs;
  pp.value = value;
  pp.w = p->w;
  pp.b = p->b;
  pp.inv_tau = p->inv_tau;
  pp.act_mode = p->rule.mode;
  DeviceGuard guard(h->device);
  launch_params(policy_kernel(p->dims), (unsigned)((h->p.B + wab::kPolicyEnvs - 1) / wab::kPolicyEnvs), p->lds.total,
                (hipStream_t)stream, pp);
  HIP_TRY(hipGetLastError());
  return WAB_OK;
}

// ---- device policy: the action rule (host state; wab_policy_act and wab_rollout_policy read it) --

int wab_policy_set_action_rule(wab_policy* p, const wab_action_rule* rule) {
  g_err.clear();
  if (!p) return fail(WAB_E_INVALID, "wab_policy_set_action_rule: NULL policy");
  static_assert(sizeof(wab_action_rule) == 8, "wab_action_rule's layout is part of the ABI");
  static_assert(WAB_ACT_SAMPLE == wab::kActSample && WAB_ACT_GREEDY == wab::kActGreedy, "the kernels' modes");
  const wab_action_rule r = rule ? *rule : wab_action_rule{WAB_ACT_SAMPLE, 1.0f};
  if (r.mode != WAB_ACT_SAMPLE && r.mode != WAB_ACT_GREEDY)
    return fail(WAB_E_INVALID, "wab_policy_set_action_rule: mode " + std::to_string(r.mode) +
                                   " is neither WAB_ACT_SAMPLE nor WAB_ACT_GREEDY");
  if (!(std::isfinite(r.temperature) && r.temperature > 0.0f))
    return fail(WAB_E_INVALID, "wab_policy_set_action_rule: temperature must be finite and > 0");
  volatile float inv_v = 1.0f / r.temperature;  // (float32, rounded once: never kept wider)
  const float inv = inv_v;
  if (!std::isnormal(inv))
    return fail(WAB_E_INVALID, "wab_policy_set_action_rule: 1 / temperature is not a normal float32");
  p->rule = r;
  p->inv_tau = inv;
  return WAB_OK;
}

int wab_policy_get_action_rule(const wab_policy* p, wab_action_rule* out) {
  g_err.clear();
  if (!p || !out) return fail(WAB_E_INVALID, "wab_policy_get_action_rule: NULL argument");
  *out = p->rule;
  return WAB_OK;
}

// ---- device policy: loss and parameter gradients (wab_policy_grad.hip) ---------------------

namespace {

// rows per chunk a call runs with: 0 = the default; a positive multiple of 128 otherwise
int64_t grad_chunk_rows(int32_t chunk_rows) {
  if (chunk_rows == 0) return wab::kGradDefaultChunk;
  if (chunk_rows < 0 || chunk_rows % wab::kGradRows != 0) return -1;
  return chunk_rows;
}

}  // namespace

size_t wab_policy_grad_workspace(const wab_policy* p, int64_t N, int32_t chunk_rows) {
  g_err.clear();
  const int64_t cr = grad_chunk_rows(chunk_rows);
  if (!p || N < 0 || N > INT32_MAX || cr < 0) {
    g_err = "wab_policy_grad_workspace: NULL policy, N outside [0, 2^31) or chunk_rows not a multiple of 128";
    return 0;
  }
  // (the size does not shrink with N: a cached workspace serves every call of the policy)
  return wab::grad_workspace(wab::grad_plan(p->dims), cr).total;
}

namespace {

// What the calls on wab_policy_bwd_kernel differ in: wab_policy_grad leaves the ppo fields NULL,
// wab_policy_evaluate loss and grads_out as well; the _gather calls set gather, rows and M
// (features and the per-row inputs are then [M], read through rows [N]); the _packed calls set
// packed and bits in place of features, and gather where they are given an index.
struct GradCall {
  const char* name;
  int mode;  // wab::GradMode
  const float *features, *weight, *target, *old_logp, *old_value;
  const int8_t* actions;
  int64_t N;
  bool gather;
  const int32_t* rows;
  int64_t M;
  bool packed;
  const uint32_t* bits;
  const wab_policy_loss* loss;
  const wab_ppo_config* ppo;
  const wab_policy_weights* grads_out;
  float *loss_out, *ppo_out, *logp, *value, *entropy, *ratio;
  void* workspace;
  size_t workspace_bytes;
  void* stream;
};

// The checks, the parameter blocks and the chunk loop of wab_policy_grad, wab_policy_grad_ppo and
// wab_policy_evaluate, and of their _gather forms.
int policy_grad_run(wab_policy* p, const GradCall& c) {
  const std::string w = std::string(c.name) + ": ";
  const bool eval = c.mode == wab::kGradModeEval, ppo = c.mode == wab::kGradModePpo;
  if (!p || !c.workspace || (!eval && (!c.loss || !c.grads_out)) || (ppo && !c.ppo))
    return fail(WAB_E_INVALID, w + "NULL argument");
  const int64_t N = c.N;
  if (N < 0 || N > INT32_MAX) return fail(WAB_E_INVALID, w + "N outside [0, 2^31)");
  if (c.gather) {
    if (N > 0 && !c.rows) return fail(WAB_E_INVALID, w + "NULL argument (rows is required)");
    if (c.M < 1 || c.M > INT32_MAX) return fail(WAB_E_INVALID, w + "M outside [1, 2^31)");
    if ((reinterpret_cast<uintptr_t>(c.rows) & 3u) != 0) return fail(WAB_E_INVALID, w + "rows must be 4-byte aligned");
  }
  if (c.packed) {
    if (N > 0 && !c.bits) return fail(WAB_E_INVALID, w + "NULL argument (feature_bits is required)");
    if (!aligned16(c.bits)) return fail(WAB_E_INVALID, w + "feature_bits must be 16-byte aligned");
  }
  const bool no_rows = N > 0 && !c.packed && !c.features;
  if (eval) {
    if (no_rows || (N > 0 && c.logp && !c.actions))
      return fail(WAB_E_INVALID, w + "NULL argument (features are required, and actions with logp)");
  } else if (no_rows || (N > 0 && (!c.actions || !c.weight || !c.target))) {
    return fail(WAB_E_INVALID, w + "NULL argument (features, actions, " + (ppo ? "advantage" : "weight") +
                                   " and target are required)");
  }
  int64_t cr = wab::kGradRows;
  if (!eval) {
    if (check_set(*c.grads_out).any_null) return fail(WAB_E_INVALID, w + "every gradient pointer must be set");
    if (c.loss->value_loss != WAB_VALUE_LOSS_SMOOTH_L1 && c.loss->value_loss != WAB_VALUE_LOSS_MSE)
      return fail(WAB_E_INVALID, w + "value_loss must be WAB_VALUE_LOSS_SMOOTH_L1 or WAB_VALUE_LOSS_MSE");
    cr = grad_chunk_rows(c.loss->chunk_rows);
    if (cr < 0) return fail(WAB_E_INVALID, w + "chunk_rows must be 0 or a positive multiple of 128");
  }
  if (ppo) {
    if (!(c.ppo->clip > 0.0f && c.ppo->clip < 1.0f)) return fail(WAB_E_INVALID, w + "clip must be inside (0, 1)");
    if (c.ppo->value_clip != c.ppo->value_clip) return fail(WAB_E_INVALID, w + "value_clip is NaN");
    if (N > 0 && !c.old_logp) return fail(WAB_E_INVALID, w + "NULL argument (old_logp is required)");
    if (c.ppo->value_clip > 0.0f && !c.old_value)
      return fail(WAB_E_INVALID, w + "value_clip > 0 needs old_value");
  }
  if (!p->loaded) return fail(WAB_E_STATE, w + "call wab_policy_load first");
  const wab::GradPlan g = wab::grad_plan(p->dims);
  const wab::GradWorkspace lay = wab::grad_workspace(g, cr);
  // (evaluate keeps nothing in the workspace but the two counts, its first two words)
  const size_t need = eval ? (size_t)256 : lay.total;
  if (c.workspace_bytes < need)
    return fail(WAB_E_INVALID, w + "the workspace has " + std::to_string(c.workspace_bytes) + " bytes, " +
                                   (eval ? std::string("256 are needed")
                                         : "wab_policy_grad_workspace asks for " + std::to_string(need)));
  if ((reinterpret_cast<uintptr_t>(c.workspace) & 255u) != 0)
    return fail(WAB_E_INVALID, w + "the workspace must be 256-byte aligned");
  bool misaligned = !eval && check_set(*c.grads_out).first == SET_MISALIGNED;  // (no NULL in it by now)
  const void* f32s[] = {c.features, c.weight, c.target, c.old_logp, c.old_value, c.loss_out, c.ppo_out, c.logp,
                        c.value, c.entropy, c.ratio};
  for (const void* q : f32s) misaligned = misaligned || (reinterpret_cast<uintptr_t>(q) & 3u) != 0;
  if (misaligned) return fail(WAB_E_INVALID, w + "float arrays must be 4-byte aligned");
  DeviceGuard guard(p->device);
  // wab_policy_bwd_kernel's dynamic LDS can exceed the 64 KB default: as wab_policy_create's
  const void* const bwd = policy_bwd_kernel(p->dims, c.mode, c.gather, c.packed);
  HIP_TRY(raise_lds(p->device, bwd, p->lds_max));
  unsigned char* const base = static_cast<unsigned char*>(c.workspace);
  uint32_t* const bad = reinterpret_cast<uint32_t*>(base + lay.bad);
  uint16_t* const wt = reinterpret_cast<uint16_t*>(base + lay.wt);
  uint16_t* const ws = reinterpret_cast<uint16_t*>(base + lay.ws);
  float* const slab = reinterpret_cast<float*>(base + lay.slab);
  double* const part = reinterpret_cast<double*>(base + lay.part);
  double* const lsum = reinterpret_cast<double*>(base + lay.loss);
  hipStream_t st = (hipStream_t)c.stream;

  if (eval) {
    HIP_TRY(hipMemsetAsync(bad, 0, 2 * sizeof(uint32_t), st));
    cr = ((std::max<int64_t>(N, 1) + wab::kGradRows - 1) / wab::kGradRows) * wab::kGradRows;  // one pass
  } else {
    // the transposed image, from the packed weights as they are at this point of the stream (every
    // call: a flag on the host would go stale under graph replay)
    wab::GradPackParams kp;
    kp.g = g;
    kp.w = p->w;
    kp.wt = wt;
    kp.bad = bad;
    hipLaunchKernelGGL(wab::wab_policy_grad_pack, dim3(std::min<uint32_t>((g.wt_total + 255u) / 256u, 1024u)),
                       dim3(256), 0, st, kp);
    HIP_TRY(hipGetLastError());
  }

  wab::GradBwdParams bp;
  bp.g = g;
  bp.N = N;
  bp.chunk_rows = cr;
  bp.features = c.features;
  bp.actions = c.actions;
  bp.weight = c.weight;
  bp.target = c.target;
  bp.old_logp = c.old_logp;
  bp.old_value = ppo && c.ppo->value_clip > 0.0f ? c.old_value : nullptr;
  bp.rows = c.gather ? c.rows : nullptr;
  bp.M = c.gather ? c.M : 0;
  bp.bits = c.packed ? c.bits : nullptr;
  bp.P = (int32_t)wab::feature_bits_pitch((uint32_t)p->dims.F);
  bp.clip = ppo ? c.ppo->clip : 0.0f;
  bp.value_clip = ppo ? c.ppo->value_clip : 0.0f;
  bp.w = p->w;
  bp.b = p->b;
  bp.wt = eval ? nullptr : wt;
  bp.value_coef = eval ? 0.0f : c.loss->value_coef;
  bp.entropy_coef = eval ? 0.0f : c.loss->entropy_coef;
  bp.mse = !eval && c.loss->value_loss == WAB_VALUE_LOSS_MSE ? 1 : 0;
  bp.logp = c.logp;
  bp.value = c.value;
  bp.entropy = c.entropy;
  bp.ratio = c.ratio;
  bp.ws = eval ? nullptr : ws;
  bp.part = eval ? nullptr : part;
  bp.bad = bad;
  wab::GradWgradParams wp;
  wp.g = g;
  wp.N = N;
  wp.chunk_rows = cr;
  wp.n_terms = ppo ? wab::kGradPpoTerms : wab::kGradLossTerms;
  wp.features = c.features;
  wp.rows = bp.rows;
  wp.M = bp.M;
  wp.bits = bp.bits;
  wp.P = bp.P;
  wp.ws = ws;
  wp.part = part;
  wp.slab = slab;
  wp.loss = lsum;
  for (int64_t row0 = 0; row0 < N; row0 += cr) {
    const int64_t rows = std::min<int64_t>(cr, N - row0);
    const unsigned blocks = (unsigned)((rows + wab::kGradRows - 1) / wab::kGradRows);
    bp.row0 = row0;
    launch_params(bwd, blocks, g.lds.total, st, bp);
    HIP_TRY(hipGetLastError());
    if (eval) continue;
    wp.row0 = row0;
    wp.n_blocks = (int32_t)blocks;
    wp.first = row0 == 0 ? 1 : 0;
    void* wargs[] = {&wp};
    (void)hipLaunchKernel(policy_wgrad_kernel(c.gather, c.packed), dim3((unsigned)g.n_tasks + 1u, (unsigned)g.slabs), dim3(64),
                          wargs, 0, st);
    HIP_TRY(hipGetLastError());
  }
  if (eval) return WAB_OK;

  wab::GradReduceParams rp;
  rp.g = g;
  rp.empty = N == 0 ? 1 : 0;
  rp.accumulate = c.loss->accumulate ? 1 : 0;
  rp.scale = c.loss->scale;
  rp.value_coef = c.loss->value_coef;
  rp.entropy_coef = c.loss->entropy_coef;
  rp.slab = slab;
  rp.loss = lsum;
  rp.out = tensor_set<float*>(*c.grads_out);
  rp.loss_out = c.loss_out;
  rp.ppo_out = ppo ? c.ppo_out : nullptr;
  const wab::PolicyDims& d = p->dims;
  const int64_t elems = (int64_t)d.h1 * (d.F + 1) + (int64_t)d.h2 * (d.h1 + 1) + (int64_t)d.h3 * (d.h2 + 1) +
                        (int64_t)(d.A + 1) * (d.h3 + 1);
  hipLaunchKernelGGL(wab::wab_policy_grad_reduce_kernel, dim3((unsigned)std::min<int64_t>((elems + 255) / 256, 4096)),
                     dim3(256), 0, st, rp);
  HIP_TRY(hipGetLastError());
  return WAB_OK;
}

}  // namespace

namespace {

// Starts an entry point's call: clears the error and fills what every GradCall has (all of
// wab_policy_evaluate's).  A _gather form is its twin's fill, then gather, rows and M.
GradCall grad_call(const char* name, int mode, const float* features, const int8_t* actions, int64_t N, float* logp,
                   float* value, float* entropy, void* workspace, size_t workspace_bytes, void* stream) {
  g_err.clear();
  GradCall c = {};
  c.name = name;
  c.mode = mode;
  c.features = features; c.actions = actions; c.N = N;
  c.logp = logp; c.value = value; c.entropy = entropy;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream;
  return c;
}

// one of the workspace's two counts (GradWorkspace::bad), read once the stream's work is done
int grad_bad_count(const char* name, const wab_policy* p, const void* workspace, int word, void* stream,
                   uint64_t* out) {
  g_err.clear();
  if (!p || !workspace || !out) return fail(WAB_E_INVALID, std::string(name) + ": NULL argument");
  DeviceGuard guard(p->device);
  uint32_t v = 0;
  HIP_TRY(hipMemcpyAsync(&v, static_cast<const uint32_t*>(workspace) + word, sizeof(v), hipMemcpyDeviceToHost,
                         (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  *out = v;
  return WAB_OK;
}

}  // namespace

int wab_policy_grad(wab_policy* p, const float* features, const int8_t* actions, const float* weight,
                    const float* target, int64_t N, const wab_policy_loss* loss, const wab_policy_weights* grads_out,
                    float loss_out[4], float* logp, float* value, float* entropy, void* workspace,
                    size_t workspace_bytes, void* stream) {
  GradCall c = grad_call("wab_policy_grad", wab::kGradModeGrad, features, actions, N, logp, value, entropy, workspace,
                         workspace_bytes, stream);
  c.weight = weight; c.target = target; c.loss = loss; c.grads_out = grads_out; c.loss_out = loss_out;
  return policy_grad_run(p, c);
}

int wab_policy_grad_gather(wab_policy* p, const float* features, const int8_t* actions, const float* weight,
                           const float* target, int64_t N, const wab_policy_loss* loss,
                           const wab_policy_weights* grads_out, float loss_out[4], float* logp, float* value,
                           float* entropy, void* workspace, size_t workspace_bytes, void* stream, const int32_t* rows,
                           int64_t M) {
  GradCall c = grad_call("wab_policy_grad_gather", wab::kGradModeGrad, features, actions, N, logp, value, entropy,
                         workspace, workspace_bytes, stream);
  c.weight = weight; c.target = target; c.loss = loss; c.grads_out = grads_out; c.loss_out = loss_out;
  c.gather = true; c.rows = rows; c.M = M;
  return policy_grad_run(p, c);
}

int wab_policy_grad_ppo(wab_policy* p, const float* features, const int8_t* actions, const float* advantage,
                        const float* target, const float* old_logp, const float* old_value, int64_t N,
                        const wab_policy_loss* loss, const wab_ppo_config* ppo, const wab_policy_weights* grads_out,
                        float loss_out[4], float ppo_out[4], float* logp, float* value, float* entropy, float* ratio,
                        void* workspace, size_t workspace_bytes, void* stream) {
  GradCall c = grad_call("wab_policy_grad_ppo", wab::kGradModePpo, features, actions, N, logp, value, entropy,
                         workspace, workspace_bytes, stream);
  c.weight = advantage; c.target = target; c.loss = loss; c.grads_out = grads_out; c.loss_out = loss_out;
  c.old_logp = old_logp; c.old_value = old_value; c.ppo = ppo; c.ppo_out = ppo_out; c.ratio = ratio;
  return policy_grad_run(p, c);
}

int wab_policy_grad_ppo_gather(wab_policy* p, const float* features, const int8_t* actions, const float* advantage,
                               const float* target, const float* old_logp, const float* old_value, int64_t N,
                               const wab_policy_loss* loss, const wab_ppo_config* ppo,
                               const wab_policy_weights* grads_out, float loss_out[4], float ppo_out[4], float* logp,
                               float* value, float* entropy, float* ratio, void* workspace, size_t workspace_bytes,
                               void* stream, const int32_t* rows, int64_t M) {
  GradCall c = grad_call("wab_policy_grad_ppo_gather", wab::kGradModePpo, features, actions, N, logp, value, entropy,
                         workspace, workspace_bytes, stream);
  c.weight = advantage; c.target = target; c.loss = loss; c.grads_out = grads_out; c.loss_out = loss_out;
  c.old_logp = old_logp; c.old_value = old_value; c.ppo = ppo; c.ppo_out = ppo_out; c.ratio = ratio;
  c.gather = true; c.rows = rows; c.M = M;
  return policy_grad_run(p, c);
}

int wab_policy_evaluate(wab_policy* p, const float* features, const int8_t* actions, int64_t N, float* logp,
                        float* value, float* entropy, void* workspace, size_t workspace_bytes, void* stream) {
  return policy_grad_run(p, grad_call("wab_policy_evaluate", wab::kGradModeEval, features, actions, N, logp, value,
                                      entropy, workspace, workspace_bytes, stream));
}

int wab_policy_evaluate_gather(wab_policy* p, const float* features, const int8_t* actions, int64_t N, float* logp,
                               float* value, float* entropy, void* workspace, size_t workspace_bytes, void* stream,
                               const int32_t* rows, int64_t M) {
  GradCall c = grad_call("wab_policy_evaluate_gather", wab::kGradModeEval, features, actions, N, logp, value, entropy,
                         workspace, workspace_bytes, stream);
  c.gather = true; c.rows = rows; c.M = M;
  return policy_grad_run(p, c);
}

// ---- packed feature rows (include/wab.h, WAB_HAS_PACKED_FEATURES) --------------------------

namespace {

// a _packed call: its _gather twin's fill with the bits in place of the features; an index is optional
void grad_call_packed(GradCall& c, const uint32_t* bits, const int32_t* rows, int64_t M) {
  c.packed = true; c.bits = bits;
  c.gather = rows != nullptr; c.rows = rows; c.M = rows ? M : 0;
}

}  // namespace

int wab_policy_evaluate_packed(wab_policy* p, const uint32_t* feature_bits, const int8_t* actions, int64_t N,
                               float* logp, float* value, float* entropy, void* workspace, size_t workspace_bytes,
                               void* stream, const int32_t* rows, int64_t M) {
  GradCall c = grad_call("wab_policy_evaluate_packed", wab::kGradModeEval, nullptr, actions, N, logp, value, entropy,
                         workspace, workspace_bytes, stream);
  grad_call_packed(c, feature_bits, rows, M);
  return policy_grad_run(p, c);
}

int wab_policy_grad_packed(wab_policy* p, const uint32_t* feature_bits, const int8_t* actions, const float* weight,
                           const float* target, int64_t N, const wab_policy_loss* loss,
                           const wab_policy_weights* grads_out, float loss_out[4], float* logp, float* value,
                           float* entropy, void* workspace, size_t workspace_bytes, void* stream, const int32_t* rows,
                           int64_t M) {
  GradCall c = grad_call("wab_policy_grad_packed", wab::kGradModeGrad, nullptr, actions, N, logp, value, entropy,
                         workspace, workspace_bytes, stream);
  c.weight = weight; c.target = target; c.loss = loss; c.grads_out = grads_out; c.loss_out = loss_out;
  grad_call_packed(c, feature_bits, rows, M);
  return policy_grad_run(p, c);
}

int wab_policy_grad_ppo_packed(wab_policy* p, const uint32_t* feature_bits, const int8_t* actions,
                               const float* advantage, const float* target, const float* old_logp,
                               const float* old_value, int64_t N, const wab_policy_loss* loss,
                               const wab_ppo_config* ppo, const wab_policy_weights* grads_out, float loss_out[4],
                               float ppo_out[4], float* logp, float* value, float* entropy, float* ratio,
                               void* workspace, size_t workspace_bytes, void* stream, const int32_t* rows, int64_t M) {
  GradCall c = grad_call("wab_policy_grad_ppo_packed", wab::kGradModePpo, nullptr, actions, N, logp, value, entropy,
                         workspace, workspace_bytes, stream);
  c.weight = advantage; c.target = target; c.loss = loss; c.grads_out = grads_out; c.loss_out = loss_out;
  c.old_logp = old_logp; c.old_value = old_value; c.ppo = ppo; c.ppo_out = ppo_out; c.ratio = ratio;
  grad_call_packed(c, feature_bits, rows, M);
  return policy_grad_run(p, c);
}

int wab_feature_bits_pitch(int32_t in_features) {
  g_err.clear();
  if (in_features < 1 || in_features > (1 << 20))
    return fail(WAB_E_INVALID, "wab_feature_bits_pitch: in_features outside [1, 2^20]");
  return (int)wab::feature_bits_pitch((uint32_t)in_features);
}

namespace {

constexpr int kPackMaxF = 4096;  // the LDS kernels: 64 rows of F bits, 32 KB

int features_pack_args(const char* name, const void* features, const void* bits, const void* nonbinary,
                       int64_t n_rows, int32_t F) {
  const std::string w = std::string(name) + ": ";
  if (n_rows < 0) return fail(WAB_E_INVALID, w + "n_rows must be >= 0");
  if (F < 1 || F > (1 << 20)) return fail(WAB_E_INVALID, w + "F outside [1, 2^20]");
  if (n_rows > 0 && (!features || !bits)) return fail(WAB_E_INVALID, w + "NULL argument");
  if ((reinterpret_cast<uintptr_t>(features) & 3u) != 0) return fail(WAB_E_INVALID, w + "features must be 4-byte aligned");
  if (!aligned16(bits)) return fail(WAB_E_INVALID, w + "bits must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(nonbinary) & 7u) != 0) return fail(WAB_E_INVALID, w + "nonbinary must be 8-byte aligned");
  return WAB_OK;
}

}  // namespace

int wab_features_pack(const float* features, int64_t n_rows, int32_t F, uint32_t* bits, uint64_t* nonbinary,
                      void* stream) {
  g_err.clear();
  if (int rc = features_pack_args("wab_features_pack", features, bits, nonbinary, n_rows, F)) return rc;
  if (n_rows == 0) return WAB_OK;
  wab::PackParams pp = {};
  pp.F = F;
  pp.P = (int32_t)wab::feature_bits_pitch((uint32_t)F);
  pp.n_rows = n_rows;
  pp.features = features;
  pp.bits = bits;
  pp.nonbinary = reinterpret_cast<unsigned long long*>(nonbinary);
  hipStream_t st = (hipStream_t)stream;
  // (a group's 64 rows start 16-byte aligned where the array does: 64 F floats)
  if (F <= kPackMaxF && aligned16(features)) {
    const size_t lds = ((((size_t)64 * (size_t)F + 31u) >> 5) + 1u) * 4u;
    hipLaunchKernelGGL(wab::wab_pack_rows_kernel, dim3((unsigned)((n_rows + 63) / 64)), dim3(256), lds, st, pp);
  } else {
    hipLaunchKernelGGL(wab::wab_pack_wave_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, st, pp);
  }
  HIP_TRY(hipGetLastError());
  return WAB_OK;
}

int wab_features_unpack(const uint32_t* bits, int64_t n_rows, int32_t F, float* features, void* stream) {
  g_err.clear();
  if (int rc = features_pack_args("wab_features_unpack", features, bits, nullptr, n_rows, F)) return rc;
  if (n_rows == 0) return WAB_OK;
  wab::PackParams pp = {};
  pp.F = F;
  pp.P = (int32_t)wab::feature_bits_pitch((uint32_t)F);
  pp.n_rows = n_rows;
  pp.features_out = features;
  pp.bits = const_cast<uint32_t*>(bits);
  hipStream_t st = (hipStream_t)stream;
  if (F <= kPackMaxF && aligned16(features)) {
    hipLaunchKernelGGL(wab::wab_unpack_rows_kernel, dim3((unsigned)((n_rows + 63) / 64)), dim3(256),
                       (size_t)64 * (size_t)pp.P * 4u, st, pp);
  } else {
    const int64_t blocks = std::min<int64_t>((n_rows * (int64_t)F + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(wab::wab_unpack_elem_kernel, dim3((unsigned)blocks), dim3(256), 0, st, pp);
  }
  HIP_TRY(hipGetLastError());
  return WAB_OK;
}

int wab_policy_grad_bad_rows(const wab_policy* p, const void* workspace, void* stream, uint64_t* out) {
  if (int rc = grad_bad_count("wab_policy_grad_bad_rows", p, workspace, 1, stream, out)) return rc;
  if (*out != 0)
    return fail(WAB_E_INVALID, "wab_policy_grad_gather: " + std::to_string(*out) +
                                   " rows had an index outside the source's rows; they were left out of the loss "
                                   "and the gradients");
  return WAB_OK;
}

int wab_policy_grad_bad_actions(const wab_policy* p, const void* workspace, void* stream, uint64_t* out) {
  if (int rc = grad_bad_count("wab_policy_grad_bad_actions", p, workspace, 0, stream, out)) return rc;
  if (*out != 0)
    return fail(WAB_E_INVALID, "wab_policy_grad: " + std::to_string(*out) + " rows had an action outside [0, " +
                                   std::to_string(p->dims.A) + "); they were left out of the loss and the gradients");
  return WAB_OK;
}

int wab_debug_policy_grad_plan(const wab_policy* p, int32_t chunk_rows, int32_t out[5]) {
  g_err.clear();
  if (!p || !out) return fail(WAB_E_INVALID, "wab_debug_policy_grad_plan: NULL argument");
  const int64_t cr = grad_chunk_rows(chunk_rows);
  if (cr < 0) return fail(WAB_E_INVALID, "wab_debug_policy_grad_plan: chunk_rows must be 0 or a positive multiple of 128");
  const wab::GradPlan g = wab::grad_plan(p->dims);
  out[0] = wab::kGradRows;
  out[1] = g.slabs;
  out[2] = (int32_t)cr;
  out[3] = (int32_t)g.lds.total;
  out[4] = 0;  // wab_policy_wgrad_kernel uses no LDS
  return WAB_OK;
}

// ---- device policy: the optimizer step (wab_policy_opt.hip) --------------------------------

size_t wab_policy_adam_workspace(const wab_policy* p) {
  g_err.clear();
  if (!p) {
    g_err = "wab_policy_adam_workspace: NULL policy";
    return 0;
  }
  return (size_t)wab::adam_levels(wab::adam_flat(p->dims).off[wab::kAdamTensors]).total * sizeof(double);
}

int wab_policy_adam_step(wab_policy* p, const wab_policy_weights* params, const wab_policy_weights* grads,
                         const wab_policy_weights* exp_avg, const wab_policy_weights* exp_avg_sq,
                         const wab_adam_config* cfg, wab_adam_state* state, void* workspace, size_t workspace_bytes,
                         void* stream) {
  g_err.clear();
  if (!p || !params || !grads || !exp_avg || !exp_avg_sq || !cfg || !state || !workspace)
    return fail(WAB_E_INVALID, "wab_policy_adam_step: NULL argument");
  const wab_policy_weights* const sets[4] = {params, grads, exp_avg, exp_avg_sq};
  const char* const set_names[4] = {"params", "grads", "exp_avg", "exp_avg_sq"};
  for (int s = 0; s < 4; ++s) {
    const SetFault f = check_set(*sets[s]).first;
    if (f == SET_NULL)
      return fail(WAB_E_INVALID, std::string("wab_policy_adam_step: every pointer of ") + set_names[s] + " must be set");
    if (f == SET_MISALIGNED) return fail(WAB_E_INVALID, "wab_policy_adam_step: float arrays must be 4-byte aligned");
  }
  // (written so that a NaN is refused too)
  if (!(cfg->lr >= 0.0)) return fail(WAB_E_INVALID, "wab_policy_adam_step: lr must be >= 0");
  if (!(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0) || !(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0))
    return fail(WAB_E_INVALID, "wab_policy_adam_step: beta1 and beta2 must be in [0, 1)");
  if (!(cfg->eps > 0.0)) return fail(WAB_E_INVALID, "wab_policy_adam_step: eps must be > 0");
  if (!(cfg->weight_decay >= 0.0)) return fail(WAB_E_INVALID, "wab_policy_adam_step: weight_decay must be >= 0");
  if (cfg->max_grad_norm != cfg->max_grad_norm)
    return fail(WAB_E_INVALID, "wab_policy_adam_step: max_grad_norm is NaN");
  wab::AdamFlat flat = wab::adam_flat(p->dims);
  const wab::AdamLevels lv = wab::adam_levels(flat.off[wab::kAdamTensors]);
  if (workspace_bytes < (size_t)lv.total * sizeof(double))
    return fail(WAB_E_INVALID, "wab_policy_adam_step: the workspace has " + std::to_string(workspace_bytes) +
                                   " bytes, wab_policy_adam_workspace asks for " +
                                   std::to_string((size_t)lv.total * sizeof(double)));
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 || (reinterpret_cast<uintptr_t>(state) & 7u) != 0)
    return fail(WAB_E_INVALID, "wab_policy_adam_step: the workspace and the state must be 8-byte aligned");
  if (!p->loaded) return fail(WAB_E_STATE, "wab_policy_adam_step: call wab_policy_load first");

  static_assert(sizeof(wab_adam_state) == 48 && sizeof(wab::AdamState) == sizeof(wab_adam_state),
                "wab_adam_state's layout is part of the ABI");
  wab::AdamConsts c;
  c.lr = cfg->lr;
  c.beta1 = cfg->beta1;
  c.beta2 = cfg->beta2;
  c.max_grad_norm = cfg->max_grad_norm;
  c.b1f = (float)cfg->beta1;
  c.omb1 = (float)(1.0 - cfg->beta1);
  c.b2f = (float)cfg->beta2;
  c.omb2 = (float)(1.0 - cfg->beta2);
  c.epsf = (float)cfg->eps;
  c.wdf = (float)cfg->weight_decay;
  c.decayf = (float)(1.0 - cfg->lr * cfg->weight_decay);
  c.decay = cfg->weight_decay != 0.0 ? (cfg->decoupled ? 2 : 1) : 0;

  DeviceGuard guard(p->device);
  hipStream_t st = (hipStream_t)stream;
  double* const part = static_cast<double*>(workspace);
  wab::AdamUpdateParams up;
  up.g = tensor_set<const float*>(*grads);
  wab::AdamNormParams np;
  np.flat = flat;
  static_assert(sizeof(np.flat.g) == sizeof(up.g), "the flat order is the set's field order");
  std::memcpy(np.flat.g, &up.g, sizeof(up.g));
  np.part = part + lv.offset[0];
  hipLaunchKernelGGL(wab::wab_adam_norm_kernel, dim3(lv.count[0]), dim3(256), 0, st, np);
  HIP_TRY(hipGetLastError());
  for (int l = 1; l < lv.n_levels; ++l) {
    wab::AdamMidParams mp;
    mp.in = part + lv.offset[l - 1];
    mp.n_in = lv.count[l - 1];
    mp.out = part + lv.offset[l];
    hipLaunchKernelGGL(wab::wab_adam_mid_kernel, dim3(lv.count[l]), dim3(256), 0, st, mp);
    HIP_TRY(hipGetLastError());
  }
  const int last = lv.n_levels - 1;

  up.d = p->dims;
  up.c = c;
  up.part = part + lv.offset[last];
  up.n_part = lv.count[last];
  up.state = reinterpret_cast<const wab::AdamState*>(state);
  up.p = tensor_set<float*>(*params);
  up.m = tensor_set<float*>(*exp_avg);
  up.v = tensor_set<float*>(*exp_avg_sq);
  up.w = p->w;
  up.b = p->b;
  // one thread per image element up to 2^16 workgroups (16 M elements), a grid-stride loop beyond
  const unsigned blocks = (unsigned)std::min<uint32_t>((p->dims.w_total + 255u) / 256u, 65536u);
  hipLaunchKernelGGL(wab::wab_adam_update_kernel, dim3(blocks), dim3(256), 0, st, up);
  HIP_TRY(hipGetLastError());

  wab::AdamFinishParams fp;
  fp.c = c;
  fp.part = up.part;
  fp.n_part = up.n_part;
  fp.state = reinterpret_cast<wab::AdamState*>(state);
  hipLaunchKernelGGL(wab::wab_adam_finish_kernel, dim3(1), dim3(256), 0, st, fp);
  HIP_TRY(hipGetLastError());
  return WAB_OK;
}

int wab_rollout_policy_fused(const wab_handle* h, const wab_policy* p) {
  g_err.clear();
  if (!h || !p) return fail(WAB_E_INVALID, "wab_rollout_policy_fused: NULL argument");
  if (int rc = check_pair(h, p, "wab_rollout_policy_fused", 0)) return rc;
  return roll_policy_plan(h, p, 1, false, nullptr, &g_err) ? 1 : 0;
}

}  // extern "C"

namespace {

// wab_rollout_policy (features: [T][B][F] or null) and wab_rollout_policy_packed (packed: bits
// [T][B][P] in place of features, which is null)
int rollout_policy_run(const char* name, bool packed, wab_handle* h, wab_policy* p, const float* features0, int32_t T,
                       const wab_obs* obs_seq, int8_t* actions, float* value, float* probs, float* reward,
                       uint8_t* done, float* features, uint32_t* bits, float* features_last, double gamma,
                       const float* bootstrap, float* returns, void* stream) {
  g_err.clear();
  const std::string nm = std::string(name);
  if (!h || !p) return fail(WAB_E_INVALID, nm + ": NULL argument");
  if (packed && !bits) return fail(WAB_E_INVALID, nm + ": NULL argument (feature_bits is required)");
  if (packed && !aligned16(bits)) return fail(WAB_E_INVALID, nm + ": feature_bits must be 16-byte aligned");
  if (T < 0) return fail(WAB_E_INVALID, nm + ": T must be >= 0");
  if (!features0 || !actions || !reward || !done || !features_last || !obs_seq || !obs_seq->food_turns ||
      !obs_seq->role || !obs_seq->status)
    return fail(WAB_E_INVALID, nm + ": NULL argument (features0, actions, reward, done, features_last "
                               "and the scalars of obs_seq are required)");
  if (int rc = check_pair(h, p, name, PAIR_RUNS | PAIR_FEATURES)) return rc;
  const int F = p->dims.F;
  const auto misaligned4 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3u) != 0; };
  if (misaligned4(features0) || (probs && misaligned4(probs)) || (value && misaligned4(value)))
    return fail(WAB_E_INVALID, nm + ": features0, probs and value must be 4-byte aligned");
  if (!aligned16(features_last) || (features && !aligned16(features)))
    return fail(WAB_E_INVALID, nm + ": features and features_last must be 16-byte aligned");
  if (obs_seq->planes && !aligned16(obs_seq->planes))
    return fail(WAB_E_INVALID, nm + ": planes must be 16-byte aligned");
  const int64_t B = h->p.B;
  const size_t OB = (size_t)h->p.OB, BF = (size_t)B * (size_t)F;
  if (T == 0 || B == 0) return WAB_OK;
  // packed: slice 0 is the pack of features0, queued in front of everything else
  const size_t BP = (size_t)B * (size_t)wab::feature_bits_pitch((uint32_t)F);
  if (packed) {
    DeviceGuard guard(h->device);
    if (int rc = wab_features_pack(features0, B, F, bits, nullptr, stream)) return rc;
  }
  const bool fused_returns = returns && T <= wab::kMaxFusedReturnSteps;
  wab::RollPolicy rp;
  bool fused = roll_policy_plan(h, p, T, fused_returns, &rp, nullptr);
  if (obs_seq->planes && ((size_t)B * OB) % 16u != 0) fused = false;  // (the launch's 16-byte obs stores)
  if (returns && !(fused && fused_returns) && h->rewards.n < 0)  // (checked before anything runs)
    return fail(WAB_E_INVALID, nm + ": returns of this segment need the exact-reward scan, and two of "
                               "the options' rewards round to the same float32 (pass returns = NULL)");
  if (fused) {
    // one launch: each workgroup runs its 64 envs through the T steps, the policy between them
    // (wab_step_small<8, 11, FEAT, ROLL, .., POLICY>), the returns of the segment at its end
    Params q = h->p;
    bind_obs(q, obs_seq);
    bind_step(q, actions, reward, done);
    q.features = features_last;  // (non-null: the featurizer is on; the rows go where q.pol says)
    q.n_steps = T;
    if (fused_returns) {
      q.returns = returns;
      q.bootstrap = bootstrap;
      q.gamma = gamma;
    }
    rp.features0 = features0;
    rp.features = features;
    rp.feature_bits = packed ? bits : nullptr;
    rp.features_last = features_last;
    rp.actions = actions;
    rp.probs = probs;
    rp.value = value;
    rp.w = p->w;
    rp.b = p->b;
    rp.inv_tau = p->inv_tau;
    rp.act_mode = p->rule.mode;
    q.pol = rp;
    DeviceGuard guard(h->device);
    ++h->rollout_launches;
    launch_params(small_kernel(h, true, true, true, packed), (unsigned)h->n_blocks, rp.reg_a + rp.lds.total, (hipStream_t)stream, q);
    HIP_TRY(hipGetLastError());
    if (fused_returns || !returns) return WAB_OK;
    return wab_discounted_returns_exact(h, reward, done, T, B, gamma, bootstrap, returns, stream);
  }
  // the 2 T calls; a step's rows go straight to their slice when there is one and it is aligned,
  // else through the handle's pair of rows (alternating: step t reads one, writes the other)
  ++h->rollout_step_calls;
  const bool direct = features && (BF * 4u) % 16u == 0;
  float* bounce = nullptr;
  if (!direct && T > 1) {
    bounce = bounce_rows(h, BF);
    if (!bounce) return fail(WAB_E_NOMEM, nm + ": hipMalloc");
  }
  const size_t bounce_stride = (BF + 3u) & ~(size_t)3u;
  if (features && features != features0) {
    DeviceGuard guard(h->device);
    HIP_TRY(hipMemcpyAsync(features, features0, BF * 4u, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  const float* cur = features0;
  for (int32_t t = 0; t < T; ++t) {
    const size_t tb = (size_t)t * (size_t)B;
    int rc = wab_policy_act(h, p, cur, actions + tb, probs ? probs + tb * (size_t)p->dims.A : nullptr,
                            value ? value + tb : nullptr, stream);
    if (rc != WAB_OK) return rc;
    ObsSlice s;
    if ((rc = obs_slice(h, obs_seq, t, name, &s)) != WAB_OK) return rc;
    float* slice = features && t + 1 < T ? features + (size_t)(t + 1) * BF : nullptr;
    float* dst = t + 1 == T ? features_last : direct ? slice : bounce + (size_t)(t & 1) * bounce_stride;
    rc = wab_step_features(h, actions + tb, &s.o, reward + tb, done + tb, dst, stream);
    if (rc != WAB_OK) return rc;
    if ((rc = obs_slice_done(h, s, stream)) != WAB_OK) return rc;
    if (slice && dst != slice) {
      DeviceGuard guard(h->device);
      HIP_TRY(hipMemcpyAsync(slice, dst, BF * 4u, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    if (packed && t + 1 < T) {
      DeviceGuard guard(h->device);
      if ((rc = wab_features_pack(dst, B, F, bits + (size_t)(t + 1) * BP, nullptr, stream)) != WAB_OK) return rc;
    }
    cur = dst;
  }
  if (!returns) return WAB_OK;
  return wab_discounted_returns_exact(h, reward, done, T, B, gamma, bootstrap, returns, stream);
}

}  // namespace

extern "C" {

int wab_rollout_policy(wab_handle* h, wab_policy* p, const float* features0, int32_t T, const wab_obs* obs_seq,
                       int8_t* actions, float* value, float* probs, float* reward, uint8_t* done, float* features,
                       float* features_last, double gamma, const float* bootstrap, float* returns, void* stream) {
  return rollout_policy_run("wab_rollout_policy", false, h, p, features0, T, obs_seq, actions, value, probs, reward,
                            done, features, nullptr, features_last, gamma, bootstrap, returns, stream);
}

int wab_rollout_policy_packed(wab_handle* h, wab_policy* p, const float* features0, int32_t T, const wab_obs* obs_seq,
                              int8_t* actions, float* value, float* probs, float* reward, uint8_t* done,
                              uint32_t* feature_bits, float* features_last, double gamma, const float* bootstrap,
                              float* returns, void* stream) {
  return rollout_policy_run("wab_rollout_policy_packed", true, h, p, features0, T, obs_seq, actions, value, probs,
                            reward, done, nullptr, feature_bits, features_last, gamma, bootstrap, returns, stream);
}

int wab_debug_policy_plan(const wab_policy* p, int32_t out[5]) {
  g_err.clear();
  if (!p || !out) return fail(WAB_E_INVALID, "wab_debug_policy_plan: NULL argument");
  out[0] = p->lds.n_chunks;
  out[1] = p->lds.KC;
  out[2] = 16 * p->dims.KS1 - (p->lds.n_chunks - 1) * p->lds.KC;
  out[3] = (int32_t)p->lds.total;
  out[4] = policy_two_tiles(p->dims) ? 1 : 0;
  return WAB_OK;
}

}  // extern "C"
