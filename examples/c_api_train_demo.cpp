// actor_critic.py's whole training loop through the C-ABI with no Python in the process
// (include/wab.h): 256 envs of the default options, the reference's 449-128-150-128-{5, 1} network
// with weights made up on the host, and three updates of
//   wab_rollout_policy (T = 16) -> wab_policy_act (the value after the last step) -> wab_gae ->
//   wab_whiten -> wab_policy_grad (mean over the rows) -> wab_policy_adam_step (clip at 0.5)
// on one stream, with nothing copied to the host in between.  The demo checks what it can without
// the network on the host: the optimizer's state counts the steps, its beta powers are the
// running products, the clip factor follows from the norm, and every parameter and moment is
// finite.  Prints one line per update and one OK line, or what is wrong and exits non-zero.  With
// a path argument the ten parameters, the ten first and the ten second moments (raw float32, in
// wab_policy_weights' order) and the 48 bytes of the state are also written there
// (tests/test_gpu_adam_capi.py drives the same loop from Python and compares).
//   usage: c_api_train_demo [dump-file]
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/wab.h"

#define CHECK_WAB(x)                                                          \
  do {                                                                        \
    if ((x) != WAB_OK) {                                                      \
      std::fprintf(stderr, "%s failed: %s\n", #x, wab_last_error());          \
      return 1;                                                               \
    }                                                                         \
  } while (0)
#define CHECK_HIP(x)                                                          \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) {                                                   \
      std::fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));     \
      return 1;                                                               \
    }                                                                         \
  } while (0)

namespace {

constexpr int64_t kB = 256;
constexpr int kT = 16, kUpdates = 3, kF = 449, kA = 5;
constexpr uint64_t kSeed = 0x5EEDull;
constexpr double kGamma = 0.99, kLambda = 0.95, kWhitenEps = 1.1920928955078125e-07;
const int kOut[5] = {128, 150, 128, kA, 1}, kIn[5] = {kF, 128, 150, 128, 128};

uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// default_game_options (wab_env.py:11-39)
wab_config default_config() {
  wab_config c;
  std::memset(&c, 0, sizeof(c));
  c.reward_per_turn = 0;
  c.reward_for_being_killed = -1;
  c.reward_for_starving = -1;
  c.reward_for_finishing = 1;
  c.reward_for_eating = 0.1;
  c.lookout_only = 1;
  c.starting_role = 1;  // (neither random: the reference's None)
  c.starting_food = 1.0;
  c.max_turns = 80;
  c.height = 11;
  c.width = 11;
  c.max_berries_per_bush = 200;
  c.bush_power = 100;
  c.turns_to_fill_food = 8;
  c.turns_to_empty_food = 40;
  c.wolf_spawn_margin = 1;
  c.chance_wolf_on_square = 0.001;
  c.wolf_chance_to_despawn = 0.05;
  c.wolves = 1;
  c.wolves_can_move = 1;
  c.autoreset = 1;
  c.bush_thresholds = nullptr;  // computed by wab_create (wab_bush_thresholds)
  return c;
}

// n floats uniform in +-bound, like torch's default Linear init, from one running state
std::vector<float> uniform(uint64_t* state, size_t n, double bound) {
  std::vector<float> v(n);
  for (float& x : v) {
    *state = mix64(*state + 0x9E3779B97F4A7C15ull);
    x = (float)((((double)(*state >> 11) * 0x1p-53) * 2.0 - 1.0) * bound);
  }
  return v;
}

int upload(const std::vector<float>& h, float** d) {
  CHECK_HIP(hipMalloc(d, h.size() * 4));
  CHECK_HIP(hipMemcpy(*d, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

int zeros(size_t n, float** d) {
  CHECK_HIP(hipMalloc(d, n * 4));
  CHECK_HIP(hipMemset(*d, 0, n * 4));
  return 0;
}

wab_policy_weights weights_of(float* const* x) {
  wab_policy_weights w = {x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9]};
  return w;
}

}  // namespace

int main(int argc, char** argv) {
  if (wab_abi_version() != WAB_ABI_VERSION) {
    std::fprintf(stderr, "library ABI %d, header %d\n", wab_abi_version(), WAB_ABI_VERSION);
    return 1;
  }
  wab_config c = default_config();
  wab_handle* h = nullptr;
  CHECK_WAB(wab_create(&c, kB, kSeed, 0, 0, &h));
  if (wab_feature_dim(h) != kF || wab_num_actions(&c) != kA) {
    std::fprintf(stderr, "feature_dim %d, actions %d\n", wab_feature_dim(h), wab_num_actions(&c));
    return 1;
  }

  // the network, its gradients and the optimizer's moments: ten arrays each, weight then bias per layer
  float *prm[10], *grd[10], *mom1[10], *mom2[10];
  size_t count[10];
  uint64_t rng = kSeed;
  for (int l = 0; l < 5; ++l) {
    const double bound = 1.0 / std::sqrt((double)kIn[l]);
    count[2 * l] = (size_t)kOut[l] * (size_t)kIn[l];
    count[2 * l + 1] = (size_t)kOut[l];
    for (int part = 0; part < 2; ++part) {
      const int i = 2 * l + part;
      if (upload(uniform(&rng, count[i], bound), &prm[i]) || zeros(count[i], &grd[i]) || zeros(count[i], &mom1[i]) ||
          zeros(count[i], &mom2[i]))
        return 1;
    }
  }
  const wab_policy_weights params = weights_of(prm), grads = weights_of(grd), exp_avg = weights_of(mom1),
                           exp_avg_sq = weights_of(mom2);
  wab_policy_shape shape = {kF, kOut[0], kOut[1], kOut[2], kA};
  wab_policy* pol = nullptr;
  CHECK_WAB(wab_policy_create(&shape, 0, &pol));

  wab_adam_config adam = {};
  adam.lr = 3e-4;
  adam.beta1 = 0.9;
  adam.beta2 = 0.999;
  adam.eps = 1e-8;
  adam.weight_decay = 0.0;
  adam.max_grad_norm = 0.5;
  adam.decoupled = 0;
  const size_t adam_bytes = wab_policy_adam_workspace(pol);
  if (adam_bytes == 0) {
    std::fprintf(stderr, "wab_policy_adam_workspace: %s\n", wab_last_error());
    return 1;
  }
  void* adam_ws = nullptr;
  wab_adam_state* adam_state = nullptr;  // device; all-zero bytes = a fresh optimizer
  CHECK_HIP(hipMalloc(&adam_ws, adam_bytes));
  CHECK_HIP(hipMalloc(&adam_state, sizeof(wab_adam_state)));
  CHECK_HIP(hipMemset(adam_state, 0, sizeof(wab_adam_state)));
  if (wab_policy_adam_step(pol, &params, &grads, &exp_avg, &exp_avg_sq, &adam, adam_state, adam_ws, adam_bytes,
                           nullptr) != WAB_E_STATE) {
    std::fprintf(stderr, "wab_policy_adam_step before wab_policy_load was not refused\n");
    return 1;
  }
  CHECK_WAB(wab_policy_load(pol, &params, nullptr));
  wab_adam_config bad_adam = adam;
  bad_adam.beta2 = 1.0;
  if (wab_policy_adam_step(pol, &params, &grads, &exp_avg, &exp_avg_sq, &bad_adam, adam_state, adam_ws, adam_bytes,
                           nullptr) != WAB_E_INVALID ||
      wab_policy_adam_step(pol, &params, &grads, &exp_avg, &exp_avg_sq, &adam, adam_state, adam_ws, adam_bytes - 1,
                           nullptr) != WAB_E_INVALID) {
    std::fprintf(stderr, "beta2 = 1 or a workspace one byte short was not refused\n");
    return 1;
  }

  // the segment's buffers
  const size_t n = (size_t)kT * (size_t)kB;
  uint8_t *planes = nullptr, *scal0 = nullptr, *scal = nullptr, *done = nullptr;
  int8_t *actions = nullptr, *scratch_actions = nullptr;
  float *feat = nullptr, *feats = nullptr, *value = nullptr, *last_value = nullptr, *rew = nullptr, *adv = nullptr,
        *tgt = nullptr, *loss = nullptr;
  CHECK_HIP(hipMalloc(&planes, (size_t)kB * 3 * 11 * 11));
  CHECK_HIP(hipMalloc(&scal0, 3 * (size_t)kB));
  CHECK_HIP(hipMalloc(&scal, 3 * n));
  CHECK_HIP(hipMalloc(&done, n));
  CHECK_HIP(hipMalloc(&actions, n));
  CHECK_HIP(hipMalloc(&scratch_actions, (size_t)kB));
  CHECK_HIP(hipMalloc(&feat, (size_t)kB * kF * 4));
  CHECK_HIP(hipMalloc(&feats, n * kF * 4));
  CHECK_HIP(hipMalloc(&value, n * 4));
  CHECK_HIP(hipMalloc(&last_value, (size_t)kB * 4));
  CHECK_HIP(hipMalloc(&rew, n * 4));
  CHECK_HIP(hipMalloc(&adv, n * 4));
  CHECK_HIP(hipMalloc(&tgt, n * 4));
  CHECK_HIP(hipMalloc(&loss, 16));
  const wab_obs obs0 = {planes, scal0, scal0 + kB, scal0 + 2 * kB};
  const wab_obs obs_seq = {nullptr, scal, scal + n, scal + 2 * n};
  const int64_t whiten_bytes = wab_whiten_workspace((int64_t)n);
  wab_policy_loss lcfg = {};
  lcfg.value_coef = 1.0f;
  lcfg.entropy_coef = 0.0f;
  lcfg.value_loss = WAB_VALUE_LOSS_SMOOTH_L1;
  lcfg.scale = (float)(1.0 / (double)n);
  const size_t grad_bytes = wab_policy_grad_workspace(pol, (int64_t)n, 0);
  if (whiten_bytes < 0 || grad_bytes == 0) {
    std::fprintf(stderr, "workspace sizes: %s\n", wab_last_error());
    return 1;
  }
  void *whiten_ws = nullptr, *grad_ws = nullptr;
  CHECK_HIP(hipMalloc(&whiten_ws, (size_t)whiten_bytes + 8));
  CHECK_HIP(hipMalloc(&grad_ws, grad_bytes));

  CHECK_WAB(wab_reset(h, nullptr, &obs0, nullptr));
  CHECK_WAB(wab_featurize(h, &obs0, nullptr, feat, nullptr));
  double b1p = 1.0, b2p = 1.0;
  for (int u = 0; u < kUpdates; ++u) {
    // slice 0 of the stored rows is the row the segment starts from; `feat` ends as the row after it
    CHECK_HIP(hipMemcpyAsync(feats, feat, (size_t)kB * kF * 4, hipMemcpyDeviceToDevice, nullptr));
    CHECK_WAB(wab_rollout_policy(h, pol, feats, kT, &obs_seq, actions, value, nullptr, rew, done, feats, feat, kGamma,
                                 nullptr, nullptr, nullptr));
    CHECK_WAB(wab_policy_act(h, pol, feat, scratch_actions, nullptr, last_value, nullptr));
    CHECK_WAB(wab_gae(h, rew, done, value, last_value, kT, kB, kGamma, kLambda, adv, tgt, nullptr));
    CHECK_WAB(wab_whiten(adv, (int64_t)n, kWhitenEps, adv, whiten_ws, nullptr));
    CHECK_WAB(wab_policy_grad(pol, feats, actions, adv, tgt, (int64_t)n, &lcfg, &grads, loss, nullptr, nullptr,
                              nullptr, grad_ws, grad_bytes, nullptr));
    CHECK_WAB(wab_policy_adam_step(pol, &params, &grads, &exp_avg, &exp_avg_sq, &adam, adam_state, adam_ws, adam_bytes,
                                   nullptr));
    // (read for the report and the checks only: the loop itself never leaves the device)
    float hl[4];
    wab_adam_state hs;
    CHECK_HIP(hipMemcpy(hl, loss, 16, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(&hs, adam_state, sizeof(hs), hipMemcpyDeviceToHost));
    std::printf("update %d: loss %.9g  policy %.9g  value %.9g  entropy %.9g  grad_norm %.9g  clip %.9g\n", u,
                (double)hl[3], (double)hl[0], (double)hl[1], (double)hl[2], (double)hs.grad_norm, (double)hs.clip_scale);
    b1p *= adam.beta1;
    b2p *= adam.beta2;
    const double r = adam.max_grad_norm / ((double)hs.grad_norm + 1e-6);
    const double clip = r < 1.0 ? r : 1.0;
    if (hs.step != (uint64_t)(u + 1) || hs.skipped != 0 || hs.beta1_pow != b1p || hs.beta2_pow != b2p ||
        !std::isfinite(hs.grad_norm) || !(hs.grad_norm > 0.0f) || !std::isfinite(hl[3]) ||
        std::fabs((double)hs.clip_scale - clip) > 1e-6 * clip) {
      std::fprintf(stderr, "update %d: state {step %llu, skipped %llu, beta powers %.17g %.17g}, expected {%d, 0, "
                           "%.17g %.17g}; clip %.9g, from the norm %.9g\n", u, (unsigned long long)hs.step,
                   (unsigned long long)hs.skipped, hs.beta1_pow, hs.beta2_pow, u + 1, b1p, b2p, (double)hs.clip_scale,
                   clip);
      return 1;
    }
  }
  uint64_t bad = 1;
  CHECK_WAB(wab_policy_grad_bad_actions(pol, grad_ws, nullptr, &bad));

  std::FILE* dump = argc > 1 ? std::fopen(argv[1], "wb") : nullptr;
  if (argc > 1 && !dump) {
    std::fprintf(stderr, "cannot write %s\n", argv[1]);
    return 1;
  }
  size_t moved = 0;
  float* const* const sets[3] = {prm, mom1, mom2};
  for (int s = 0; s < 3; ++s)
    for (int i = 0; i < 10; ++i) {
      std::vector<float> x(count[i]);
      CHECK_HIP(hipMemcpy(x.data(), sets[s][i], x.size() * 4, hipMemcpyDeviceToHost));
      for (float v : x) {
        if (!std::isfinite(v)) {
          std::fprintf(stderr, "set %d, tensor %d has a non-finite entry\n", s, i);
          return 1;
        }
        moved += s == 1 && v != 0.0f;
      }
      if (dump) std::fwrite(x.data(), 4, x.size(), dump);
    }
  if (dump) {
    wab_adam_state hs;
    CHECK_HIP(hipMemcpy(&hs, adam_state, sizeof(hs), hipMemcpyDeviceToHost));
    std::fwrite(&hs, sizeof(hs), 1, dump);
    std::fclose(dump);
  }
  if (moved == 0) {
    std::fprintf(stderr, "every first moment is still zero\n");
    return 1;
  }

  CHECK_WAB(wab_policy_destroy(pol));
  CHECK_WAB(wab_destroy(h));
  for (int i = 0; i < 10; ++i)
    for (void* q : {(void*)prm[i], (void*)grd[i], (void*)mom1[i], (void*)mom2[i]}) CHECK_HIP(hipFree(q));
  for (void* q : {(void*)planes, (void*)scal0, (void*)scal, (void*)done, (void*)actions, (void*)scratch_actions,
                  (void*)feat, (void*)feats, (void*)value, (void*)last_value, (void*)rew, (void*)adv, (void*)tgt,
                  (void*)loss, adam_ws, (void*)adam_state, whiten_ws, grad_ws})
    CHECK_HIP(hipFree(q));
  std::printf("OK c_api_train_demo: %lld envs x %d steps x %d updates, rollout -> GAE -> loss and gradients -> Adam "
              "step on one stream (%zu first moments moved)\n", (long long)kB, kT, kUpdates, moved);
  return 0;
}
