// A closed loop through the C-ABI with no Python in the process (include/wab.h: wab_policy_*):
// 200 envs, the reference's 449-128-150-128-{5, 1} network with weights made up on the host.
// Each step is two launches, wab_policy_act (probs, value, sampled action) and wab_step_features
// (the step and the next features), with nothing copied to the host in between.  The demo then
// checks on the host what a caller can check without the network: every probs row sums to 1, and
// every action is the sampling rule's function of that row and the keyed draw of the env's
// (episode, turn).  Prints one OK line, or the first difference and exits non-zero.
//   usage: c_api_policy_demo [seed]
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

constexpr int64_t kB = 200;
constexpr int kSteps = 20, kA = 5;

uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}
// the keyed uniform of site 11 at tile (0, 0), k = 0 (oracle/keyed_rng.py)
double policy_u(uint64_t seed, uint64_t env, uint32_t episode, int32_t turn) {
  const uint64_t ek = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15ull) ^ env) ^ (uint64_t)episode);
  const uint32_t b0 = (uint32_t)ek, b1 = (uint32_t)(ek >> 32);
  const uint32_t ts = 11u | (((uint32_t)turn & 0xFFFFFu) << 12);
  const uint32_t h1 = fmix32(0u ^ b0);
  const uint32_t hi = fmix32(h1 ^ ts ^ b1);
  const uint32_t lo = fmix32(h1 ^ ((ts << 16) | (ts >> 16)) ^ b0 ^ 0x9E3779B9u);
  return (double)(((uint64_t)hi << 21) | (lo >> 11)) * 0x1p-53;
}

// a Linear layer's weights and bias, uniform in +-1/sqrt(in) like torch's default, on the device
int make_linear(uint64_t* state, int out, int in, float** w, float** b) {
  std::vector<float> hw((size_t)out * in), hb((size_t)out);
  const double bound = 1.0 / std::sqrt((double)in);
  auto next = [&]() {
    *state = mix64(*state + 0x9E3779B97F4A7C15ull);
    return (float)((((double)(*state >> 11) * 0x1p-53) * 2.0 - 1.0) * bound);
  };
  for (float& v : hw) v = next();
  for (float& v : hb) v = next();
  CHECK_HIP(hipMalloc(w, hw.size() * 4));
  CHECK_HIP(hipMalloc(b, hb.size() * 4));
  CHECK_HIP(hipMemcpy(*w, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(*b, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 0x5EEDull;

  wab_config c = {};  // default_game_options (wab_env.py:11-39), short episodes
  c.reward_for_being_killed = -1;
  c.reward_for_starving = -1;
  c.reward_for_finishing = 1;
  c.reward_for_eating = 0.1;
  c.lookout_only = 1;
  c.starting_role = 1;
  c.starting_role_random = 1;
  c.starting_food_random = 1;
  c.starting_food = 1.0;
  c.max_turns = 8;
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

  wab_handle* h = nullptr;
  CHECK_WAB(wab_create(&c, kB, seed, 0, 0, &h));
  const int F = wab_feature_dim(h);
  if (F != 449) {
    std::printf("wab_feature_dim: %d\n", F);
    return 1;
  }
  uint8_t *planes = nullptr, *scal = nullptr, *done = nullptr;
  int8_t* act = nullptr;
  float *rew = nullptr, *feat = nullptr, *probs = nullptr, *value = nullptr;
  CHECK_HIP(hipMalloc(&planes, kB * 3 * 11 * 11));
  CHECK_HIP(hipMalloc(&scal, 3 * kB));
  CHECK_HIP(hipMalloc(&done, kB));
  CHECK_HIP(hipMalloc(&act, kB));
  CHECK_HIP(hipMalloc(&rew, 4 * kB));
  CHECK_HIP(hipMalloc(&feat, 4 * kB * F));
  CHECK_HIP(hipMalloc(&probs, 4 * kB * kA));
  CHECK_HIP(hipMalloc(&value, 4 * kB));
  const wab_obs obs = {planes, scal, scal + kB, scal + 2 * kB};
  const wab_obs no_planes = {nullptr, scal, scal + kB, scal + 2 * kB};

  // the network: refused shapes first, then the reference's
  wab_policy* pol = nullptr;
  wab_policy_shape shape = {F, 128, 257, 128, kA};
  if (wab_policy_create(&shape, 0, &pol) != WAB_E_INVALID) {
    std::printf("a width of 257 was not refused\n");
    return 1;
  }
  shape.h2 = 150;
  CHECK_WAB(wab_policy_create(&shape, 0, &pol));
  if (wab_policy_act(h, pol, feat, act, probs, value, nullptr) != WAB_E_STATE) {
    std::printf("wab_policy_act before wab_policy_load was not refused\n");
    return 1;
  }
  wab_policy_weights w = {};
  float *w1, *b1, *w2, *b2, *w3, *b3, *wa, *ba, *wv, *bv;
  uint64_t state = seed;
  if (make_linear(&state, 128, F, &w1, &b1) || make_linear(&state, 150, 128, &w2, &b2) ||
      make_linear(&state, 128, 150, &w3, &b3) || make_linear(&state, kA, 128, &wa, &ba) ||
      make_linear(&state, 1, 128, &wv, &bv))
    return 1;
  w.w1 = w1; w.b1 = b1; w.w2 = w2; w.b2 = b2; w.w3 = w3; w.b3 = b3; w.wa = wa; w.ba = ba; w.wv = wv; w.bv = bv;
  CHECK_WAB(wab_policy_load(pol, &w, nullptr));

  CHECK_WAB(wab_reset(h, nullptr, &obs, nullptr));
  CHECK_WAB(wab_featurize(h, &obs, nullptr, feat, nullptr));
  std::vector<float> hp((size_t)kB * kA), hv((size_t)kB);
  std::vector<int8_t> ha((size_t)kB);
  std::vector<int32_t> turn((size_t)kB);
  std::vector<uint32_t> episode((size_t)kB);
  long long counts[kA] = {};
  uint32_t max_episode = 0;
  for (int t = 0; t < kSteps; ++t) {
    // (the state is read for the check only: the loop itself never leaves the device)
    CHECK_WAB(wab_get_state(h, nullptr, nullptr, nullptr, turn.data(), nullptr, episode.data(), nullptr));
    CHECK_WAB(wab_policy_act(h, pol, feat, act, probs, value, nullptr));
    CHECK_WAB(wab_step_features(h, act, &no_planes, rew, done, feat, nullptr));
    CHECK_HIP(hipMemcpy(hp.data(), probs, hp.size() * 4, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(hv.data(), value, hv.size() * 4, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(ha.data(), act, ha.size(), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < kB; ++i) {
      const float* p = &hp[(size_t)i * kA];
      double c_k = 0.0, sum = 0.0;
      const double u = policy_u(seed, (uint64_t)i, episode[(size_t)i], turn[(size_t)i]);
      int a = 0;
      for (int k = 0; k < kA; ++k) {
        if (!(p[k] >= 0.0f && p[k] <= 1.0f)) {
          std::printf("step %d env %lld: probs[%d] = %g\n", t, (long long)i, k, (double)p[k]);
          return 1;
        }
        sum += (double)p[k];
        c_k += (double)p[k];
        if (k < kA - 1 && c_k <= u) ++a;
      }
      if (std::fabs(sum - 1.0) > 1e-5 || !std::isfinite(hv[(size_t)i])) {
        std::printf("step %d env %lld: probs sum to %.9g, value %g\n", t, (long long)i, sum, (double)hv[(size_t)i]);
        return 1;
      }
      if (ha[(size_t)i] != a) {
        std::printf("step %d env %lld: action %d, the sampling rule gives %d (u = %.17g)\n", t, (long long)i,
                    (int)ha[(size_t)i], a, u);
        return 1;
      }
      counts[a]++;
      if (episode[(size_t)i] > max_episode) max_episode = episode[(size_t)i];
    }
  }
  wab_counters ctr;
  CHECK_WAB(wab_get_counters(h, &ctr, nullptr));
  if (ctr.handoff_timeouts || ctr.bad_actions || ctr.steps != (uint64_t)kB * kSteps) {
    std::printf("counters: handoff %llu bad %llu steps %llu\n", (unsigned long long)ctr.handoff_timeouts,
                (unsigned long long)ctr.bad_actions, (unsigned long long)ctr.steps);
    return 1;
  }
  if (max_episode < 1) {
    std::printf("no env reached a second episode in %d steps\n", kSteps);
    return 1;
  }
  CHECK_WAB(wab_policy_destroy(pol));
  CHECK_WAB(wab_destroy(h));
  for (void* p : {(void*)planes, (void*)scal, (void*)done, (void*)act, (void*)rew, (void*)feat, (void*)probs,
                  (void*)value, (void*)w1, (void*)b1, (void*)w2, (void*)b2, (void*)w3, (void*)b3, (void*)wa, (void*)ba,
                  (void*)wv, (void*)bv})
    CHECK_HIP(hipFree(p));
  std::printf("OK c_api_policy_demo: %lld envs x %d closed-loop steps, every action the sampling rule's function of "
              "its probs row and keyed draw (actions taken: %lld %lld %lld %lld %lld; episodes up to %u)\n",
              (long long)kB, kSteps, counts[0], counts[1], counts[2], counts[3], counts[4], max_episode);
  return 0;
}
