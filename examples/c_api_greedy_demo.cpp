// Evaluation through the C-ABI with no Python in the process (include/wab.h only,
// WAB_HAS_ACTION_RULE): B envs, the reference's 449-128-150-128-{5, 1} network with weights made
// up on the host, the greedy action rule set on the policy, then one wab_rollout_policy of T
// steps.  The demo checks on the host what a caller can check without the network: the rule
// round-trips through the getter, a bad rule is refused and leaves the stored one alone, and
// every action is the first maximum of its probs row.  With a dump file it writes the ten weight
// tensors (wab_policy_weights' order, float32), then actions [T][B] int8, probs [T][B][5], value
// [T][B], reward [T][B] float32 and done [T][B] u8, for a host that repeats the run.
// Prints one OK line, or the first difference and exits non-zero.
//   usage: c_api_greedy_demo [B T seed [dump-file]]
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

constexpr int kA = 5;

uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// a Linear layer's weights and bias, uniform in +-gain/sqrt(in) (gain 1: torch's default), kept
// on the host in `keep` and copied to the device
int make_linear(uint64_t* state, int out, int in, double gain, std::vector<std::vector<float>>* keep, float** w,
                float** b) {
  std::vector<float> hw((size_t)out * in), hb((size_t)out);
  const double bound = gain / std::sqrt((double)in);
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
  keep->push_back(hw);
  keep->push_back(hb);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 1 && argc != 4 && argc != 5) {
    std::fprintf(stderr, "usage: %s [B T seed [dump-file]]\n", argv[0]);
    return 2;
  }
  const int64_t B = argc > 1 ? std::atoll(argv[1]) : 256;
  const int T = argc > 1 ? std::atoi(argv[2]) : 8;
  const uint64_t seed = argc > 1 ? std::strtoull(argv[3], nullptr, 0) : 0x5EEDull;
  if (B < 1 || T < 1) {
    std::fprintf(stderr, "B and T must be >= 1\n");
    return 2;
  }

  wab_config c = {};  // default_game_options (wab_env.py:11-39), short episodes
  c.reward_for_being_killed = -1;
  c.reward_for_starving = -1;
  c.reward_for_finishing = 1;
  c.reward_for_eating = 0.1;
  c.lookout_only = 1;
  c.starting_role = 1;
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
  CHECK_WAB(wab_create(&c, B, seed, 0, 0, &h));
  const int F = wab_feature_dim(h);
  if (F != 449) {
    std::printf("wab_feature_dim: %d\n", F);
    return 1;
  }
  const size_t TB = (size_t)T * (size_t)B;
  uint8_t *planes = nullptr, *scal = nullptr, *scal_seq = nullptr, *done = nullptr;
  int8_t* act = nullptr;
  float *rew = nullptr, *feat = nullptr, *last = nullptr, *probs = nullptr, *value = nullptr;
  CHECK_HIP(hipMalloc(&planes, (size_t)B * 3 * 11 * 11));
  CHECK_HIP(hipMalloc(&scal, 3 * (size_t)B));
  CHECK_HIP(hipMalloc(&scal_seq, 3 * TB));
  CHECK_HIP(hipMalloc(&done, TB));
  CHECK_HIP(hipMalloc(&act, TB));
  CHECK_HIP(hipMalloc(&rew, 4 * TB));
  CHECK_HIP(hipMalloc(&feat, 4 * (size_t)B * F));
  CHECK_HIP(hipMalloc(&last, 4 * (size_t)B * F));
  CHECK_HIP(hipMalloc(&probs, 4 * TB * kA));
  CHECK_HIP(hipMalloc(&value, 4 * TB));
  const wab_obs obs = {planes, scal, scal + B, scal + 2 * B};
  const wab_obs seq = {nullptr, scal_seq, scal_seq + TB, scal_seq + 2 * TB};

  // the network; the action head four times torch's default, so that the argmax moves with the input
  wab_policy* pol = nullptr;
  const wab_policy_shape shape = {F, 128, 150, 128, kA};
  CHECK_WAB(wab_policy_create(&shape, 0, &pol));
  wab_policy_weights w = {};
  float *w1, *b1, *w2, *b2, *w3, *b3, *wa, *ba, *wv, *bv;
  std::vector<std::vector<float>> tensors;
  uint64_t state = seed;
  if (make_linear(&state, 128, F, 1.0, &tensors, &w1, &b1) || make_linear(&state, 150, 128, 3.0, &tensors, &w2, &b2) ||
      make_linear(&state, 128, 150, 1.0, &tensors, &w3, &b3) || make_linear(&state, kA, 128, 4.0, &tensors, &wa, &ba) ||
      make_linear(&state, 1, 128, 1.0, &tensors, &wv, &bv))
    return 1;
  w.w1 = w1; w.b1 = b1; w.w2 = w2; w.b2 = b2; w.w3 = w3; w.b3 = b3; w.wa = wa; w.ba = ba; w.wv = wv; w.bv = bv;
  CHECK_WAB(wab_policy_load(pol, &w, nullptr));

  // the rule: a fresh policy samples at temperature 1; greedy is stored; a bad rule changes nothing
  wab_action_rule rule = {-1, -1.0f};
  CHECK_WAB(wab_policy_get_action_rule(pol, &rule));
  if (rule.mode != WAB_ACT_SAMPLE || rule.temperature != 1.0f) {
    std::printf("a fresh policy's rule is {%d, %g}\n", rule.mode, (double)rule.temperature);
    return 1;
  }
  const wab_action_rule greedy = {WAB_ACT_GREEDY, 1.0f};
  CHECK_WAB(wab_policy_set_action_rule(pol, &greedy));
  const wab_action_rule bad_rules[] = {{2, 1.0f}, {WAB_ACT_SAMPLE, 0.0f}, {WAB_ACT_SAMPLE, -1.0f},
                                       {WAB_ACT_GREEDY, INFINITY}, {WAB_ACT_GREEDY, NAN}};
  for (const wab_action_rule& bad : bad_rules) {
    if (wab_policy_set_action_rule(pol, &bad) != WAB_E_INVALID) {
      std::printf("the rule {%d, %g} was not refused\n", bad.mode, (double)bad.temperature);
      return 1;
    }
  }
  CHECK_WAB(wab_policy_get_action_rule(pol, &rule));
  if (rule.mode != WAB_ACT_GREEDY || rule.temperature != 1.0f) {
    std::printf("after the refusals the rule is {%d, %g}\n", rule.mode, (double)rule.temperature);
    return 1;
  }

  CHECK_WAB(wab_reset(h, nullptr, &obs, nullptr));
  CHECK_WAB(wab_featurize(h, &obs, nullptr, feat, nullptr));
  CHECK_WAB(wab_rollout_policy(h, pol, feat, T, &seq, act, value, probs, rew, done, nullptr, last, 0.99, nullptr,
                               nullptr, nullptr));
  CHECK_HIP(hipDeviceSynchronize());

  std::vector<int8_t> ha(TB);
  std::vector<float> hp(TB * kA), hv(TB), hr(TB);
  std::vector<uint8_t> hd(TB);
  CHECK_HIP(hipMemcpy(ha.data(), act, TB, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hp.data(), probs, 4 * TB * kA, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hv.data(), value, 4 * TB, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hr.data(), rew, 4 * TB, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hd.data(), done, TB, hipMemcpyDeviceToHost));
  long long counts[kA] = {}, ends = 0;
  for (size_t i = 0; i < TB; ++i) {
    const float* p = &hp[i * kA];
    double sum = 0.0;
    int a = 0;
    float best = p[0];
    for (int k = 0; k < kA; ++k) {
      if (!(p[k] >= 0.0f && p[k] <= 1.0f)) {
        std::printf("row %zu: probs[%d] = %g\n", i, k, (double)p[k]);
        return 1;
      }
      sum += (double)p[k];
      if (k > 0 && p[k] > best) {
        best = p[k];
        a = k;
      }
    }
    if (std::fabs(sum - 1.0) > 1e-5 || !std::isfinite(hv[i])) {
      std::printf("row %zu: probs sum to %.9g, value %g\n", i, sum, (double)hv[i]);
      return 1;
    }
    if (ha[i] != a) {
      std::printf("row %zu: action %d, the first maximum of its probs is %d\n", i, (int)ha[i], a);
      return 1;
    }
    counts[a]++;
    ends += hd[i];
  }
  wab_counters ctr;
  CHECK_WAB(wab_get_counters(h, &ctr, nullptr));
  if (ctr.handoff_timeouts || ctr.bad_actions || ctr.steps != (uint64_t)TB) {
    std::printf("counters: handoff %llu bad %llu steps %llu\n", (unsigned long long)ctr.handoff_timeouts,
                (unsigned long long)ctr.bad_actions, (unsigned long long)ctr.steps);
    return 1;
  }
  if (argc > 4) {
    std::FILE* dump = std::fopen(argv[4], "wb");
    if (!dump) {
      std::fprintf(stderr, "cannot write %s\n", argv[4]);
      return 1;
    }
    for (const std::vector<float>& x : tensors) std::fwrite(x.data(), 4, x.size(), dump);
    std::fwrite(ha.data(), 1, ha.size(), dump);
    std::fwrite(hp.data(), 4, hp.size(), dump);
    std::fwrite(hv.data(), 4, hv.size(), dump);
    std::fwrite(hr.data(), 4, hr.size(), dump);
    std::fwrite(hd.data(), 1, hd.size(), dump);
    std::fclose(dump);
  }
  CHECK_WAB(wab_policy_destroy(pol));
  CHECK_WAB(wab_destroy(h));
  for (void* p : {(void*)planes, (void*)scal, (void*)scal_seq, (void*)done, (void*)act, (void*)rew, (void*)feat,
                  (void*)last, (void*)probs, (void*)value, (void*)w1, (void*)b1, (void*)w2, (void*)b2, (void*)w3,
                  (void*)b3, (void*)wa, (void*)ba, (void*)wv, (void*)bv})
    CHECK_HIP(hipFree(p));
  std::printf("OK c_api_greedy_demo: %lld envs x %d greedy steps in %s, every action the first maximum of its probs "
              "row (actions taken: %lld %lld %lld %lld %lld; %lld episodes ended)\n",
              (long long)B, T, ctr.rollout_launches ? "one launch" : "2 T launches", counts[0], counts[1], counts[2],
              counts[3], counts[4], ends);
  return 0;
}
