// Episode statistics and per-episode normalisation through the C-ABI with no Python in the
// process (include/wab.h: wab_episode_stats_update, wab_normalize_episode_returns).
// A hand-made [T][B] segment of the default options' rewards (0.1f, 1.1f, -0.9f, -1.0f, ...) and a
// sprinkling of dones goes through two wab_episode_stats_update calls, split at a step that an
// episode spans, with a handle of the default options (exact double rewards) and with h = NULL
// (rewards as given); then with capacity 0 and NULL record arrays; then the segment's discounted
// returns are normalised per episode.  Everything is compared with the same arithmetic done on
// the host in step order: double sums by their bits, the normalised values within one float32
// step.  Prints one OK line, or the first difference and exits non-zero.
//   usage: c_api_episodes_demo
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

constexpr int kT = 45, kSplit = 19;
constexpr int64_t kB = 150;

struct Episode {
  double ret;
  int32_t length, env, step;
};

uint64_t bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}
uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
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
  c.starting_role = 1;
  c.starting_role_random = 1;
  c.starting_food_random = 1;
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

// the reference step's double reward of a float32 device reward: 0 + r_x or 0 + r_eat + r_x for
// r_x in per turn, finishing, starving, killed (wab_env.py:299-340); other floats as given
double exact_reward(const wab_config& c, float f) {
  const double rx[4] = {c.reward_per_turn, c.reward_for_finishing, c.reward_for_starving,
                        c.reward_for_being_killed};
  for (double r : rx)
    for (int eat = 0; eat < 2; ++eat) {
      const double d = eat ? (0.0 + c.reward_for_eating) + r : 0.0 + r;
      if ((float)d == f) return d;
    }
  return (double)f;
}

// the host's walk: T steps of (ret += r, length += 1, close at done), episodes in (step, env) order
void host_walk(const wab_config& cfg, const std::vector<float>& rew, const std::vector<uint8_t>& done, int t0, int t1, bool exact,
               std::vector<double>& ret, std::vector<int64_t>& len, std::vector<Episode>& eps) {
  for (int t = t0; t < t1; ++t)
    for (int64_t b = 0; b < kB; ++b) {
      const float f = rew[(size_t)t * kB + b];
      ret[b] += exact ? exact_reward(cfg, f) : (double)f;
      len[b] += 1;
      if (done[(size_t)t * kB + b]) {
        eps.push_back({ret[b], (int32_t)len[b], (int32_t)b, t - t0});
        ret[b] = 0.0;
        len[b] = 0;
      }
    }
}

template <typename V>
int upload(V** dst, const std::vector<V>& src) {
  CHECK_HIP(hipMalloc(dst, src.size() * sizeof(V) + 8));
  CHECK_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(V), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

int main() {
  if (wab_abi_version() != WAB_ABI_VERSION) {
    std::fprintf(stderr, "library ABI %d, header %d\n", wab_abi_version(), WAB_ABI_VERSION);
    return 1;
  }
  // the segment: rewards from the env's own set and two arbitrary floats, dones about one in nine
  // with a burst (a whole step done) and env 7 never done
  std::vector<float> rew((size_t)kT * kB);
  std::vector<uint8_t> done((size_t)kT * kB);
  const float vals[8] = {0.0f, 0.1f, 1.0f, 1.1f, -0.9f, -1.0f, 0.25f, 0.3f};
  uint64_t z = 0x5EED;
  for (size_t i = 0; i < rew.size(); ++i) {
    z = z * 6364136223846793005ull + 1442695040888963407ull;
    rew[i] = vals[(z >> 33) % 8];
    const int t = (int)(i / kB), b = (int)(i % kB);
    done[i] = (uint8_t)(((z >> 40) % 9 == 0 || t == 30) && b != 7);
  }
  done[(size_t)(kSplit - 1) * kB + 3] = 0;  // env 3's episode spans the split
  done[(size_t)kSplit * kB + 3] = 0;

  wab_config cfg = default_config();
  wab_handle* h = nullptr;
  CHECK_WAB(wab_create(&cfg, 1, 1, 0, 0, &h));

  float *d_rew = nullptr, *d_ret32 = nullptr, *d_norm = nullptr;
  uint8_t* d_done = nullptr;
  if (upload(&d_rew, rew) || upload(&d_done, done)) return 1;
  const int64_t cap = (int64_t)kT * kB;
  double *d_ret = nullptr, *d_epr = nullptr;
  int64_t *d_len = nullptr, *d_count = nullptr;
  int32_t *d_epl = nullptr, *d_epe = nullptr, *d_eps = nullptr;
  void* d_ws = nullptr;
  const int64_t ws = wab_episode_stats_workspace(kT, kB);
  if (ws < 0) {
    std::fprintf(stderr, "wab_episode_stats_workspace: %s\n", wab_last_error());
    return 1;
  }
  CHECK_HIP(hipMalloc(&d_ws, (size_t)ws + 8));
  CHECK_HIP(hipMalloc(&d_ret, kB * 8));
  CHECK_HIP(hipMalloc(&d_len, kB * 8));
  CHECK_HIP(hipMalloc(&d_count, 16));
  CHECK_HIP(hipMalloc(&d_epr, cap * 8));
  CHECK_HIP(hipMalloc(&d_epl, cap * 4));
  CHECK_HIP(hipMalloc(&d_epe, cap * 4));
  CHECK_HIP(hipMalloc(&d_eps, cap * 4));

  bool some_sum_differs = false;
  std::vector<uint64_t> exact_bits;
  for (int exact = 1; exact >= 0; --exact) {
    CHECK_HIP(hipMemset(d_ret, 0, kB * 8));
    CHECK_HIP(hipMemset(d_len, 0, kB * 8));
    std::vector<double> ret(kB, 0.0);
    std::vector<int64_t> len(kB, 0);
    size_t n_all = 0;
    const int cuts[3] = {0, kSplit, kT};
    for (int part = 0; part < 2; ++part) {
      const int t0 = cuts[part], t1 = cuts[part + 1];
      std::vector<Episode> want;
      host_walk(cfg, rew, done, t0, t1, exact != 0, ret, len, want);
      CHECK_WAB(wab_episode_stats_update(exact ? h : nullptr, d_rew + (size_t)t0 * kB, d_done + (size_t)t0 * kB,
                                         t1 - t0, kB, d_ret, d_len, d_epr, d_epl, d_epe, d_eps, cap, d_count, d_ws,
                                         nullptr));
      int64_t count[2];
      CHECK_HIP(hipMemcpy(count, d_count, 16, hipMemcpyDeviceToHost));
      if (count[0] != (int64_t)want.size() || count[1] != count[0]) {
        std::fprintf(stderr, "part %d: count {%lld, %lld}, expected %zu\n", part, (long long)count[0],
                     (long long)count[1], want.size());
        return 1;
      }
      std::vector<double> epr(want.size());
      std::vector<int32_t> epl(want.size()), epe(want.size()), eps(want.size());
      CHECK_HIP(hipMemcpy(epr.data(), d_epr, want.size() * 8, hipMemcpyDeviceToHost));
      CHECK_HIP(hipMemcpy(epl.data(), d_epl, want.size() * 4, hipMemcpyDeviceToHost));
      CHECK_HIP(hipMemcpy(epe.data(), d_epe, want.size() * 4, hipMemcpyDeviceToHost));
      CHECK_HIP(hipMemcpy(eps.data(), d_eps, want.size() * 4, hipMemcpyDeviceToHost));
      for (size_t k = 0; k < want.size(); ++k) {
        if (bits(epr[k]) != bits(want[k].ret) || epl[k] != want[k].length || epe[k] != want[k].env ||
            eps[k] != want[k].step) {
          std::fprintf(stderr, "part %d episode %zu: (%.17g, %d, %d, %d), expected (%.17g, %d, %d, %d)\n", part, k,
                       epr[k], epl[k], epe[k], eps[k], want[k].ret, want[k].length, want[k].env, want[k].step);
          return 1;
        }
        if (exact) exact_bits.push_back(bits(epr[k]));
        else if (n_all + k < exact_bits.size() && exact_bits[n_all + k] != bits(epr[k])) some_sum_differs = true;
      }
      n_all += want.size();
      if (part == 0 && len[3] < 1) {
        std::fprintf(stderr, "env 3's episode does not span the split\n");
        return 1;
      }
    }
    std::vector<double> g_ret(kB);
    std::vector<int64_t> g_len(kB);
    CHECK_HIP(hipMemcpy(g_ret.data(), d_ret, kB * 8, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(g_len.data(), d_len, kB * 8, hipMemcpyDeviceToHost));
    for (int64_t b = 0; b < kB; ++b)
      if (bits(g_ret[b]) != bits(ret[b]) || g_len[b] != len[b]) {
        std::fprintf(stderr, "running state of env %lld: (%.17g, %lld), expected (%.17g, %lld)\n", (long long)b,
                     g_ret[b], (long long)g_len[b], ret[b], (long long)len[b]);
        return 1;
      }
    if (g_len[7] != kT) {
      std::fprintf(stderr, "env 7 should still be in its first episode\n");
      return 1;
    }
  }
  if (!some_sum_differs) {
    std::fprintf(stderr, "no episode sum differs between the exact and the float32 rewards\n");
    return 1;
  }
  // count only: NULL record arrays, capacity 0
  {
    CHECK_HIP(hipMemset(d_ret, 0, kB * 8));
    CHECK_HIP(hipMemset(d_len, 0, kB * 8));
    CHECK_WAB(wab_episode_stats_update(h, d_rew, d_done, kT, kB, d_ret, d_len, nullptr, nullptr, nullptr, nullptr,
                                       0, d_count, d_ws, nullptr));
    int64_t count[2], dones = 0;
    CHECK_HIP(hipMemcpy(count, d_count, 16, hipMemcpyDeviceToHost));
    for (uint8_t d : done) dones += d;
    if (count[0] != dones || count[1] != 0) {
      std::fprintf(stderr, "count only: {%lld, %lld}, expected {%lld, 0}\n", (long long)count[0],
                   (long long)count[1], (long long)dones);
      return 1;
    }
  }
  // discounted returns of the segment (exact rewards), then their per-episode normalisation
  CHECK_HIP(hipMalloc(&d_ret32, rew.size() * 4));
  CHECK_HIP(hipMalloc(&d_norm, rew.size() * 4));
  CHECK_WAB(wab_discounted_returns_exact(h, d_rew, d_done, kT, kB, 0.99, nullptr, d_ret32, nullptr));
  const double eps = 1.1920928955078125e-07;
  CHECK_WAB(wab_normalize_episode_returns(d_ret32, d_done, kT, kB, eps, d_norm, nullptr));
  std::vector<float> x(rew.size()), got(rew.size());
  CHECK_HIP(hipMemcpy(x.data(), d_ret32, x.size() * 4, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(got.data(), d_norm, got.size() * 4, hipMemcpyDeviceToHost));
  size_t nans = 0;
  for (int64_t b = 0; b < kB; ++b) {
    int s = 0;
    while (s < kT) {
      int e = s;
      while (e < kT - 1 && !done[(size_t)e * kB + b]) ++e;
      const int n = e - s + 1;
      double sum = 0.0, ss = 0.0;
      for (int t = s; t <= e; ++t) sum += (double)x[(size_t)t * kB + b];
      const double mean = sum / (double)n;
      for (int t = s; t <= e; ++t) {
        const double dev = (double)x[(size_t)t * kB + b] - mean;
        ss += dev * dev;
      }
      const double denom = std::sqrt(ss / (double)(n - 1)) + eps;
      for (int t = s; t <= e; ++t) {
        const float want = (float)(((double)x[(size_t)t * kB + b] - mean) / denom);
        const float g = got[(size_t)t * kB + b];
        const bool ok = std::isnan(want) ? std::isnan(g)
                                         : (g == want || g == std::nextafterf(want, INFINITY) ||
                                            g == std::nextafterf(want, -INFINITY));
        if (!ok) {
          std::fprintf(stderr, "normalised [%d][%lld] = %.9g (%08x), expected %.9g (%08x)\n", t, (long long)b, g,
                       bits(g), want, bits(want));
          return 1;
        }
        nans += std::isnan(want);
      }
      s = e + 1;
    }
  }
  if (nans == 0) {
    std::fprintf(stderr, "the segment has no one-step episode\n");
    return 1;
  }
  CHECK_WAB(wab_destroy(h));
  std::printf("OK: %d x %lld segment in two calls, episodes and running state equal the host's bit for bit "
              "(exact and float32 rewards), count-only call, per-episode normalisation (%zu NaN of one-step "
              "episodes)\n", kT, (long long)kB, nans);
  return 0;
}
