// Advantages and their whole-batch normalisation through the C-ABI with no Python in the process
// (include/wab.h: wab_gae, wab_whiten).  A hand-made [T][B] segment (the default options'
// rewards, arbitrary floats and -0.0; dones of the byte values 1, 0x80 and 0xFF; values with a
// -0.0) goes through wab_gae with a handle of the default options (exact double rewards) and with
// h = NULL (rewards as given), with and without last_value, and with one output only.  Every
// result is compared with the contract's arithmetic done on the host, bit for bit.  The
// advantages are then whitened, in place and out of place, and compared with the host's sums
// within one float32 step.  Prints one OK line, or the first difference and exits non-zero.
//   usage: c_api_gae_demo
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

constexpr int kT = 37;
constexpr int64_t kB = 300;
constexpr double kGamma = 0.99, kLambda = 0.95;

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

// the contract of wab_gae (include/wab.h) on the host
void host_gae(const wab_config* cfg, const std::vector<float>& rew, const std::vector<uint8_t>& done,
              const std::vector<float>& val, const std::vector<float>* last, std::vector<float>& adv,
              std::vector<float>& tgt) {
  const double gl = kGamma * kLambda;
  for (int64_t b = 0; b < kB; ++b) {
    double A = 0.0, vnext = last ? (double)(*last)[b] : 0.0;
    for (int t = kT - 1; t >= 0; --t) {
      const size_t i = (size_t)t * kB + b;
      const double v = (double)val[i];
      const double r = cfg ? exact_reward(*cfg, rew[i]) : (double)rew[i];
      const bool d = done[i] != 0;
      const double delta = (r + (d ? 0.0 : kGamma * vnext)) - v;
      A = delta + (d ? 0.0 : gl * A);
      adv[i] = (float)A;
      tgt[i] = (float)(A + v);
      vnext = v;
    }
  }
}

template <typename V>
int upload(V** dst, const std::vector<V>& src) {
  CHECK_HIP(hipMalloc(dst, src.size() * sizeof(V) + 8));
  CHECK_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(V), hipMemcpyHostToDevice));
  return 0;
}

int compare(const char* what, const float* d_got, const std::vector<float>& want) {
  std::vector<float> got(want.size());
  CHECK_HIP(hipMemcpy(got.data(), d_got, got.size() * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < want.size(); ++i)
    if (bits(got[i]) != bits(want[i])) {
      std::fprintf(stderr, "%s [%zu][%zu] = %.9g (%08x), expected %.9g (%08x)\n", what, i / kB, i % kB, got[i],
                   bits(got[i]), want[i], bits(want[i]));
      return 1;
    }
  return 0;
}

}  // namespace

int main() {
  if (wab_abi_version() != WAB_ABI_VERSION) {
    std::fprintf(stderr, "library ABI %d, header %d\n", wab_abi_version(), WAB_ABI_VERSION);
    return 1;
  }
  const size_t n = (size_t)kT * kB;
  std::vector<float> rew(n), val(n), last(kB);
  std::vector<uint8_t> done(n);
  const float vals[8] = {0.0f, 0.1f, 1.0f, 1.1f, -0.9f, -1.0f, 0.25f, -0.0f};
  const uint8_t done_bytes[3] = {1, 0x80, 0xFF};
  uint64_t z = 0x6AE;
  for (size_t i = 0; i < n; ++i) {
    z = z * 6364136223846793005ull + 1442695040888963407ull;
    rew[i] = vals[(z >> 33) % 8];
    const int t = (int)(i / kB), b = (int)(i % kB);
    done[i] = ((z >> 40) % 9 == 0 && b != 7) || b == 8 ? done_bytes[(t + b) % 3] : 0;  // env 7 never, env 8 always
    val[i] = (float)((double)((z >> 8) % 2001) / 250.0 - 4.0);
    if ((z >> 50) % 31 == 0) val[i] = -0.0f;
  }
  for (int64_t b = 0; b < kB; ++b) last[b] = (float)((double)((b * 37) % 101) / 25.0 - 2.0);

  wab_config cfg = default_config();
  wab_handle* h = nullptr;
  CHECK_WAB(wab_create(&cfg, 1, 1, 0, 0, &h));

  float *d_rew = nullptr, *d_val = nullptr, *d_last = nullptr, *d_adv = nullptr, *d_tgt = nullptr, *d_white = nullptr;
  uint8_t* d_done = nullptr;
  if (upload(&d_rew, rew) || upload(&d_val, val) || upload(&d_last, last) || upload(&d_done, done)) return 1;
  CHECK_HIP(hipMalloc(&d_adv, n * 4));
  CHECK_HIP(hipMalloc(&d_tgt, n * 4));
  CHECK_HIP(hipMalloc(&d_white, n * 4));

  std::vector<float> adv(n), tgt(n), adv_exact(n);
  size_t exact_differs = 0;
  for (int exact = 1; exact >= 0; --exact)
    for (int with_last = 1; with_last >= 0; --with_last) {
      host_gae(exact ? &cfg : nullptr, rew, done, val, with_last ? &last : nullptr, adv, tgt);
      CHECK_HIP(hipMemset(d_adv, 0xFF, n * 4));
      CHECK_HIP(hipMemset(d_tgt, 0xFF, n * 4));
      CHECK_WAB(wab_gae(exact ? h : nullptr, d_rew, d_done, d_val, with_last ? d_last : nullptr, kT, kB, kGamma,
                        kLambda, d_adv, d_tgt, nullptr));
      if (compare("advantage", d_adv, adv) || compare("target", d_tgt, tgt)) return 1;
      if (exact && with_last) adv_exact = adv;
      if (!exact && with_last)
        for (size_t i = 0; i < n; ++i) exact_differs += bits(adv[i]) != bits(adv_exact[i]);
    }
  if (exact_differs == 0) {
    std::fprintf(stderr, "no advantage differs between the exact and the float32 rewards\n");
    return 1;
  }
  // one output only
  host_gae(&cfg, rew, done, val, &last, adv, tgt);
  CHECK_HIP(hipMemset(d_adv, 0xFF, n * 4));
  CHECK_HIP(hipMemset(d_tgt, 0xFF, n * 4));
  CHECK_WAB(wab_gae(h, d_rew, d_done, d_val, d_last, kT, kB, kGamma, kLambda, nullptr, d_tgt, nullptr));
  if (compare("target alone", d_tgt, tgt)) return 1;
  CHECK_WAB(wab_gae(h, d_rew, d_done, d_val, d_last, kT, kB, kGamma, kLambda, d_adv, nullptr, nullptr));
  if (compare("advantage alone", d_adv, adv)) return 1;
  // refusals: both outputs NULL, an output over an input
  if (wab_gae(h, d_rew, d_done, d_val, d_last, kT, kB, kGamma, kLambda, nullptr, nullptr, nullptr) != WAB_E_INVALID ||
      wab_gae(h, d_rew, d_done, d_val, d_last, kT, kB, kGamma, kLambda, d_val, nullptr, nullptr) != WAB_E_INVALID) {
    std::fprintf(stderr, "wab_gae accepted NULL outputs or an output over value\n");
    return 1;
  }

  // whitening of the advantages: out of place, then in place
  const int64_t ws = wab_whiten_workspace((int64_t)n);
  if (ws < 0) {
    std::fprintf(stderr, "wab_whiten_workspace: %s\n", wab_last_error());
    return 1;
  }
  void* d_ws = nullptr;
  CHECK_HIP(hipMalloc(&d_ws, (size_t)ws + 8));
  const double eps = 1.1920928955078125e-07;
  CHECK_WAB(wab_whiten(d_adv, (int64_t)n, eps, d_white, d_ws, nullptr));
  CHECK_WAB(wab_whiten(d_adv, (int64_t)n, eps, d_adv, d_ws, nullptr));
  std::vector<float> got(n), got_in_place(n);
  CHECK_HIP(hipMemcpy(got.data(), d_white, n * 4, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(got_in_place.data(), d_adv, n * 4, hipMemcpyDeviceToHost));
  {
    double sum = 0.0, ss = 0.0;
    for (size_t i = 0; i < n; ++i) sum += (double)adv[i];
    const double mean = sum / (double)n;
    for (size_t i = 0; i < n; ++i) ss += ((double)adv[i] - mean) * ((double)adv[i] - mean);
    const double denom = std::sqrt(ss / (double)(n - 1)) + eps;
    for (size_t i = 0; i < n; ++i) {
      const float want = (float)(((double)adv[i] - mean) / denom);
      const float g = got[i];
      // (the device adds in another order: the sums differ by parts in 10^13, the quotient by
      // at most one float32 step where it lies on a rounding boundary)
      if (!(g == want || g == std::nextafterf(want, INFINITY) || g == std::nextafterf(want, -INFINITY))) {
        std::fprintf(stderr, "whitened [%zu] = %.9g (%08x), expected %.9g (%08x)\n", i, g, bits(g), want, bits(want));
        return 1;
      }
      if (bits(g) != bits(got_in_place[i])) {
        std::fprintf(stderr, "whitened in place [%zu] = %08x, out of place %08x\n", i, bits(got_in_place[i]), bits(g));
        return 1;
      }
    }
  }
  CHECK_WAB(wab_destroy(h));
  std::printf("OK: %d x %lld segment, advantages and targets equal the host's contract bit for bit (exact and "
              "float32 rewards, %zu advantages differ between them; with and without last_value; one output "
              "alone), refusals, whitening in and out of place\n", kT, (long long)kB, exact_differs);
  return 0;
}
