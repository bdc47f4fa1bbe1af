// Snapshots through the C-ABI with no Python in the process (include/wab.h:
// wab_snapshot_save / wab_snapshot_restore).
//   1. one handle of 128 envs: reset, 20 steps, save;
//   2. 30 more steps, every output kept on the host;
//   3. restore, the same 30 steps again: byte for byte the same outputs (a rewind);
//   4. the records copied to the host, the handle destroyed;
//   5. two handles of 64 envs (env_id_base 0 and 64), never reset, each restored from the host
//      copy (a resume in another handle, re-sharded);
//   6. the same 30 steps on both: their concatenated outputs equal step 2's.
// Prints one OK line, or the first difference and exits non-zero.
//   usage: c_api_snapshot_demo [seed]
#include <hip/hip_runtime_api.h>

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

constexpr int64_t kB = 128;
constexpr int kBefore = 20, kAfter = 30;
constexpr size_t kOB = 3 * 11 * 11;

// one handle with its device buffers
struct Env {
  wab_handle* h = nullptr;
  int64_t B = 0;
  uint8_t *planes = nullptr, *scal = nullptr, *done = nullptr;
  int8_t* act = nullptr;
  float* rew = nullptr;
  wab_obs obs() const { return wab_obs{planes, scal, scal + B, scal + 2 * B}; }
};

// what `T` steps of B envs gave, step-major: planes, scalars, reward, done
struct Trace {
  std::vector<uint8_t> planes, scal, done;
  std::vector<float> rew;
};

int8_t action_of(uint64_t seed, int t, int64_t env) {  // splitmix64 of (seed, step, global env id)
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)t * 1000003ull + (uint64_t)env + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (int8_t)((z ^ (z >> 31)) % 5);
}

int make_env(const wab_config& c, int64_t B, uint64_t seed, int64_t base, Env* e) {
  e->B = B;
  CHECK_WAB(wab_create(&c, B, seed, base, 0, &e->h));
  CHECK_HIP(hipMalloc(&e->planes, B * kOB));
  CHECK_HIP(hipMalloc(&e->scal, 3 * B));
  CHECK_HIP(hipMalloc(&e->done, B));
  CHECK_HIP(hipMalloc(&e->act, B));
  CHECK_HIP(hipMalloc(&e->rew, 4 * B));
  return 0;
}

int free_env(Env* e) {
  CHECK_WAB(wab_destroy(e->h));
  for (void* p : {(void*)e->planes, (void*)e->scal, (void*)e->done, (void*)e->act, (void*)e->rew})
    CHECK_HIP(hipFree(p));
  *e = Env();
  return 0;
}

// steps t0 .. t0 + T - 1 of envs with global ids [base, base + B); outputs into columns
// [col, col + B) of a trace of `width` envs per step (nullptr: not kept)
int run(Env* e, uint64_t seed, int64_t base, int t0, int T, Trace* tr, int64_t width, int64_t col) {
  const int64_t B = e->B;
  std::vector<int8_t> a((size_t)B);
  const wab_obs o = e->obs();
  for (int t = 0; t < T; ++t) {
    for (int64_t i = 0; i < B; ++i) a[(size_t)i] = action_of(seed, t0 + t, base + i);
    CHECK_HIP(hipMemcpy(e->act, a.data(), B, hipMemcpyHostToDevice));
    CHECK_WAB(wab_step(e->h, e->act, &o, e->rew, e->done, nullptr, nullptr));
    if (!tr) continue;
    const size_t row = (size_t)t * (size_t)width + (size_t)col;
    CHECK_HIP(hipMemcpy(tr->planes.data() + row * kOB, e->planes, B * kOB, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; ++k)
      CHECK_HIP(hipMemcpy(tr->scal.data() + ((size_t)t * 3 + k) * (size_t)width + (size_t)col, e->scal + k * B, B,
                          hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(tr->rew.data() + row, e->rew, 4 * B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(tr->done.data() + row, e->done, B, hipMemcpyDeviceToHost));
  }
  return 0;
}

Trace make_trace(int T, int64_t width) {
  Trace tr;
  tr.planes.resize((size_t)T * width * kOB);
  tr.scal.resize((size_t)T * 3 * width);
  tr.done.resize((size_t)T * width);
  tr.rew.resize((size_t)T * width);
  return tr;
}

// 0 when equal; else prints the first difference
int compare(const Trace& a, const Trace& b, const char* what) {
  const auto first_diff = [](const void* x, const void* y, size_t n) -> long long {
    const uint8_t* p = static_cast<const uint8_t*>(x);
    const uint8_t* q = static_cast<const uint8_t*>(y);
    for (size_t i = 0; i < n; ++i)
      if (p[i] != q[i]) return (long long)i;
    return -1;
  };
  long long d;
  if ((d = first_diff(a.planes.data(), b.planes.data(), a.planes.size())) >= 0) {
    std::printf("%s: planes differ first at step %lld env %lld byte %lld\n", what, d / (long long)(kB * kOB),
                d / (long long)kOB % (long long)kB, d % (long long)kOB);
    return 1;
  }
  if ((d = first_diff(a.scal.data(), b.scal.data(), a.scal.size())) >= 0) {
    std::printf("%s: obs scalars differ first at step %lld scalar %lld env %lld\n", what, d / (3 * kB),
                d / kB % 3, d % kB);
    return 1;
  }
  if ((d = first_diff(a.rew.data(), b.rew.data(), a.rew.size() * 4)) >= 0) {
    std::printf("%s: reward differs first at step %lld env %lld\n", what, d / 4 / kB, d / 4 % kB);
    return 1;
  }
  if ((d = first_diff(a.done.data(), b.done.data(), a.done.size())) >= 0) {
    std::printf("%s: done differs first at step %lld env %lld\n", what, d / kB, d % kB);
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 0) : 0x5EEDull;

  wab_config c = {};  // default_game_options (wab_env.py:11-39)
  c.reward_for_being_killed = -1;
  c.reward_for_starving = -1;
  c.reward_for_finishing = 1;
  c.reward_for_eating = 0.1;
  c.lookout_only = 1;
  c.starting_role = 1;
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

  const int R = wab_snapshot_bytes(&c);
  if (R <= 0 || R % 16) {
    std::printf("wab_snapshot_bytes: %d\n", R);
    return 1;
  }

  // 1. reset, 20 steps, save
  Env e;
  if (make_env(c, kB, seed, 0, &e)) return 1;
  wab_obs o = e.obs();
  CHECK_WAB(wab_reset(e.h, nullptr, &o, nullptr));
  if (run(&e, seed, 0, 0, kBefore, nullptr, kB, 0)) return 1;
  void* records = nullptr;
  CHECK_HIP(hipMalloc(&records, (size_t)kB * (size_t)R));
  wab_snapshot_info info;
  CHECK_WAB(wab_snapshot_save(e.h, 0, kB, records, &info, nullptr));
  if (info.count != kB || info.env_id_first != 0 || info.record_bytes != R || info.seed != seed ||
      info.config_hash != wab_snapshot_hash(&c)) {
    std::printf("wab_snapshot_save: unexpected info\n");
    return 1;
  }
  // 2. 30 steps, kept
  Trace first = make_trace(kAfter, kB);
  if (run(&e, seed, 0, kBefore, kAfter, &first, kB, 0)) return 1;
  // 3. rewind and replay
  CHECK_WAB(wab_snapshot_restore(e.h, &info, records, nullptr, nullptr));
  Trace again = make_trace(kAfter, kB);
  if (run(&e, seed, 0, kBefore, kAfter, &again, kB, 0)) return 1;
  if (compare(first, again, "rewind")) return 1;
  // 4. records to the host, the handle gone
  std::vector<uint8_t> host((size_t)kB * (size_t)R);
  CHECK_HIP(hipMemcpy(host.data(), records, host.size(), hipMemcpyDeviceToHost));
  CHECK_HIP(hipFree(records));
  if (free_env(&e)) return 1;
  // 5. + 6. two fresh handles of 64 envs, each restored from the host copy, the same 30 steps
  Trace shards = make_trace(kAfter, kB);
  unsigned long long dones = 0;
  for (int s = 0; s < 2; ++s) {
    const int64_t half = kB / 2, base = s * half;
    Env f;
    if (make_env(c, half, seed, base, &f)) return 1;
    void* dev = nullptr;  // the whole snapshot: the handle takes the records of its own ids
    CHECK_HIP(hipMalloc(&dev, host.size()));
    CHECK_HIP(hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice));
    CHECK_WAB(wab_snapshot_restore(f.h, &info, dev, nullptr, nullptr));
    if (run(&f, seed, base, kBefore, kAfter, &shards, kB, base)) return 1;
    wab_counters ctr;
    CHECK_WAB(wab_get_counters(f.h, &ctr, nullptr));
    if (ctr.handoff_timeouts || ctr.wolf_overflow || ctr.eaten_overflow || ctr.bad_actions) {
      std::printf("counters: handoff %llu wolf %llu eaten %llu bad %llu\n",
                  (unsigned long long)ctr.handoff_timeouts, (unsigned long long)ctr.wolf_overflow,
                  (unsigned long long)ctr.eaten_overflow, (unsigned long long)ctr.bad_actions);
      return 1;
    }
    CHECK_HIP(hipFree(dev));
    if (free_env(&f)) return 1;
  }
  if (compare(first, shards, "re-sharded resume")) return 1;
  for (uint8_t d : first.done) dones += d;
  std::printf("OK c_api_snapshot_demo: %lld envs, snapshot after %d steps (%d bytes per env), %d steps replayed "
              "after a rewind and in two fresh handles of %lld envs, byte for byte (%llu episodes ended)\n",
              (long long)kB, kBefore, R, kAfter, (long long)(kB / 2), dones);
  return 0;
}
