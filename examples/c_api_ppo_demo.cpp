// PPO's clipped loss through the C-ABI with no Python in the process (include/wab.h:
// wab_policy_evaluate, wab_policy_grad_ppo): c_api_grad_demo's 17-33-33-33-{5, 1} network and 200
// rows made up on the host by the same formulas.
//   1. wab_policy_evaluate gives old_logp (and the values) of the rows;
//   2. wab_policy_grad_ppo with that old_logp: every ratio is exactly 1, so every gradient must
//      equal wab_policy_grad's with weight = advantage bit for bit, and ppo_out {0, 0, 0, 200}
//      (the demo checks both itself);
//   3. a second call with old_logp shifted by a fixed pattern and the value loss clipped around
//      values shifted likewise: prints one line per gradient tensor ("sum <name> <sum>"), the four
//      losses, ppo_out and one OK line; with a path argument the ten tensors, loss_out[4],
//      ppo_out[4], old_logp[200], old_value[200] and ratio[200] of that call are written there as
//      raw float32 (tests/test_gpu_ppo_capi.py compares them with the numeric contract).
//   usage: c_api_ppo_demo [dump-file]
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

constexpr int64_t kN = 200;
constexpr int kF = 17, kH = 33, kA = 5;
const int kOut[5] = {kH, kH, kH, kA, 1}, kIn[5] = {kF, kH, kH, kH, kH};
const char* const kNames[5] = {"affine1", "affine2", "affine3", "action_head", "value_head"};

// multiples of 1/16 and 1/8: exact in bf16
float weight_of(int layer, int n, int k) { return (float)((n * 5 + k * 3 + layer * 7) % 11 - 5) / 16.0f; }
float bias_of(int layer, int n) { return (float)((n * 3 + layer) % 7 - 3) / 8.0f; }
float feature_of(int64_t i, int k) { return (float)((i * 7 + k * 5) % 9) / 8.0f; }
// the second call's shifts: old_logp = logp + {-0.5, -0.25, 0, 0.25, 0.5}, old_value = value + {-0.6, -0.2, 0.2, 0.6}
float logp_shift(int64_t i) { return (float)(i % 5 - 2) * 0.25f; }
float value_shift(int64_t i) { return ((float)(i % 4) - 1.5f) * 0.4f; }

template <typename T>
int to_device(const std::vector<T>& h, T** d) {
  CHECK_HIP(hipMalloc(d, h.size() * sizeof(T)));
  CHECK_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (wab_abi_version() != WAB_ABI_VERSION) {
    std::fprintf(stderr, "library ABI %d, header %d\n", wab_abi_version(), WAB_ABI_VERSION);
    return 1;
  }
  wab_policy_shape shape = {kF, kH, kH, kH, kA};
  wab_policy* pol = nullptr;
  CHECK_WAB(wab_policy_create(&shape, 0, &pol));

  float *dw[5], *db[5], *gw[5], *gb[5], *rw[5], *rb[5];  // weights, the PPO call's gradients, wab_policy_grad's
  size_t nw[5], nb[5];
  for (int l = 0; l < 5; ++l) {
    std::vector<float> w((size_t)kOut[l] * kIn[l]), b((size_t)kOut[l]);
    for (int n = 0; n < kOut[l]; ++n) {
      b[(size_t)n] = bias_of(l, n);
      for (int k = 0; k < kIn[l]; ++k) w[(size_t)n * kIn[l] + k] = weight_of(l, n, k);
    }
    nw[l] = w.size();
    nb[l] = b.size();
    if (to_device(w, &dw[l]) || to_device(b, &db[l])) return 1;
    CHECK_HIP(hipMalloc(&gw[l], w.size() * 4));
    CHECK_HIP(hipMalloc(&gb[l], b.size() * 4));
    CHECK_HIP(hipMalloc(&rw[l], w.size() * 4));
    CHECK_HIP(hipMalloc(&rb[l], b.size() * 4));
  }
  const wab_policy_weights weights = {dw[0], db[0], dw[1], db[1], dw[2], db[2], dw[3], db[3], dw[4], db[4]};
  const wab_policy_weights grads = {gw[0], gb[0], gw[1], gb[1], gw[2], gb[2], gw[3], gb[3], gw[4], gb[4]};
  const wab_policy_weights a2c = {rw[0], rb[0], rw[1], rb[1], rw[2], rb[2], rw[3], rb[3], rw[4], rb[4]};

  std::vector<float> hx((size_t)kN * kF), hadv((size_t)kN), htgt((size_t)kN);
  std::vector<int8_t> hact((size_t)kN);
  for (int64_t i = 0; i < kN; ++i) {
    for (int k = 0; k < kF; ++k) hx[(size_t)i * kF + k] = feature_of(i, k);
    hact[(size_t)i] = (int8_t)(i % kA);
    hadv[(size_t)i] = (float)(i % 7 - 3) / 2.0f;
    htgt[(size_t)i] = (float)(i % 5 - 2) / 2.0f;
  }
  float *x, *adv, *tgt, *sums, *old_logp, *old_value, *ratio;
  int8_t* act;
  if (to_device(hx, &x) || to_device(hadv, &adv) || to_device(htgt, &tgt) || to_device(hact, &act)) return 1;
  CHECK_HIP(hipMalloc(&sums, 32));  // loss_out[4], ppo_out[4]
  CHECK_HIP(hipMalloc(&old_logp, kN * 4));
  CHECK_HIP(hipMalloc(&old_value, kN * 4));
  CHECK_HIP(hipMalloc(&ratio, kN * 4));

  wab_policy_loss cfg = {};
  cfg.value_coef = 0.5f;
  cfg.entropy_coef = 0.01f;
  cfg.value_loss = WAB_VALUE_LOSS_SMOOTH_L1;
  cfg.scale = 1.0f;
  cfg.chunk_rows = 128;  // two chunks
  wab_ppo_config ppo = {0.2f, 0.0f};
  const size_t ws_bytes = wab_policy_grad_workspace(pol, kN, cfg.chunk_rows);
  if (ws_bytes == 0) {
    std::fprintf(stderr, "wab_policy_grad_workspace: %s\n", wab_last_error());
    return 1;
  }
  void* ws = nullptr;
  CHECK_HIP(hipMalloc(&ws, ws_bytes));
  if (wab_policy_evaluate(pol, x, act, kN, old_logp, old_value, nullptr, ws, ws_bytes, nullptr) != WAB_E_STATE) {
    std::printf("wab_policy_evaluate before wab_policy_load was not refused\n");
    return 1;
  }
  CHECK_WAB(wab_policy_load(pol, &weights, nullptr));

  // 1. old_logp and the values, through a workspace of the 256 bytes evaluate needs
  CHECK_WAB(wab_policy_evaluate(pol, x, act, kN, old_logp, old_value, nullptr, ws, 256, nullptr));
  uint64_t bad = 1;
  CHECK_WAB(wab_policy_grad_bad_actions(pol, ws, nullptr, &bad));

  // 2. ratio 1: wab_policy_grad's gradients bit for bit, nothing clipped
  ppo.clip = 2.0f;
  if (wab_policy_grad_ppo(pol, x, act, adv, tgt, old_logp, nullptr, kN, &cfg, &ppo, &grads, sums, sums + 4, nullptr,
                          nullptr, nullptr, ratio, ws, ws_bytes, nullptr) != WAB_E_INVALID) {
    std::printf("clip = 2 was not refused\n");
    return 1;
  }
  ppo.clip = 0.2f;
  CHECK_WAB(wab_policy_grad_ppo(pol, x, act, adv, tgt, old_logp, nullptr, kN, &cfg, &ppo, &grads, sums, sums + 4,
                                nullptr, nullptr, nullptr, ratio, ws, ws_bytes, nullptr));
  float hs[8];
  CHECK_HIP(hipMemcpy(hs, sums, 32, hipMemcpyDeviceToHost));
  if (hs[4] != 0.0f || hs[5] != 0.0f || hs[6] != 0.0f || hs[7] != (float)kN) {
    std::printf("ratio 1: ppo_out = {%g, %g, %g, %g}, not {0, 0, 0, %lld}\n", (double)hs[4], (double)hs[5],
                (double)hs[6], (double)hs[7], (long long)kN);
    return 1;
  }
  CHECK_WAB(wab_policy_grad(pol, x, act, adv, tgt, kN, &cfg, &a2c, nullptr, nullptr, nullptr, nullptr, ws, ws_bytes,
                            nullptr));
  size_t compared = 0;
  for (int l = 0; l < 5; ++l)
    for (int part = 0; part < 2; ++part) {
      const size_t n = part == 0 ? nw[l] : nb[l];
      std::vector<float> g(n), r(n);
      CHECK_HIP(hipMemcpy(g.data(), part == 0 ? gw[l] : gb[l], n * 4, hipMemcpyDeviceToHost));
      CHECK_HIP(hipMemcpy(r.data(), part == 0 ? rw[l] : rb[l], n * 4, hipMemcpyDeviceToHost));
      if (std::memcmp(g.data(), r.data(), n * 4) != 0) {
        std::printf("ratio 1: %s.%s differs from wab_policy_grad's\n", kNames[l], part == 0 ? "weight" : "bias");
        return 1;
      }
      compared += n;
    }

  // 3. shifted old_logp, the value loss clipped around shifted values
  std::vector<float> holp((size_t)kN), hov((size_t)kN), hratio((size_t)kN);
  CHECK_HIP(hipMemcpy(holp.data(), old_logp, holp.size() * 4, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hov.data(), old_value, hov.size() * 4, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < kN; ++i) {
    holp[(size_t)i] += logp_shift(i);
    hov[(size_t)i] += value_shift(i);
  }
  CHECK_HIP(hipMemcpy(old_logp, holp.data(), holp.size() * 4, hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(old_value, hov.data(), hov.size() * 4, hipMemcpyHostToDevice));
  ppo.value_clip = 0.25f;
  if (wab_policy_grad_ppo(pol, x, act, adv, tgt, old_logp, nullptr, kN, &cfg, &ppo, &grads, sums, sums + 4, nullptr,
                          nullptr, nullptr, ratio, ws, ws_bytes, nullptr) != WAB_E_INVALID) {
    std::printf("value_clip > 0 without old_value was not refused\n");
    return 1;
  }
  CHECK_WAB(wab_policy_grad_ppo(pol, x, act, adv, tgt, old_logp, old_value, kN, &cfg, &ppo, &grads, sums, sums + 4,
                                nullptr, nullptr, nullptr, ratio, ws, ws_bytes, nullptr));
  CHECK_WAB(wab_policy_grad_bad_actions(pol, ws, nullptr, &bad));

  std::FILE* dump = argc > 1 ? std::fopen(argv[1], "wb") : nullptr;
  if (argc > 1 && !dump) {
    std::fprintf(stderr, "cannot write %s\n", argv[1]);
    return 1;
  }
  for (int l = 0; l < 5; ++l)
    for (int part = 0; part < 2; ++part) {
      std::vector<float> g(part == 0 ? nw[l] : nb[l]);
      CHECK_HIP(hipMemcpy(g.data(), part == 0 ? gw[l] : gb[l], g.size() * 4, hipMemcpyDeviceToHost));
      double sum = 0.0;
      for (float v : g) {
        if (!std::isfinite(v)) {
          std::printf("%s.%s has a non-finite entry\n", kNames[l], part == 0 ? "weight" : "bias");
          return 1;
        }
        sum += (double)v;
      }
      std::printf("sum %s.%s %.17g\n", kNames[l], part == 0 ? "weight" : "bias", sum);
      if (dump) std::fwrite(g.data(), 4, g.size(), dump);
    }
  CHECK_HIP(hipMemcpy(hs, sums, 32, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hratio.data(), ratio, hratio.size() * 4, hipMemcpyDeviceToHost));
  std::printf("loss %.9g %.9g %.9g %.9g\n", (double)hs[0], (double)hs[1], (double)hs[2], (double)hs[3]);
  std::printf("ppo %.9g %.9g %.9g %.9g\n", (double)hs[4], (double)hs[5], (double)hs[6], (double)hs[7]);
  if (dump) {
    std::fwrite(hs, 4, 8, dump);
    std::fwrite(holp.data(), 4, holp.size(), dump);
    std::fwrite(hov.data(), 4, hov.size(), dump);
    std::fwrite(hratio.data(), 4, hratio.size(), dump);
    std::fclose(dump);
  }

  CHECK_WAB(wab_policy_destroy(pol));
  for (int l = 0; l < 5; ++l)
    for (void* p : {(void*)dw[l], (void*)db[l], (void*)gw[l], (void*)gb[l], (void*)rw[l], (void*)rb[l]})
      CHECK_HIP(hipFree(p));
  for (void* p : {(void*)x, (void*)adv, (void*)tgt, (void*)act, (void*)sums, (void*)old_logp, (void*)old_value,
                  (void*)ratio, ws})
    CHECK_HIP(hipFree(p));
  std::printf("OK c_api_ppo_demo: %lld rows in two chunks, ratio 1 gave wab_policy_grad's %zu gradient entries "
              "bit for bit\n", (long long)kN, compared);
  return 0;
}
