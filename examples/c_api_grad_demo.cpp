// The actor-critic loss and its parameter gradients through the C-ABI with no Python in the
// process (include/wab.h: wab_policy_grad): a 17-33-33-33-{5, 1} network and 200 rows made up on
// the host by the formulas below (tests/test_gpu_policy_grad_capi.py makes the same ones and
// compares with the numeric contract).
// The demo's own check needs no network on the host: with one live row (every other row has
// weight 0 and its own value as target, so it contributes exactly 0), the first layer's weight
// gradient must be, bit for bit, the outer product of its bias gradient and the row's features:
// each entry is one bf16 x bf16 product, exact in float32.
// Prints one line per gradient tensor ("sum <name> <sum of its entries>"), the four losses and
// one OK line; with a path argument the ten tensors and the losses are also written there as
// raw float32.
//   usage: c_api_grad_demo [dump-file]
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
constexpr int kF = 17, kH = 33, kA = 5, kLive = 131;
const int kOut[5] = {kH, kH, kH, kA, 1}, kIn[5] = {kF, kH, kH, kH, kH};
const char* const kNames[5] = {"affine1", "affine2", "affine3", "action_head", "value_head"};

// multiples of 1/16 and 1/8: exact in bf16
float weight_of(int layer, int n, int k) { return (float)((n * 5 + k * 3 + layer * 7) % 11 - 5) / 16.0f; }
float bias_of(int layer, int n) { return (float)((n * 3 + layer) % 7 - 3) / 8.0f; }
float feature_of(int64_t i, int k) { return (float)((i * 7 + k * 5) % 9) / 8.0f; }

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

  float *dw[5], *db[5], *gw[5], *gb[5];
  for (int l = 0; l < 5; ++l) {
    std::vector<float> w((size_t)kOut[l] * kIn[l]), b((size_t)kOut[l]);
    for (int n = 0; n < kOut[l]; ++n) {
      b[(size_t)n] = bias_of(l, n);
      for (int k = 0; k < kIn[l]; ++k) w[(size_t)n * kIn[l] + k] = weight_of(l, n, k);
    }
    if (to_device(w, &dw[l]) || to_device(b, &db[l])) return 1;
    CHECK_HIP(hipMalloc(&gw[l], w.size() * 4));
    CHECK_HIP(hipMalloc(&gb[l], b.size() * 4));
  }
  const wab_policy_weights weights = {dw[0], db[0], dw[1], db[1], dw[2], db[2], dw[3], db[3], dw[4], db[4]};
  const wab_policy_weights grads = {gw[0], gb[0], gw[1], gb[1], gw[2], gb[2], gw[3], gb[3], gw[4], gb[4]};

  std::vector<float> hx((size_t)kN * kF), hwgt((size_t)kN), htgt((size_t)kN);
  std::vector<int8_t> hact((size_t)kN);
  for (int64_t i = 0; i < kN; ++i) {
    for (int k = 0; k < kF; ++k) hx[(size_t)i * kF + k] = feature_of(i, k);
    hact[(size_t)i] = (int8_t)(i % kA);
    hwgt[(size_t)i] = (float)(i % 7 - 3) / 2.0f;
    htgt[(size_t)i] = (float)(i % 5 - 2) / 2.0f;
  }
  float *x, *wgt, *tgt, *loss, *value;
  int8_t* act;
  if (to_device(hx, &x) || to_device(hwgt, &wgt) || to_device(htgt, &tgt) || to_device(hact, &act)) return 1;
  CHECK_HIP(hipMalloc(&loss, 16));
  CHECK_HIP(hipMalloc(&value, kN * 4));

  wab_policy_loss cfg = {};
  cfg.value_coef = 0.5f;
  cfg.entropy_coef = 0.01f;
  cfg.value_loss = WAB_VALUE_LOSS_SMOOTH_L1;
  cfg.scale = 1.0f;
  cfg.chunk_rows = 128;  // two chunks
  const size_t ws_bytes = wab_policy_grad_workspace(pol, kN, cfg.chunk_rows);
  if (ws_bytes == 0) {
    std::fprintf(stderr, "wab_policy_grad_workspace: %s\n", wab_last_error());
    return 1;
  }
  void* ws = nullptr;
  CHECK_HIP(hipMalloc(&ws, ws_bytes));
  if (wab_policy_grad(pol, x, act, wgt, tgt, kN, &cfg, &grads, loss, nullptr, value, nullptr, ws, ws_bytes, nullptr) !=
      WAB_E_STATE) {
    std::printf("wab_policy_grad before wab_policy_load was not refused\n");
    return 1;
  }
  CHECK_WAB(wab_policy_load(pol, &weights, nullptr));
  if (wab_policy_grad(pol, x, act, wgt, tgt, kN, &cfg, &grads, loss, nullptr, value, nullptr, ws, ws_bytes - 1,
                      nullptr) != WAB_E_INVALID) {
    std::printf("a workspace one byte short was not refused\n");
    return 1;
  }
  CHECK_WAB(wab_policy_grad(pol, x, act, wgt, tgt, kN, &cfg, &grads, loss, nullptr, value, nullptr, ws, ws_bytes,
                            nullptr));
  uint64_t bad = 1;
  CHECK_WAB(wab_policy_grad_bad_actions(pol, ws, nullptr, &bad));

  // the full run's results: sums per tensor, the losses, the optional dump
  std::FILE* dump = argc > 1 ? std::fopen(argv[1], "wb") : nullptr;
  if (argc > 1 && !dump) {
    std::fprintf(stderr, "cannot write %s\n", argv[1]);
    return 1;
  }
  for (int l = 0; l < 5; ++l)
    for (int part = 0; part < 2; ++part) {
      std::vector<float> g(part == 0 ? (size_t)kOut[l] * kIn[l] : (size_t)kOut[l]);
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
  float hl[4];
  CHECK_HIP(hipMemcpy(hl, loss, 16, hipMemcpyDeviceToHost));
  std::printf("loss %.9g %.9g %.9g %.9g\n", (double)hl[0], (double)hl[1], (double)hl[2], (double)hl[3]);
  if (dump) {
    std::fwrite(hl, 4, 4, dump);
    std::fclose(dump);
  }

  // one live row: every other row gets weight 0 and its own value as target, no entropy term
  std::vector<float> hv((size_t)kN);
  CHECK_HIP(hipMemcpy(hv.data(), value, hv.size() * 4, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < kN; ++i)
    if (i != kLive) {
      hwgt[(size_t)i] = 0.0f;
      htgt[(size_t)i] = hv[(size_t)i];
    }
  CHECK_HIP(hipMemcpy(wgt, hwgt.data(), hwgt.size() * 4, hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(tgt, htgt.data(), htgt.size() * 4, hipMemcpyHostToDevice));
  cfg.entropy_coef = 0.0f;
  CHECK_WAB(wab_policy_grad(pol, x, act, wgt, tgt, kN, &cfg, &grads, loss, nullptr, nullptr, nullptr, ws, ws_bytes,
                            nullptr));
  std::vector<float> g1((size_t)kH * kF), b1((size_t)kH);
  CHECK_HIP(hipMemcpy(g1.data(), gw[0], g1.size() * 4, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(b1.data(), gb[0], b1.size() * 4, hipMemcpyDeviceToHost));
  int nonzero = 0;
  for (int n = 0; n < kH; ++n) {
    nonzero += b1[(size_t)n] != 0.0f;
    for (int k = 0; k < kF; ++k) {
      const float want = b1[(size_t)n] * feature_of(kLive, k), got = g1[(size_t)n * kF + k];
      if (std::memcmp(&want, &got, 4) != 0 && !(want == 0.0f && got == 0.0f)) {
        std::printf("one live row: dW1[%d][%d] = %.9g, db1[%d] * x[%d] = %.9g\n", n, k, (double)got, n, k, (double)want);
        return 1;
      }
    }
  }
  if (nonzero < kH / 4) {
    std::printf("one live row: only %d of %d units of layer 1 have a gradient\n", nonzero, kH);
    return 1;
  }

  CHECK_WAB(wab_policy_destroy(pol));
  for (int l = 0; l < 5; ++l)
    for (void* p : {(void*)dw[l], (void*)db[l], (void*)gw[l], (void*)gb[l]}) CHECK_HIP(hipFree(p));
  for (void* p : {(void*)x, (void*)wgt, (void*)tgt, (void*)act, (void*)loss, (void*)value, ws}) CHECK_HIP(hipFree(p));
  std::printf("OK c_api_grad_demo: %lld rows in two chunks, one-live-row outer product exact in %d units\n",
              (long long)kN, nonzero);
  return 0;
}
