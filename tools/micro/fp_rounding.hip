// Probe: are the operations wab_policy_adam_step's contract calls "correctly rounded" so on the
// device?  fp64 sqrt and divide, fp32 sqrtf and divide, and the fp64 -> fp32 conversion, compiled
// with the library's flags, over N pseudo-random operands each (every exponent the optimizer can
// meet, fp32 denormals included) plus hand-picked edges, compared bit for bit with the host's
// IEEE results.  Prints the mismatch count per operation and exits non-zero if there is any.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o fp_rounding fp_rounding.hip
//   usage: fp_rounding [N = 2^24]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

__global__ void k_f64(const double* a, const double* b, double* sq, double* dv, float* cv, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  sq[i] = sqrt(a[i]);
  dv[i] = a[i] / b[i];
  cv[i] = (float)a[i];
}

__global__ void k_f32(const float* a, const float* b, float* sq, float* dv, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  sq[i] = sqrtf(a[i]);
  dv[i] = a[i] / b[i];
}

static uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <typename T, typename U>
static size_t mismatches(const char* what, const std::vector<T>& got, const std::vector<T>& want) {
  size_t bad = 0;
  for (size_t i = 0; i < got.size(); ++i) {
    U g, w;
    std::memcpy(&g, &got[i], sizeof(U));
    std::memcpy(&w, &want[i], sizeof(U));
    if (g != w && !(got[i] != got[i] && want[i] != want[i])) {
      if (bad < 3) std::printf("  %s [%zu]: got %.17g, expected %.17g\n", what, i, (double)got[i], (double)want[i]);
      ++bad;
    }
  }
  std::printf("%-28s %zu of %zu differ\n", what, bad, got.size());
  return bad;
}

#define CHECK(x)                                                           \
  do {                                                                     \
    hipError_t e_ = (x);                                                   \
    if (e_ != hipSuccess) {                                                \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));         \
      return 2;                                                            \
    }                                                                      \
  } while (0)

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? (size_t)std::strtoull(argv[1], nullptr, 0) : (size_t)1 << 24;
  std::vector<double> a(n), b(n);
  std::vector<float> fa(n), fb(n);
  uint64_t s = 0x5EED;
  for (size_t i = 0; i < n; ++i) {
    // positive doubles with exponents in [-160, 160] (the norm's S spans the squares of fp32), and
    // positive floats over every exponent, denormals included
    s = mix64(s + 0x9E3779B97F4A7C15ull);
    const uint64_t m1 = s & 0xFFFFFFFFFFFFFull;
    s = mix64(s + 0x9E3779B97F4A7C15ull);
    const uint64_t m2 = s & 0xFFFFFFFFFFFFFull;
    s = mix64(s + 0x9E3779B97F4A7C15ull);
    const uint64_t e1 = 1023 - 160 + (s >> 8) % 321, e2 = 1023 - 160 + (s >> 24) % 321;
    const uint64_t u1 = (e1 << 52) | m1, u2 = (e2 << 52) | m2;
    std::memcpy(&a[i], &u1, 8);
    std::memcpy(&b[i], &u2, 8);
    s = mix64(s + 0x9E3779B97F4A7C15ull);
    const uint32_t v1 = (uint32_t)(s & 0x7FFFFFFFu) % 0x7F800000u, v2 = (uint32_t)((s >> 32) & 0x7FFFFFFFu) % 0x7F800000u;
    std::memcpy(&fa[i], &v1, 4);
    std::memcpy(&fb[i], &v2, 4);
  }
  const double edges[] = {0.0, 1.0, 2.0, 4.0, 0.25, 1.0 + 0x1p-52, 1.0 - 0x1p-53, 2.0 - 0x1p-52, 0x1p-1022, 0x1p-1074,
                          1.7976931348623157e308, INFINITY, NAN, 3.4028234663852886e38, 3.4028235677973366e38,
                          0x1p-149, 0x1p-150, 1.0 + 0x1p-24, 1.0 + 0x1p-24 + 0x1p-52};
  for (size_t i = 0; i < sizeof(edges) / sizeof(edges[0]) && i < n; ++i) {
    a[i] = edges[i];
    fa[i] = (float)edges[i];
  }
  if (n > 40) {
    b[20] = 0.0, fb[20] = 0.0f;
    fa[21] = 1e-30f * 1e-30f, fb[21] = 1e-45f;
  }

  double *da, *db, *dsq, *ddv;
  float *dcv, *dfa, *dfb, *dfsq, *dfdv;
  CHECK(hipMalloc(&da, n * 8));
  CHECK(hipMalloc(&db, n * 8));
  CHECK(hipMalloc(&dsq, n * 8));
  CHECK(hipMalloc(&ddv, n * 8));
  CHECK(hipMalloc(&dcv, n * 4));
  CHECK(hipMalloc(&dfa, n * 4));
  CHECK(hipMalloc(&dfb, n * 4));
  CHECK(hipMalloc(&dfsq, n * 4));
  CHECK(hipMalloc(&dfdv, n * 4));
  CHECK(hipMemcpy(da, a.data(), n * 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(db, b.data(), n * 8, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dfa, fa.data(), n * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dfb, fb.data(), n * 4, hipMemcpyHostToDevice));
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_f64, dim3(blocks), dim3(256), 0, nullptr, da, db, dsq, ddv, dcv, n);
  hipLaunchKernelGGL(k_f32, dim3(blocks), dim3(256), 0, nullptr, dfa, dfb, dfsq, dfdv, n);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<double> sq(n), dv(n), wsq(n), wdv(n);
  std::vector<float> cv(n), fsq(n), fdv(n), wcv(n), wfsq(n), wfdv(n);
  CHECK(hipMemcpy(sq.data(), dsq, n * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(dv.data(), ddv, n * 8, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(cv.data(), dcv, n * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(fsq.data(), dfsq, n * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(fdv.data(), dfdv, n * 4, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    volatile double x = a[i], y = b[i];  // (volatile: computed at run time, in IEEE double and float)
    volatile float fx = fa[i], fy = fb[i];
    wsq[i] = std::sqrt(x);
    wdv[i] = x / y;
    wcv[i] = (float)x;
    wfsq[i] = std::sqrt(fx);
    wfdv[i] = fx / fy;
  }
  size_t bad = 0;
  bad += mismatches<double, uint64_t>("sqrt (double)", sq, wsq);
  bad += mismatches<double, uint64_t>("divide (double)", dv, wdv);
  bad += mismatches<float, uint32_t>("(float) of a double", cv, wcv);
  bad += mismatches<float, uint32_t>("sqrtf", fsq, wfsq);
  bad += mismatches<float, uint32_t>("divide (float)", fdv, wfdv);
  std::printf(bad ? "DIFFERENT\n" : "OK: every operation is correctly rounded on these operands\n");
  return bad ? 1 : 0;
}
