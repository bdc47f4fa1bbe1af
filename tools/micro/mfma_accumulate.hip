// Probe: what does v_mfma_f32_32x32x16_bf16 return for D = C + a b when one of its 16 products is
// nonzero?  wab_policy_wgrad_kernel keeps a slab's sum in the instruction's accumulator, so a test
// that predicts the sum bit for bit (tests/test_gpu_policy_grad_slabs.py) needs the instruction's
// own rounding, which is not fl32(C + a b): the accumulator is aligned to the larger exponent and
// cut before the add (tests/policy_grad_cases.py mfma_accumulate has the model).
//
// Every output element (m, n) of a tile gets C[m][n] + A[m][k] B[k][n] for one k (0..15, one per
// tile), A and B bf16 normals of both signs, C an fp32 normal of either sign whose exponent lies
// within +-30 of the product's (and 0 now and then).  Writes N records of four floats (C, a, b, D)
// to the file named, N a multiple of 1024; with no file it prints how many results differ from
// the correctly rounded sum.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o mfma_accumulate mfma_accumulate.hip
//   usage: mfma_accumulate [tiles = 64] [out.f32]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// one wave per tile: a[tile][32], b[tile][32] bf16 bits, c and d [tile][32][32] (m major), kk[tile]
__global__ __launch_bounds__(64) void k_mfma(const uint16_t* a, const uint16_t* b, const float* c, float* d,
                                             const int* kk, int tiles) {
  const int tile = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (tile >= tiles) return;
  const int r = lane & 31, h = lane >> 5, k = kk[tile];
  uint16_t av[8] = {}, bv[8] = {};
  if (k >> 3 == h) {  // lane (r, h) holds k = 8 h .. 8 h + 7 of row m = r of A and of column n = r of B
    av[k & 7] = a[tile * 32 + r];
    bv[k & 7] = b[tile * 32 + r];
  }
  uint4 aw, bw;
  aw.x = av[0] | ((uint32_t)av[1] << 16); aw.y = av[2] | ((uint32_t)av[3] << 16);
  aw.z = av[4] | ((uint32_t)av[5] << 16); aw.w = av[6] | ((uint32_t)av[7] << 16);
  bw.x = bv[0] | ((uint32_t)bv[1] << 16); bw.y = bv[2] | ((uint32_t)bv[3] << 16);
  bw.z = bv[4] | ((uint32_t)bv[5] << 16); bw.w = bv[6] | ((uint32_t)bv[7] << 16);
  f32x16 acc;
  // register q of lane (r, h) is element (m, n) = (8 (q >> 2) + 4 h + (q & 3), r)
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = c[((size_t)tile * 32 + (size_t)(8 * (q >> 2) + 4 * h + (q & 3))) * 32 + (size_t)r];
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, aw), __builtin_bit_cast(bf16x8, bw), acc, 0, 0, 0);
#pragma unroll
  for (int q = 0; q < 16; ++q) d[((size_t)tile * 32 + (size_t)(8 * (q >> 2) + 4 * h + (q & 3))) * 32 + (size_t)r] = acc[q];
}

static uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static float bf16_value(uint16_t v) {
  const uint32_t u = (uint32_t)v << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
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
  const int tiles = argc > 1 ? std::atoi(argv[1]) : 64;
  if (tiles < 1 || tiles > 65536) {
    std::fprintf(stderr, "tiles must be in [1, 65536]\n");
    return 2;
  }
  const size_t n = (size_t)tiles * 1024;
  std::vector<uint16_t> a((size_t)tiles * 32), b((size_t)tiles * 32);
  std::vector<float> c(n), d(n);
  std::vector<int> kk(tiles);
  uint64_t s = 0x5EED;
  auto next = [&]() { return s = mix64(s + 0x9E3779B97F4A7C15ull); };
  for (int t = 0; t < tiles; ++t) {
    kk[t] = (int)(next() % 16);
    for (int i = 0; i < 32; ++i) {
      // bf16 normals, exponents -20 .. 4: sign, 8 exponent bits, 7 mantissa bits
      const uint64_t u = next(), v = next();
      a[(size_t)t * 32 + i] = (uint16_t)(((u >> 40) & 1) << 15 | (uint64_t)(127 - 20 + (u >> 8) % 25) << 7 | (u & 127));
      b[(size_t)t * 32 + i] = (uint16_t)(((v >> 40) & 1) << 15 | (uint64_t)(127 - 20 + (v >> 8) % 25) << 7 | (v & 127));
    }
    for (int m = 0; m < 32; ++m)
      for (int j = 0; j < 32; ++j) {
        const uint64_t u = next();
        const int ea = (a[(size_t)t * 32 + m] >> 7) & 255, eb = (b[(size_t)t * 32 + j] >> 7) & 255;
        const int e = ea + eb - 127 + (int)((u >> 32) % 61) - 30;  // biased, within [27, 195]
        // a third of the mantissas short (a sum of few products), the rest full
        uint32_t mant = (uint32_t)(u & 0x7FFFFFu);
        if ((u >> 24) % 3 == 0) mant &= 0x7FFF00u;
        uint32_t bits = (uint32_t)((u >> 50) & 1) << 31 | (uint32_t)e << 23 | mant;
        if ((u >> 52) % 64 == 0) bits = 0u;
        std::memcpy(&c[((size_t)t * 32 + m) * 32 + j], &bits, 4);
      }
  }
  uint16_t *da, *db;
  float *dc, *dd;
  int* dk;
  CHECK(hipMalloc(&da, a.size() * 2));
  CHECK(hipMalloc(&db, b.size() * 2));
  CHECK(hipMalloc(&dc, n * 4));
  CHECK(hipMalloc(&dd, n * 4));
  CHECK(hipMalloc(&dk, (size_t)tiles * 4));
  CHECK(hipMemcpy(da, a.data(), a.size() * 2, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(db, b.data(), b.size() * 2, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dc, c.data(), n * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dk, kk.data(), (size_t)tiles * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_mfma, dim3((unsigned)tiles), dim3(64), 0, nullptr, da, db, dc, dd, dk, tiles);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(d.data(), dd, n * 4, hipMemcpyDeviceToHost));

  std::vector<float> rec(n * 4);
  size_t differ = 0, inexact = 0;
  for (int t = 0; t < tiles; ++t)
    for (int m = 0; m < 32; ++m)
      for (int j = 0; j < 32; ++j) {
        const size_t i = ((size_t)t * 32 + m) * 32 + j;
        const float av = bf16_value(a[(size_t)t * 32 + m]), bv = bf16_value(b[(size_t)t * 32 + j]);
        rec[4 * i] = c[i]; rec[4 * i + 1] = av; rec[4 * i + 2] = bv; rec[4 * i + 3] = d[i];
        const double exact = (double)c[i] + (double)av * (double)bv;  // (61 bits at most apart: see below)
        const float rne = (float)exact;
        inexact += (double)rne != exact;
        differ += rne != d[i];
      }
  // (the double sum is exact unless the exponents are more than 28 apart, where neither rounding
  // can move the result off the larger operand's neighbourhood; the count is indicative)
  std::printf("%zu results, %zu inexact in fp32, %zu differ from the correctly rounded sum\n", n, inexact, differ);
  if (argc > 2) {
    FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(rec.data(), 16, n, f) != n) {
      std::fprintf(stderr, "cannot write %s\n", argv[2]);
      return 2;
    }
    std::fclose(f);
  }
  return 0;
}
