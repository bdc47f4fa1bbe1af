// wab_policy_grad.h — the plan, the workspace layout and the parameter blocks of the device
// policy's loss and parameter gradients (wab_policy_grad.hip; wab_policy_grad in include/wab.h),
// shared with the C-ABI host code.
#pragma once

#include "wab_policy.h"

namespace wab {

constexpr int kGradRows = kPolicyEnvs;  // rows per row block: one workgroup of wab_policy_bwd_kernel
constexpr int kGradTiles = 4;           // 32-unit output tiles one wab_policy_wgrad_kernel wave carries
constexpr int kGradHeadUnits = 16;      // G_4's columns: [0, 8) the action logits, [8] the value, the rest zero
constexpr int kGradMaxSlabs = 64;
constexpr int kGradDefaultChunk = 32768;  // rows per chunk: the bf16 workspace of the reference net is 54 MiB

// wab_policy_bwd_kernel's modes: the loss and gradients of wab_policy_grad, those of the clipped
// surrogate (wab_policy_grad_ppo), or forward and head alone (wab_policy_evaluate)
enum GradMode : int { kGradModeGrad = 0, kGradModePpo = 1, kGradModeEval = 2 };
// The rows' sums a wave hands on, as doubles: {loss_policy, loss_value, entropy} in every gradient
// mode, then the clipped surrogate's {clipped rows, sum of k3, value-clipped rows, sum of r}.
constexpr int kGradLossTerms = 3;  // terms of wab_policy_grad
constexpr int kGradPpoTerms = 7;   // terms of wab_policy_grad_ppo
constexpr int kGradTermPitch = 8;  // doubles per wave and per slab

// The transposed packed weights the backward chain reads (the A operands of dx_l = D_{l+1} . W_{l+1}):
// image l is pack_layer's layout of W_{l+1}^T, NT_l tiles of 32 units of layer l by KS k-steps of
// 16 units of layer l + 1.  The head's image has one k-step: columns 0..7 the action head's rows,
// column 8 the value head.
//
// The bf16 workspace of one chunk holds, for every unit u of X_1, X_2, X_3, D_1, D_2, D_3, D_4 in
// that order (each array padded to its 32 NT units, D_4 to 16), the chunk's rows as one contiguous
// run of chunk_rows bf16: element (u, row) at u * chunk_rows + row.  Eight consecutive rows of a unit are
// the 16 bytes a lane of v_mfma_f32_32x32x16_bf16 holds of either operand of D^T . X.
//
// wab_policy_wgrad_kernel's tasks: for layer l (1, 2, 3, head) the pairs (group of up to 4 output
// tiles of D_l, 32-column tile of [X_{l-1} | 1]); column K_in of a layer is the column of ones
// whose product is the bias gradient.  Task t of slab s keeps its 4 accumulators, as the lanes
// hold them, at ((s * n_tasks + t) * 4 + tile) * 1024 + reg * 64 + lane floats.
struct GradPlan {
  PolicyDims d;
  // wab_policy_bwd_kernel's LDS, wab_policy_kernel's two regions: region A holds the input chunk,
  // then X_2, then D_4 [128][pitch4], then D_2; region B X_1, X_3, then D_3
  PolicyLds lds;
  int32_t pitch4;
  // transposed image (uint16 units) and its k-steps
  uint32_t wt1, wt2, wt3, wt_total;
  int32_t KT1, KT2, KT3;  // ceil(h2 / 16), ceil(h3 / 16), 1
  // workspace units
  int32_t u_x[4];   // u_x[l]: X_l, l = 1..3 (u_x[0] unused)
  int32_t u_d[5];   // u_d[l]: D_l, l = 1..4
  int32_t n_d[5];   // units of D_l held (32 NT_l; 16 for the head)
  int32_t u_total;
  // wgrad tasks: layer l = 1..4 has groups[l] * ktiles[l] tasks from task0[l]
  int32_t k_in[5], n_out[5], groups[5], ktiles[5], task0[6];
  int32_t n_tasks, slabs;
};

__host__ __device__ inline GradPlan grad_plan(const PolicyDims& d) {
  GradPlan g;
  g.d = d;
  g.lds = policy_lds(d, kGradRows, kPolicyLdsBudget);
  g.pitch4 = kGradHeadUnits + 8;  // (D_4's 6 KB fit region A: X_2's pitch is >= 40)

  g.KT1 = (d.h2 + 15) / 16;
  g.KT2 = (d.h3 + 15) / 16;
  g.KT3 = 1;
  uint32_t o = 0;
  g.wt1 = o; o += (uint32_t)(d.NT1 * g.KT1) * 512u;
  g.wt2 = o; o += (uint32_t)(d.NT2 * g.KT2) * 512u;
  g.wt3 = o; o += (uint32_t)(d.NT3 * g.KT3) * 512u;
  g.wt_total = o;

  const int nt[4] = {0, d.NT1, d.NT2, d.NT3};
  int u = 0;
  g.u_x[0] = 0;
  for (int l = 1; l <= 3; ++l) { g.u_x[l] = u; u += 32 * nt[l]; }
  g.u_d[0] = 0; g.n_d[0] = 0;
  for (int l = 1; l <= 3; ++l) { g.u_d[l] = u; g.n_d[l] = 32 * nt[l]; u += 32 * nt[l]; }
  g.u_d[4] = u; g.n_d[4] = kGradHeadUnits; u += kGradHeadUnits;
  g.u_total = u;

  g.k_in[0] = 0; g.n_out[0] = 0; g.groups[0] = 0; g.ktiles[0] = 0;
  g.k_in[1] = d.F;  g.n_out[1] = d.h1;
  g.k_in[2] = d.h1; g.n_out[2] = d.h2;
  g.k_in[3] = d.h2; g.n_out[3] = d.h3;
  g.k_in[4] = d.h3; g.n_out[4] = kPolicyMaxActions + 1;
  int t = 0;
  g.task0[0] = 0;
  for (int l = 1; l <= 4; ++l) {
    const int tiles = l < 4 ? nt[l] : 1;
    g.groups[l] = (tiles + kGradTiles - 1) / kGradTiles;
    g.ktiles[l] = (g.k_in[l] + 1 + 31) / 32;
    g.task0[l] = t;
    t += g.groups[l] * g.ktiles[l];
  }
  g.task0[5] = t;
  g.n_tasks = t;
  // slabs: about two waves per SIMD of the chip over all tasks, a function of the shape alone
  int s = (2048 + t - 1) / t;
  g.slabs = s < 1 ? 1 : (s > kGradMaxSlabs ? kGradMaxSlabs : s);
  return g;
}

// byte offsets of the workspace's parts for chunks of `chunk_rows` rows
struct GradWorkspace {
  size_t bad, wt, ws, slab, part, loss, total;
};

inline GradWorkspace grad_workspace(const GradPlan& g, int64_t chunk_rows) {
  auto up = [](size_t x) { return (x + 255u) & ~(size_t)255u; };
  GradWorkspace w;
  size_t o = 0;
  // two uint32: rows of the latest call whose action was outside [0, A); at offset 4, rows of a
  // gathered call whose index was outside the source [0, M) (such a row counts there alone)
  w.bad = o; o = up(o + 8u);
  w.wt = o; o = up(o + (size_t)g.wt_total * 2u);
  w.ws = o; o = up(o + (size_t)g.u_total * (size_t)chunk_rows * 2u);
  w.slab = o; o = up(o + (size_t)g.slabs * (size_t)g.n_tasks * (size_t)(kGradTiles * 1024) * 4u);
  w.part = o; o = up(o + (size_t)(chunk_rows / kGradRows) * 4u * (size_t)kGradTermPitch * 8u);  // [block][wave][8] doubles
  w.loss = o; o = up(o + (size_t)g.slabs * (size_t)kGradTermPitch * 8u);                         // [slab][8] doubles
  w.total = o;
  return w;
}

struct GradPackParams {
  GradPlan g;
  const uint16_t* w;  // the forward image (PolicyDims::w*)
  uint16_t* wt;
  uint32_t* bad;      // both counts, zeroed for the call
};

struct GradBwdParams {
  GradPlan g;
  int64_t N, row0;         // all rows; the chunk's first row (a multiple of 128)
  int64_t chunk_rows;      // the workspace's row pitch
  const float* features;   // [N][F]; GATHER: the source, [M][F]
  const int8_t* actions;   // [N]; GATHER: this and the next four [M], read at the row's source row
  const float* weight;     // [N]: the weight, or the advantage of the clipped surrogate
  const float* target;     // [N]
  const float* old_logp;   // [N] (clipped surrogate)
  const float* old_value;  // [N] or null (clipped surrogate with value_clip > 0)
  float clip, value_clip;  // (clipped surrogate) value_clip <= 0: off
  const uint16_t* w;       // forward image
  const float* b;          // padded biases
  const uint16_t* wt;      // transposed image
  float value_coef, entropy_coef;
  int32_t mse;             // 0: smooth_l1 (beta 1), 1: 0.5 d^2
  float* logp;             // [N] or null
  float* value;            // [N] or null
  float* entropy;          // [N] or null
  float* ratio;            // [N] or null (clipped surrogate)
  uint16_t* ws;            // bf16 workspace of the chunk (null: evaluate)
  double* part;            // [chunk block][wave][8]: the waves' sums of the rows' loss terms
  uint32_t* bad;           // bad[0]: count of rows whose action is outside [0, A); bad[1] (GATHER): of
                           // rows whose index is outside [0, M), which are left out in the same way
  const int32_t* rows;     // GATHER: [N], the source row of each row (null otherwise)
  int64_t M;               // GATHER: the source's rows, in [1, 2^31)
  const uint32_t* bits;    // PACKED: the rows' features as packed bits [N][P] (GATHER: [M][P]); features null
  int32_t P;               // PACKED: dwords per packed row (feature_bits_pitch)
};

struct GradWgradParams {
  GradPlan g;
  int64_t N, row0;
  int64_t chunk_rows;
  int32_t n_blocks;        // row blocks of this chunk
  int32_t first;           // 1: the slabs start from zero (the call's first chunk)
  int32_t n_terms;         // loss terms the call sums: kGradLossTerms or kGradPpoTerms
  const float* features;
  const uint16_t* ws;
  const double* part;
  float* slab;
  double* loss;
  const int32_t* rows;     // GATHER: as GradBwdParams'
  int64_t M;
  const uint32_t* bits;    // PACKED: as GradBwdParams'
  int32_t P;
};

struct GradReduceParams {
  GradPlan g;
  int32_t empty;           // 1: N == 0, the slabs hold nothing
  int32_t accumulate;
  float scale, value_coef, entropy_coef;
  const float* slab;
  const double* loss;
  PolicyTensors<float*> out;  // the ten gradients
  float* loss_out;         // {policy, value, entropy, total}
  float* ppo_out;          // {clipped rows, sum of k3, value-clipped rows, sum of r} or null
};

// the kernels (wab_policy_grad.hip), launched from wab_capi_policy.hip
__global__ void wab_policy_grad_pack(GradPackParams p);
// (GATHER: the rows are taken through GradBwdParams::rows, wab_policy_*_gather)
// (PACKED: the features are GradBwdParams::bits, wab_policy_*_packed)
template <bool TWO, int MODE = kGradModeGrad, bool GATHER = false, bool PACKED = false>
__global__ void wab_policy_bwd_kernel(GradBwdParams p);
template <bool GATHER = false, bool PACKED = false>
__global__ void wab_policy_wgrad_kernel(GradWgradParams p);
__global__ void wab_policy_grad_reduce_kernel(GradReduceParams p);

}  // namespace wab
