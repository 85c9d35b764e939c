// Streaming grids and fixed-order reductions shared by the quantizer, training and UltraNet kernels. No float
// atomics anywhere: per-thread double accumulation, the wave tree, the waves in index order, one partial per block in
// the caller's workspace, and a second launch in which thread i adds partials i, i + 256, ... in that order before
// the same tree. The same call gives the same bits.
#pragma once
#include <algorithm>

#include "qvit_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGridCap = 1024;   // 4 blocks per CU; a grid-stride loop covers the rest
constexpr int kVec = 4;          // floats per 16-byte access

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// blocks of a streaming pass over n elements, per_thread of them per thread and step, capped at kGridCap
inline int stream_grid(int64_t n, int per_thread) {
  const int64_t g = cdiv(n / per_thread, kThreads);
  return (int)(g < 1 ? 1 : (g < kGridCap ? g : kGridCap));
}

// blocks of a grid-stride pass over `work` items, one per thread and step
inline int grid_for(int64_t work, int threads) {
  const int64_t g = cdiv(work, threads);
  const int64_t cap = 256 * 16;  // 16 blocks per CU, grid-stride beyond
  return (int)(g < cap ? (g > 0 ? g : 1) : cap);
}

// wave64 sum in a fixed order; lane 0 holds the result
QVIT_DEV double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Sums of one block: every wave reduces its lanes, wave w leaves its three sums in lds[w], thread 0 adds the
// waves in index order. Returns the totals in thread 0 (other threads: unspecified).
QVIT_DEV void block_sum3(double& s0, double& s1, double& s2, double (*lds)[3]) {
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    lds[wave][0] = s0; lds[wave][1] = s1; lds[wave][2] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s0 = lds[0][0]; s1 = lds[0][1]; s2 = lds[0][2];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      s0 += lds[w][0]; s1 += lds[w][1]; s2 += lds[w][2];
    }
  }
}

// block_sum3's totals as partial blockIdx.x (three sums; every user keeps one triple per block), resp. as partial j
// (two sums; the users index by block or by channel slot). Both are called by thread 0 ALONE: they do not test the
// thread themselves, so that the index is computed inside the caller's `if (threadIdx.x == 0)`.
QVIT_DEV void store_partial3(double* partials, double s0, double s1, double s2) {
  double* out = partials + (int64_t)blockIdx.x * 3;
  out[0] = s0; out[1] = s1; out[2] = s2;
}
QVIT_DEV void store_partial2(double* __restrict__ partials, int64_t j, double s0, double s1) {
  partials[2 * j] = s0;
  partials[2 * j + 1] = s1;
}

// Second stage, one block, two sums: thread i adds partials i, i + 256, ... in that order to its sums (the caller's
// zeros), then the block reduces as above (totals in thread 0). n == 0 leaves zeros.
QVIT_DEV void fold_partials2(const double* __restrict__ p, int n, double& s0, double& s1, double (*lds)[3]) {
  for (int j = threadIdx.x; j < n; j += kThreads) {
    s0 += p[2 * (int64_t)j];
    s1 += p[2 * (int64_t)j + 1];
  }
  double unused = 0.0;
  block_sum3(s0, s1, unused, lds);
}

// ---- split weight gradients (qvit_gemm_wgrad, qvit_conv_wgrad) -----------------------------------------------
// The contraction is dealt in stages to `splits` workgroups (or waves) per output tile, each writing its raw fp32
// partial tile to part[split][npad][kpad]: as many as the stages allow, up to max_splits, until about `target` run.
inline int64_t split_count(int64_t tiles, int64_t stages, int64_t max_splits, int64_t target) {
  return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(max_splits, stages), cdiv(target, tiles)));
}

QVIT_DEV float fold_scale(const float* p) { return *p; }
QVIT_DEV float fold_scale(float v) { return v; }

// dW[n][k] = scale * sum_sp part[sp][n][k], the partials summed in ascending split order (splits == 0: zeros).
// Scale: a device pointer (d_act) or the value itself (1 / levels). Ldw: dW's row stride, or nothing for a dense dW.
// (A pack, so that the dense kernel has no stride argument at all: its kernel-argument layout and its code stay the
// ones it had before the two fold kernels were merged. Each instantiation is the kernel that ran before.)
template <typename Scale, typename... Ldw>
__global__ __launch_bounds__(256) void split_fold_kernel(const float* __restrict__ part, int splits, int N, int K,
                                                         int npad, int kpad, Scale scale, float* __restrict__ dW,
                                                         Ldw... ldw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)N * K) return;
  const int n = (int)(i / K), k = (int)(i - (int64_t)n * K);
  float v = 0.f;
  if (splits > 0) {
    float a = part[(int64_t)n * kpad + k];
    for (int sp = 1; sp < splits; ++sp) a += part[((int64_t)sp * npad + n) * kpad + k];
    v = fold_scale(scale) * a;
  }
  if constexpr (sizeof...(Ldw) == 0) dW[i] = v;
  else dW[(int64_t)n * (ldw, ...) + k] = v;
}

}  // namespace
