// Train-time glue of a transformer block in libqvit_hip.so (gfx950): the pre-op of a QuantizeLinear (LayerNorm or
// GELU) fused with that layer's activation quantizer, forward for GELU and backward for both, so that no fp32
// tensor of the pre-op's output is written, saved or read back.
//
//   qvit_layernorm_quant_backward  per row: recompute y = LayerNorm(x) exactly as the forward's ln_quant_row did
//                                  (ln_row_values), the quantizer backward at (y, grad_y) (backward_element of
//                                  qvit_quant_backward), then the LayerNorm backward. Reads x and grad_y once,
//                                  writes grad_x once: 3 rows cols 4 bytes, plus the partials below.
//   (qvit_gelu_quant_i8, the forward of the GELU pair, is qvit_quantize_act_i8's kernel with gelu_ref in front: it
//   lives beside it in quant_kernels.hip.)
//   qvit_gelu_quant_backward       qvit_quant_backward at a = GELU(h), grad_h = GELU'(h) * gy: 3 n 4 bytes.
//
// Reductions leave the kernels through per-workgroup partials folded in a fixed order by a second launch (no float
// atomics): a call is bitwise reproducible.
#include "qvit_common.h"
#include "ln_common.h"
#include "quant_bwd_common.h"

namespace {

constexpr int kLnMaxCols = 2048; // 8 float4 per lane

// ---- LayerNorm + quantizer backward: one wave per row -------------------------------------------------------
inline int ln_bwd_grid(int64_t rows) {
  const int64_t g = cdiv(rows, kWaves);
  return (int)(g < 1 ? 1 : (g < kGridCap ? g : kGridCap));
}

// Workspace: double [grid][3] scalar partials, then float [grid][2][cols] column partials (x-hat sums, plain sums).
// (the column part starts on a 16-byte boundary: it is written as float4)
inline int64_t ln_bwd_col_offset(int grid) { return ((int64_t)grid * 3 * (int64_t)sizeof(double) + 15) / 16 * 16; }

QVIT_DEV void acc4(float4& a, const float4& g, const float4& h) {
  a.x += g.x * h.x; a.y += g.y * h.y; a.z += g.z * h.z; a.w += g.w * h.w;
}

// Lane l holds columns 4 (l + 64 i) .. + 3 of its wave's row (the forward's layout). x and grad_y of the row stay
// in registers; a wave walks rows wave, wave + nwaves, ... and carries its column and scalar partials in registers.
// grad_y and grad_x may be the same buffer (ldg == ldo): a lane reads its 16-byte pieces of a row before it writes
// the same pieces, and a row belongs to one wave.
template <int NV, bool NONLINEAR>
__global__ __launch_bounds__(kThreads) void layernorm_quant_backward_kernel(
    const float* __restrict__ x, int64_t rows, int cols, int64_t ldx, const float* __restrict__ gamma,
    const float* __restrict__ beta, float eps, int qtype, const float* d, const float* qm, const float* t,
    float clip_lo, float clip_hi, const float* grad_y, int64_t ldg, float* grad_x, int64_t ldo, double* partials,
    float* col_partials) {
  __shared__ __attribute__((aligned(16))) float4 gbl[2 * 64 * NV];   // gamma, beta; then the block's column sums
  __shared__ double lds[kWaves][3];
  const BwdParams b = load_bwd_params<NONLINEAR>(qtype, d, qm, t, clip_lo, clip_hi, 0.f);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < 64 * NV; k += kThreads) {
    const int c = 4 * k;
    gbl[k] = (c < cols) ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(1.f, 1.f, 1.f, 1.f);
    gbl[64 * NV + k] = (c < cols) ? *reinterpret_cast<const float4*>(beta + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();

  double sd = 0.0, sq = 0.0, st = 0.0;
  float4 cg[NV], cb[NV];   // sum over this wave's rows of gy * xhat and of gy
#pragma unroll
  for (int i = 0; i < NV; ++i) cg[i] = cb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const float inv_cols = 1.0f / (float)cols;

  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < rows; r += nwaves) {
    float4 v[NV], g[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = 4 * (lane + 64 * i);
      const bool in = c < cols;
      v[i] = in ? *reinterpret_cast<const float4*>(x + r * ldx + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      g[i] = in ? *reinterpret_cast<const float4*>(grad_y + r * ldg + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float mean, rstd;
    float4 xh[NV], y[NV];
    ln_row_values<NV>(v, lane, cols, eps,
                      [&](int i, float4& gv, float4& bv) {
                        gv = gbl[lane + 64 * i];
                        bv = gbl[64 * NV + lane + 64 * i];
                      },
                      mean, rstd, xh, y);
    // quantizer backward at (y, grad_y): gy replaces g; lanes past the row hold zeros and add nothing
    float sa = 0.f, sb = 0.f;   // sum_c gamma gy, sum_c gamma gy xhat
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = 4 * (lane + 64 * i);
      if (c < cols) {
        g[i].x = backward_element<NONLINEAR, false>(y[i].x, g[i].x, b, sd, sq, st);
        g[i].y = backward_element<NONLINEAR, false>(y[i].y, g[i].y, b, sd, sq, st);
        g[i].z = backward_element<NONLINEAR, false>(y[i].z, g[i].z, b, sd, sq, st);
        g[i].w = backward_element<NONLINEAR, false>(y[i].w, g[i].w, b, sd, sq, st);
        acc4(cg[i], g[i], xh[i]);
        cb[i].x += g[i].x; cb[i].y += g[i].y; cb[i].z += g[i].z; cb[i].w += g[i].w;
        const float4 gv = gbl[lane + 64 * i];
        g[i].x *= gv.x; g[i].y *= gv.y; g[i].z *= gv.z; g[i].w *= gv.w;   // a = gamma gy
        sa += (g[i].x + g[i].y) + (g[i].z + g[i].w);
        sb += (g[i].x * xh[i].x + g[i].y * xh[i].y) + (g[i].z * xh[i].z + g[i].w * xh[i].w);
      }
    }
    const float ma = wave_sum_fast(sa) * inv_cols, mb = wave_sum_fast(sb) * inv_cols;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = 4 * (lane + 64 * i);
      if (c < cols) {
        float4 o;
        o.x = rstd * (g[i].x - ma - xh[i].x * mb);
        o.y = rstd * (g[i].y - ma - xh[i].y * mb);
        o.z = rstd * (g[i].z - ma - xh[i].z * mb);
        o.w = rstd * (g[i].w - ma - xh[i].w * mb);
        *reinterpret_cast<float4*>(grad_x + r * ldo + c) = o;
      }
    }
  }

  block_sum3(sd, sq, st, lds);
  if (tid == 0) store_partial3(partials, sd, sq, st);
  if (col_partials == nullptr) return;
  // column sums of the block: the waves add into LDS one after the other, in wave order
  __syncthreads();   // gamma / beta are no longer read
  for (int w = 0; w < kWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int k = lane + 64 * i;
        if (w == 0) {
          gbl[k] = cg[i];
          gbl[64 * NV + k] = cb[i];
        } else {
          float4 a = gbl[k], c2 = gbl[64 * NV + k];
          a.x += cg[i].x; a.y += cg[i].y; a.z += cg[i].z; a.w += cg[i].w;
          c2.x += cb[i].x; c2.y += cb[i].y; c2.z += cb[i].z; c2.w += cb[i].w;
          gbl[k] = a;
          gbl[64 * NV + k] = c2;
        }
      }
    }
    __syncthreads();
  }
  float* out = col_partials + (int64_t)blockIdx.x * 2 * cols;
  for (int k = tid; 4 * k < cols; k += kThreads) {
    *reinterpret_cast<float4*>(out + 4 * k) = gbl[k];
    *reinterpret_cast<float4*>(out + cols + 4 * k) = gbl[64 * NV + k];
  }
}

// Second stage. The last block folds the scalar partials as scalar_finish_kernel does. Every other block
// owns kFinCols columns: the workgroup partials are cut into kFinChunks equal runs, thread (chunk, column) adds its
// run of its column in ascending workgroup order, and the chunk-0 thread adds the kFinChunks run sums in ascending
// order (one thread walking all 1024 partials of a column alone is a chain of dependent-latency loads that costs
// several times the main kernel). The order depends on nblocks only: bitwise reproducible. nblocks == 0: zeros.
constexpr int kFinCols = 16, kFinChunks = kThreads / kFinCols;

__global__ __launch_bounds__(kThreads) void layernorm_quant_backward_finish_kernel(
    const double* partials, const float* col_partials, int nblocks, int cols, float* grad_gamma, float* grad_beta,
    float* grad_scalars) {
  __shared__ double lds[kWaves][3];
  __shared__ double run[kFinChunks][kFinCols][2];
  if (blockIdx.x == gridDim.x - 1) {
    // (scalar_finish_kernel's loop, kept here: behind a helper the compiler allocates the sums differently)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = threadIdx.x; j < nblocks; j += kThreads) {
      s0 += partials[(int64_t)j * 3 + 0];
      s1 += partials[(int64_t)j * 3 + 1];
      s2 += partials[(int64_t)j * 3 + 2];
    }
    block_sum3(s0, s1, s2, lds);
    if (threadIdx.x == 0) {
      grad_scalars[0] = (float)s0;
      grad_scalars[1] = (float)s1;
      grad_scalars[2] = (float)s2;
    }
    return;
  }
  const int cl = threadIdx.x % kFinCols, chunk = threadIdx.x / kFinCols;
  const int c = blockIdx.x * kFinCols + cl;
  const int per = (nblocks + kFinChunks - 1) / kFinChunks;
  const int j0 = chunk * per, j1 = (j0 + per < nblocks) ? j0 + per : nblocks;
  double sg = 0.0, sb = 0.0;
  if (c < cols) {
    for (int j = j0; j < j1; ++j) {
      const float* p = col_partials + (int64_t)j * 2 * cols;
      sg += (double)p[c];
      sb += (double)p[cols + c];
    }
  }
  run[chunk][cl][0] = sg;
  run[chunk][cl][1] = sb;
  __syncthreads();
  if (chunk == 0 && c < cols) {
    sg = run[0][cl][0];
    sb = run[0][cl][1];
#pragma unroll
    for (int k = 1; k < kFinChunks; ++k) {
      sg += run[k][cl][0];
      sb += run[k][cl][1];
    }
    if (grad_gamma) grad_gamma[c] = (float)sg;
    if (grad_beta) grad_beta[c] = (float)sb;
  }
}

// ---- GELU + quantizer backward (the forward, qvit_gelu_quant_i8: quant_kernels.hip's rows_to_codes_kernel) -------
// GELU'(v) = Phi(v) + v phi(v) from the pieces gelu_ref computes: Phi = (1 + erf(v / sqrt 2)) / 2 with the same erf,
// phi(v) = exp(-v^2 / 2) / sqrt(2 pi) with the same exponential (the compiler shares them with gelu_ref's).
QVIT_DEV float gelu_grad(float x) {
#pragma clang fp contract(off)
  const float u = x * 0.70710678118654752440f;
  const float t = 1.0f / fmaf(0.3275911f, fabsf(u), 1.0f);
  float r = fmaf(1.061405429f, t, -1.453152027f);
  r = fmaf(r, t, 1.421413741f);
  r = fmaf(r, t, -0.284496736f);
  r = fmaf(r, t, 0.254829592f);
  const float e = sleef_expf_u10(-(u * u));
  const float erf_abs = fmaf(-e * t, r, 1.0f);
  const float cdf = 0.5f * (1.0f + copysignf(erf_abs, u));
  return fmaf(x * 0.3989422804014327f, e, cdf);
}

// quant_backward_kernel (quant_backward.hip) at a = GELU(h): the sums and gy from backward_element, grad_h =
// GELU'(h) gy. A masked element (gy = 0) gives 0 GELU'(h), so a NaN in grad_y stays in its own element.
template <bool NONLINEAR>
QVIT_DEV float gelu_backward_element(float h, float g, const BwdParams& b, double& sd, double& sq, double& st) {
  const float gy = backward_element<NONLINEAR, false>(gelu_ref(h), g, b, sd, sq, st);
  return gelu_grad(h) * gy;
}

template <bool NONLINEAR>
__global__ __launch_bounds__(kThreads) void gelu_quant_backward_kernel(
    const float* __restrict__ h, const float* grad_y, int64_t n, int qtype, const float* d, const float* qm,
    const float* t, float clip_lo, float clip_hi, float* grad_h, double* partials) {
  __shared__ double lds[kWaves][3];
  const BwdParams b = load_bwd_params<NONLINEAR>(qtype, d, qm, t, clip_lo, clip_hi, 0.f);
  double sd = 0.0, sq = 0.0, st = 0.0;
  const int64_t nvec = n / kVec;
  const int64_t tid = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const float4* h4 = reinterpret_cast<const float4*>(h);
  const float4* g4 = reinterpret_cast<const float4*>(grad_y);
  float4* o4 = reinterpret_cast<float4*>(grad_h);
  for (int64_t i = tid; i < nvec; i += stride) {
    const float4 hv = h4[i], gv = g4[i];
    float4 o;
    o.x = gelu_backward_element<NONLINEAR>(hv.x, gv.x, b, sd, sq, st);
    o.y = gelu_backward_element<NONLINEAR>(hv.y, gv.y, b, sd, sq, st);
    o.z = gelu_backward_element<NONLINEAR>(hv.z, gv.z, b, sd, sq, st);
    o.w = gelu_backward_element<NONLINEAR>(hv.w, gv.w, b, sd, sq, st);
    o4[i] = o;
  }
  // scalar tail: the last n % 4 elements, one per thread of the grid's first threads
  const int64_t e = nvec * kVec + tid;
  if (e < n) grad_h[e] = gelu_backward_element<NONLINEAR>(h[e], grad_y[e], b, sd, sq, st);

  block_sum3(sd, sq, st, lds);
  if (threadIdx.x == 0) store_partial3(partials, sd, sq, st);
}

}  // namespace

extern "C" {

int64_t qvit_layernorm_quant_backward_workspace_bytes(int64_t rows, int64_t cols) {
  if (rows < 0 || cols < 0) return QVIT_EINVAL;
  const int grid = ln_bwd_grid(rows);
  return ln_bwd_col_offset(grid) + (int64_t)grid * 2 * cols * (int64_t)sizeof(float);
}

int qvit_layernorm_quant_backward(const float* x, int64_t rows, int64_t cols, int64_t ldx, const float* gamma,
                                  const float* beta, float eps, int qtype, const float* d_quant, const float* q_m,
                                  const float* t_quant, float clip_lo, float clip_hi, const float* grad_y,
                                  int64_t ldg, float* grad_x, int64_t ldo, float* grad_gamma, float* grad_beta,
                                  float* grad_scalars, void* workspace, int64_t workspace_bytes,
                                  hipStream_t stream) {
  if (!x || !gamma || !beta || !grad_y || !grad_x || !grad_scalars || !d_quant || !q_m || !workspace)
    return QVIT_ENULL;
  bool nonlinear = false;
  if (qvit_backward_qtype_status(qtype, nonlinear)) return QVIT_EINVAL;
  if (nonlinear && !t_quant) return QVIT_ENULL;
  if (rows < 0 || cols <= 0 || ldx < cols || ldg < cols || ldo < cols) return QVIT_EINVAL;
  if (workspace_bytes < qvit_layernorm_quant_backward_workspace_bytes(rows, cols)) return QVIT_EINVAL;
  if ((cols & 3) || cols > kLnMaxCols || (ldx & 3) || (ldg & 3) || (ldo & 3)) return QVIT_EALIGN;
  if (qvit_misaligned(15, x, gamma, beta, grad_y, grad_x, workspace)) return QVIT_EALIGN;
  if (qvit_misaligned(3, grad_gamma, grad_beta)) return QVIT_EALIGN;

  int grid = 0;
  double* partials = static_cast<double*>(workspace);
  float* colp = nullptr;
  if (rows > 0) {
    grid = ln_bwd_grid(rows);
    if (grad_gamma || grad_beta)
      colp = reinterpret_cast<float*>(static_cast<char*>(workspace) + ln_bwd_col_offset(grid));
    const dim3 g(grid), blk(kThreads);
    const int nv = (int)((cols + 255) / 256);
#define QVIT_LNB(NV)                                                                                               \
  do {                                                                                                             \
    if (nonlinear)                                                                                                 \
      hipLaunchKernelGGL((layernorm_quant_backward_kernel<NV, true>), g, blk, 0, stream, x, rows, (int)cols, ldx,  \
                         gamma, beta, eps, qtype, d_quant, q_m, t_quant, clip_lo, clip_hi, grad_y, ldg, grad_x,    \
                         ldo, partials, colp);                                                                     \
    else                                                                                                           \
      hipLaunchKernelGGL((layernorm_quant_backward_kernel<NV, false>), g, blk, 0, stream, x, rows, (int)cols, ldx, \
                         gamma, beta, eps, qtype, d_quant, q_m, t_quant, clip_lo, clip_hi, grad_y, ldg, grad_x,    \
                         ldo, partials, colp);                                                                     \
  } while (0)
    if (nv <= 1) QVIT_LNB(1);
    else if (nv <= 2) QVIT_LNB(2);
    else if (nv <= 3) QVIT_LNB(3);
    else if (nv <= 4) QVIT_LNB(4);
    else QVIT_LNB(8);
#undef QVIT_LNB
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qvit_hip_status(e);
  }
  const int col_blocks = (grad_gamma || grad_beta) ? (int)cdiv(cols, kFinCols) : 0;
  hipLaunchKernelGGL(layernorm_quant_backward_finish_kernel, dim3(col_blocks + 1), dim3(kThreads), 0, stream, partials,
                     colp, grid, (int)cols, grad_gamma, grad_beta, grad_scalars);
  return qvit_launch_status();
}

int64_t qvit_gelu_quant_backward_workspace_bytes(int64_t n) {
  if (n < 0) return QVIT_EINVAL;
  return (int64_t)stream_grid(n, kVec) * 3 * (int64_t)sizeof(double);
}

int qvit_gelu_quant_backward(const float* h, const float* grad_y, int64_t n, int qtype, const float* d_quant,
                             const float* q_m, const float* t_quant, float clip_lo, float clip_hi, float* grad_h,
                             float* grad_scalars, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  if (!h || !grad_y || !grad_h || !grad_scalars || !d_quant || !q_m || !workspace) return QVIT_ENULL;
  bool nonlinear = false;
  if (qvit_backward_qtype_status(qtype, nonlinear)) return QVIT_EINVAL;
  if (nonlinear && !t_quant) return QVIT_ENULL;
  if (n < 0) return QVIT_EINVAL;
  if (workspace_bytes < qvit_gelu_quant_backward_workspace_bytes(n)) return QVIT_EINVAL;
  if (qvit_misaligned(15, h, grad_y, grad_h) || qvit_misaligned(7, workspace)) return QVIT_EALIGN;

  double* partials = static_cast<double*>(workspace);
  int grid = 0;
  if (n > 0) {
    grid = stream_grid(n, kVec);
    if (nonlinear)
      hipLaunchKernelGGL(gelu_quant_backward_kernel<true>, dim3(grid), dim3(kThreads), 0, stream, h, grad_y, n, qtype,
                         d_quant, q_m, t_quant, clip_lo, clip_hi, grad_h, partials);
    else
      hipLaunchKernelGGL(gelu_quant_backward_kernel<false>, dim3(grid), dim3(kThreads), 0, stream, h, grad_y, n, qtype,
                         d_quant, q_m, t_quant, clip_lo, clip_hi, grad_h, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qvit_hip_status(e);
  }
  hipLaunchKernelGGL(scalar_finish_kernel, dim3(1), dim3(kThreads), 0, stream, partials, grid, grad_scalars);
  return qvit_launch_status();
}

}  // extern "C"
