// Quantizer backward of libqvit_hip.so (gfx950): the backward passes of SymQuantizerLinear
// (OTO/quantization/quant_layers.py:163-205), SymQuantizerNonLinear (:71-125) and DGEQuantizer (:248-290) as
// one streaming pass. Per element it reads x and grad_out once (16 B per lane), writes grad_x once and adds
// grad_out * term into three per-thread sums (d_quant, q_m, t_quant); the sums leave the kernel through a
// fixed-order two-stage reduction (no float atomics), so a call is bitwise reproducible.
//
// Regions of an element (a = |x|, q_s = 0), in the reference's order of assignment (later masks overwrite):
//            interior                 a >= q_m (:90,:102,:178)          a <= 0 (:93,:103,:181)
//   d term   sgn (rne(q) - q)         sgn (L - range_pow / d)           0
//   t term   sgn p ln a               sgn range_pow ln(|q_m| + 1e-6)    0
//   q_m term sgn c where not (a <= q_m) (:98,:186), else 0; c = 1 (linear) or t exp((t-1) ln(|q_m| + 1e-6))
// rne(q) is the forward's code (quant_code), so the two passes agree on every element, rounding ties included.
// Masks select: the value computed for a masked-out region (0 * -inf at x = 0) never reaches a sum, while a NaN
// in grad_out or in a parameter does (NaN * 0 = NaN, as in the reference's grad_output * term).
#include "quant_bwd_common.h"

namespace {

template <bool NONLINEAR, bool DGE>
QVIT_DEV float4 backward_vec(const float4& x, const float4& g, const BwdParams& b, double& sd, double& sq,
                             double& st) {
  float4 r;
  r.x = backward_element<NONLINEAR, DGE>(x.x, g.x, b, sd, sq, st);
  r.y = backward_element<NONLINEAR, DGE>(x.y, g.y, b, sd, sq, st);
  r.z = backward_element<NONLINEAR, DGE>(x.z, g.z, b, sd, sq, st);
  r.w = backward_element<NONLINEAR, DGE>(x.w, g.w, b, sd, sq, st);
  return r;
}

// grad_out and grad_x may be the same buffer: a thread reads its 16 bytes of grad_out before it writes the
// same 16 bytes of grad_x, and no other thread touches them.
template <bool NONLINEAR, bool DGE>
__global__ __launch_bounds__(kThreads) void quant_backward_kernel(
    const float* __restrict__ x, const float* grad_out, int64_t n, int qtype, const float* d, const float* qm,
    const float* t, float clip_lo, float clip_hi, float dge_k, float* grad_x, double* partials) {
  __shared__ double lds[kWaves][3];
  const BwdParams b = load_bwd_params<NONLINEAR>(qtype, d, qm, t, clip_lo, clip_hi, dge_k);
  double sd = 0.0, sq = 0.0, st = 0.0;

  const int64_t nvec = n / kVec;
  const int64_t tid = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const float4* g4 = reinterpret_cast<const float4*>(grad_out);
  float4* o4 = reinterpret_cast<float4*>(grad_x);
  // two 16-byte loads of each stream in flight per lane
  for (int64_t i = tid; i < nvec; i += 2 * stride) {
    const int64_t j = i + stride;
    const bool two = j < nvec;
    const float4 xa = x4[i], ga = g4[i];
    float4 xb = make_float4(0.f, 0.f, 0.f, 0.f), gb = xb;
    if (two) {
      xb = x4[j];
      gb = g4[j];
    }
    o4[i] = backward_vec<NONLINEAR, DGE>(xa, ga, b, sd, sq, st);
    if (two) o4[j] = backward_vec<NONLINEAR, DGE>(xb, gb, b, sd, sq, st);
  }
  // scalar tail: the last n % 4 elements, one per thread of the grid's first threads
  const int64_t e = nvec * kVec + tid;
  if (e < n) grad_x[e] = backward_element<NONLINEAR, DGE>(x[e], grad_out[e], b, sd, sq, st);

  block_sum3(sd, sq, st, lds);
  if (threadIdx.x == 0) store_partial3(partials, sd, sq, st);   // folded by scalar_finish_kernel
}

}  // namespace

extern "C" {

int64_t qvit_quant_backward_workspace_bytes(int64_t n) {
  if (n < 0) return QVIT_EINVAL;
  return (int64_t)stream_grid(n, kVec) * 3 * (int64_t)sizeof(double);
}

int qvit_quant_backward(const float* x, const float* grad_out, int64_t n, int qtype, const float* d_quant,
                        const float* q_m, const float* t_quant, float clip_lo, float clip_hi, float dge_k,
                        float* grad_x, float* grad_scalars, void* workspace, int64_t workspace_bytes,
                        hipStream_t stream) {
  if (!x || !grad_out || !grad_x || !grad_scalars || !d_quant || !q_m || !workspace) return QVIT_ENULL;
  bool nonlinear = false;
  if (qvit_backward_qtype_status(qtype, nonlinear)) return QVIT_EINVAL;
  if (nonlinear && !t_quant) return QVIT_ENULL;
  if (n < 0 || !(dge_k >= 0.f) || (dge_k > 0.f && nonlinear)) return QVIT_EINVAL;
  if (workspace_bytes < qvit_quant_backward_workspace_bytes(n)) return QVIT_EINVAL;
  if (qvit_misaligned(15, x, grad_out, grad_x) || qvit_misaligned(7, workspace)) return QVIT_EALIGN;

  double* partials = static_cast<double*>(workspace);
  int grid = 0;
  if (n > 0) {
    grid = stream_grid(n, kVec);
    const dim3 g(grid), blk(kThreads);
    if (nonlinear)
      hipLaunchKernelGGL((quant_backward_kernel<true, false>), g, blk, 0, stream, x, grad_out, n, qtype, d_quant,
                         q_m, t_quant, clip_lo, clip_hi, dge_k, grad_x, partials);
    else if (dge_k > 0.f)
      hipLaunchKernelGGL((quant_backward_kernel<false, true>), g, blk, 0, stream, x, grad_out, n, qtype, d_quant,
                         q_m, t_quant, clip_lo, clip_hi, dge_k, grad_x, partials);
    else
      hipLaunchKernelGGL((quant_backward_kernel<false, false>), g, blk, 0, stream, x, grad_out, n, qtype,
                         d_quant, q_m, t_quant, clip_lo, clip_hi, dge_k, grad_x, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qvit_hip_status(e);
  }
  hipLaunchKernelGGL(scalar_finish_kernel, dim3(1), dim3(kThreads), 0, stream, partials, grid,
                     grad_scalars);
  return qvit_launch_status();
}

}  // extern "C"
