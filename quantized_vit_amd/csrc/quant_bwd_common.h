// Device code of the quantizer backward shared by quant_backward.hip (qvit_quant_backward) and train_fuse.hip
// (the same backward behind a recomputed LayerNorm or GELU): the per-call uniforms and one element's terms; the
// fixed-order sums they leave through are reduce_common.h's. See quant_backward.hip for the table of regions and the
// mask rules.
#pragma once
#include "reduce_common.h"

namespace {

// The wave-uniform values of one call.
struct BwdParams {
  QParams q;
  float sat_q;     // range_pow / d (:91-92, :179-180)
  float sat_t;     // range_pow * ln(|q_m| + 1e-6) (:102)
  float qm_coef;   // 1 (:185) or t * range_pow_low (:84-86, :97)
  float clip_lo, clip_hi;
  float dge_inv_k, dge_exp, dge_half_d;   // 1/k, 1/k - 1, d/2 (:260-261)
};

template <bool NONLINEAR>
QVIT_DEV BwdParams load_bwd_params(int qtype, const float* d, const float* qm, const float* t, float clip_lo,
                                   float clip_hi, float dge_k) {
  BwdParams b;
  b.q = load_qparams(qtype, d, qm, t, 0);
  b.q.qtype = NONLINEAR ? QVIT_QT_NONLINEAR : QVIT_QT_LINEAR;   // a compile-time constant for quant_code
  if (NONLINEAR) {
    const float lq = log_cr(fabsf(b.q.qm) + 1e-6f);
    const float range_pow = exp_cr(b.q.t * lq);
    b.sat_q = range_pow / b.q.d;
    b.sat_t = range_pow * lq;
    b.qm_coef = b.q.t * exp_cr((b.q.t - 1.f) * lq);
  } else {
    b.sat_q = fabsf(b.q.qm) / b.q.d;
    b.sat_t = 0.f;
    b.qm_coef = 1.f;
  }
  b.clip_lo = clip_lo;
  b.clip_hi = clip_hi;
  b.dge_inv_k = (dge_k > 0.f) ? 1.f / dge_k : 0.f;
  b.dge_exp = b.dge_inv_k - 1.f;
  b.dge_half_d = b.q.d / 2.f;
  return b;
}

// One element: returns grad_x and adds grad_out * term into the three sums.
template <bool NONLINEAR, bool DGE>
QVIT_DEV float backward_element(float x, float g, const BwdParams& b, double& sd, double& sq, double& st) {
  const QParams& p = b.q;
  const float a = fabsf(x);
  const float sgn = (float)(x > 0.f) - (float)(x < 0.f);   // torch.sign: 0 at 0 and at NaN
  const bool zero = a <= 0.f;                              // input_abs <= q_s
  const bool sat = a >= p.qm;                              // input_abs >= q_m
  const float k = quant_code(x, p);                        // sgn * rne(q) / sgn * L / 0: the forward's code

  // p(a) and ln a. Nonlinear: the hardware log2 / exp2 (a few ulp, scaled by |t log2 a| in the power); inputs
  // it would flush to zero take the forward's careful sequence instead.
  float pw = a, ln_a = 0.f;
  if (NONLINEAR) {
    if (a > 1e-30f || zero) {   // at a == 0 both forms give p = 0 and a masked ln a
      const float l2 = __builtin_amdgcn_logf(a);
      pw = __builtin_amdgcn_exp2f(p.t * l2);
      ln_a = l2 * 0.6931471805599453f;
    } else {
      ln_a = log_cr(a);
      pw = exp_cr(p.t * ln_a);
    }
  }
  const float q = pw / p.d;   // IEEE division (-fhip-fp32-correctly-rounded-divide-sqrt)

  // sgn * (rne(q) - q) == k - sgn * q: negation is exact, so both round once
  const float term_d = k - sgn * (zero ? 0.f : (sat ? b.sat_q : q));
  const float term_q = (a <= p.qm) ? 0.f : sgn * b.qm_coef;
  sd += (double)(g * term_d);
  sq += (double)(g * term_q);
  if (NONLINEAR) {
    const float term_t = sgn * (zero ? 0.f : (sat ? b.sat_t : pw * ln_a));
    st += (double)(g * term_t);
  }

  float gx = (x >= b.clip_hi || x <= b.clip_lo) ? 0.f : g;   // :77-79
  if (DGE) {
    gx = gx * (b.dge_inv_k * powf(fabsf(x - b.dge_half_d), b.dge_exp));   // :260-262
    gx = (gx < -3.f) ? -3.f : ((gx > 3.f) ? 3.f : gx);                    // :265, NaN passes through
  }
  return gx;
}

// The three scalar gradients (d_quant, q_m, t_quant) of a quantizer backward from its nblocks x 3 partials, one
// block: thread i adds the partials of blocks i, i + 256, ... in that order, then the block reduces as block_sum3.
// nblocks == 0 writes three zeros.
__global__ __launch_bounds__(kThreads) void scalar_finish_kernel(const double* partials, int nblocks,
                                                                 float* grad_scalars) {
  __shared__ double lds[kWaves][3];
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
}

}  // namespace
