// The per-element optimizer arithmetic shared by qat_step.hip and prune_step.hip: the hyper-parameters, the
// gradient variant of optimizer/base_optimizer.py:40-86, the descent step of geta.py:571-596, d(b) of
// geta.py:787-804 and the quantizer-scalar descriptor. One definition, so that a member tensor stepped by the
// pruning kernels gets the bits the dense kernel would give it.
#pragma once
#include "reduce_common.h"

namespace {

struct QatQuant {       // 64 B
  float* s[3];          // d_quant, q_m, t_quant (t NULL: the linear type, t = 1)
  const float* g[3];    // their gradients (NULL: that scalar is skipped)
  float* mom;           // float[6]: first moments of d, q_m, t, then the second moments
  int32_t side;         // 0: weight, 1: activation
  int32_t flags;        // bits 0..2: first step of d, q_m, t
};

struct Hyper {
  int variant, first_step;
  float lr, lr_quant;
  float mom1, mom2;       // first_momentum, second_momentum
  float alpha1, alpha2;   // 1 - dampening of the two moment updates, rounded from double on the host
  float wd;               // 0: none
  float bc1, bc2;         // 1 - mom^step
  float clip_lo, clip_hi;
};

// grad_variant of one element (base_optimizer.py:40-86); m, v are read unless `fresh` and left updated.
template <int VARIANT>
QVIT_DEV float grad_variant(float p, float g, float& m, float& v, bool fresh, const Hyper& h) {
#pragma clang fp contract(off)
  g = g < h.clip_lo ? h.clip_lo : (g > h.clip_hi ? h.clip_hi : g);   // geta.py:160-165; a NaN stays
  if (VARIANT != QVIT_QAT_ADAMW && h.wd != 0.f) g = g + h.wd * p;     // :54-55
  if (h.mom1 > 0.f) m = fresh ? g : fmaf(g, h.alpha1, m * h.mom1);    // :18-27
  else m = g;
  if (VARIANT == QVIT_QAT_SGD) return m;
  const float gg = g * g;
  if (h.mom2 > 0.f) v = fresh ? gg : fmaf(gg, h.alpha2, v * h.mom2);  // :29-38
  else v = gg;
  return (m / h.bc1) / (sqrtf(v / h.bc2) + 1e-8f);                    // :79-86
}

// one gradient step of geta.py:571-596 at the rate lr: adamw's decoupled decay, then p -= lr * grad_variant
template <int VARIANT>
QVIT_DEV float descend(float p, float gv, float lr, const Hyper& h) {
#pragma clang fp contract(off)
  if (VARIANT == QVIT_QAT_ADAMW && h.wd != 0.f) p = fmaf(h.wd * p, -lr, p);
  return fmaf(gv, -lr, p);
}

template <int VARIANT>
QVIT_DEV float step_element(float p, float g, float& m, float& v, bool fresh, float lr, const Hyper& h) {
  return descend<VARIANT>(p, grad_variant<VARIANT>(p, g, m, v, fresh, h), lr, h);
}

// d(b) of geta.py:787-804 in double, as the reference evaluates it with Python floats
QVIT_DEV double d_of_bits(int b, double qm, double t) {
  const double q = fmax(fabs(qm), 1e-10);
  return exp(t * log(q)) / (exp2((double)(b - 1)) - 1.0);
}

// torch.clamp(d, lo, hi) with the bounds rounded to fp32; a NaN d stays
QVIT_DEV float clamp_keep_nan(float d, float lo, float hi) {
  return d != d ? d : fminf(fmaxf(d, lo), hi);
}

// the checks both entry points share behind their pointer and count rules
inline int variant_status(int variant) {
  return (variant == QVIT_QAT_SGD || variant == QVIT_QAT_ADAM || variant == QVIT_QAT_ADAMW) ? QVIT_OK : QVIT_EINVAL;
}

inline Hyper make_hyper(int variant, int first_step, float lr, float lr_quant, float mom1, float mom2, float alpha1,
                        float alpha2, float wd, float bc1, float bc2, float clip_lo, float clip_hi) {
  Hyper h;
  h.variant = variant; h.first_step = first_step; h.lr = lr; h.lr_quant = lr_quant; h.mom1 = mom1; h.mom2 = mom2;
  h.alpha1 = alpha1; h.alpha2 = alpha2; h.wd = wd; h.bc1 = bc1; h.bc2 = bc2; h.clip_lo = clip_lo; h.clip_hi = clip_hi;
  return h;
}

}  // namespace
