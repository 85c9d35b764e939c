// The quantization-aware stages of the GETA optimizer as two launches per step (optimizer/geta.py:571-804 and
// :873-943 with pruning absent; the gradient variant of optimizer/base_optimizer.py:40-86):
//   qvit_qat_step        every dense tensor (weights, biases, LayerNorm, cls_token, pos_embed) from one launch;
//   qvit_qat_quant_step  every quantizer scalar (d_quant, q_m, t_quant per layer and side) plus the stage's
//                        projection of d_quant, one thread per (layer, side).
// Neither reads anything back: the reference's projections fetch q_m and t_quant with .item() per layer, side and
// step; here the thread that updated them projects d with them.
//
// Dense kernel. The host keeps a table of QatTensor descriptors in device memory and a list of QatChunk = (tensor,
// chunk within the tensor); a chunk is kChunk = 4096 consecutive elements (256 threads x 4 x one 16-byte access).
// Workgroups stride over the chunk list, so a 2.4 M-element fc1 weight and a 768-element bias spread over the same
// grid (stream_grid: at most kGridCap workgroups). A chunk starts a multiple of 16 KiB into its tensor, so whether
// the 16-byte path applies is a property of the tensor's four base pointers: all 16-byte aligned -> float4 for
// len / 4 * 4 elements and a scalar tail (only a tensor's last chunk has one); any pointer off 16 bytes (a view 4
// bytes into a storage) -> the scalar path for that tensor. Both paths run the same per-element function, so the
// bits do not depend on the path. Parameters stay where they are: nothing is flattened or copied.
//
// Arithmetic: fp32, one IEEE operation per reference operation, in the reference's order. torch's CPU
// `a.add_(b, alpha=s)` is fmadd(b, s, a) in its vector loop, so those steps are fmaf here; everything else is kept
// apart by `fp contract(off)`. Division and sqrt are the correctly rounded ones (the build's
// -fhip-fp32-correctly-rounded-divide-sqrt). Traffic per element: p read and written, grad read, each moment read
// and written: 28 B (adam, adamw), 20 B (sgd with momentum), 12 B (plain sgd); no reuse, so HBM bounds the kernel.
#include "qat_common.h"

namespace {

constexpr int kChunk = kThreads * kVec * 4;   // elements per chunk
constexpr int64_t kMaxChunks = (int64_t)1 << 40;

// layouts shared with the host (qat_optim.py fills them as int64 rows)
struct QatTensor {      // 48 B
  float* p;
  const float* grad;    // NULL: the tensor is skipped, its moments stay untouched (base_optimizer.py:51)
  float* m;             // first moment, NULL when the variant keeps none
  float* v;             // second moment, NULL when the variant keeps none
  int64_t numel;
  int32_t lr_class;     // 0: lr, 1: lr_quant
  int32_t flags;        // bit 0: this tensor's first step (its moments become grad and grad^2)
};
struct QatChunk {       // 8 B
  int32_t tensor;
  int32_t index;        // elements [index * kChunk, min(numel, (index + 1) * kChunk))
};

template <int VARIANT>
__global__ __launch_bounds__(kThreads) void qat_dense_kernel(const QatTensor* __restrict__ tensors, int ntensors,
                                                             const QatChunk* __restrict__ chunks, int64_t nchunks,
                                                             Hyper h) {
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const QatChunk ch = chunks[c];
    if ((uint32_t)ch.tensor >= (uint32_t)ntensors || ch.index < 0) continue;
    const QatTensor t = tensors[ch.tensor];
    const int64_t off = (int64_t)ch.index * kChunk;
    if (!t.p || !t.grad || off >= t.numel) continue;
    const int len = t.numel - off < kChunk ? (int)(t.numel - off) : kChunk;
    float* __restrict__ p = t.p + off;
    const float* __restrict__ g = t.grad + off;
    float* __restrict__ m = (t.m && h.mom1 > 0.f) ? t.m + off : nullptr;
    float* __restrict__ v = (t.v && VARIANT != QVIT_QAT_SGD && h.mom2 > 0.f) ? t.v + off : nullptr;
    const bool fresh = h.first_step || (t.flags & 1);
    const float lr = t.lr_class ? h.lr_quant : h.lr;
    const bool vec = (((uintptr_t)t.p | (uintptr_t)t.grad | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0;
    const int nv = vec ? len / kVec : 0;
    for (int i = threadIdx.x; i < nv; i += kThreads) {
      float4 p4 = reinterpret_cast<const float4*>(p)[i];
      const float4 g4 = reinterpret_cast<const float4*>(g)[i];
      float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = m4;
      if (m && !fresh) m4 = reinterpret_cast<const float4*>(m)[i];
      if (v && !fresh) v4 = reinterpret_cast<const float4*>(v)[i];
      p4.x = step_element<VARIANT>(p4.x, g4.x, m4.x, v4.x, fresh, lr, h);
      p4.y = step_element<VARIANT>(p4.y, g4.y, m4.y, v4.y, fresh, lr, h);
      p4.z = step_element<VARIANT>(p4.z, g4.z, m4.z, v4.z, fresh, lr, h);
      p4.w = step_element<VARIANT>(p4.w, g4.w, m4.w, v4.w, fresh, lr, h);
      reinterpret_cast<float4*>(p)[i] = p4;
      if (m) reinterpret_cast<float4*>(m)[i] = m4;
      if (v) reinterpret_cast<float4*>(v)[i] = v4;
    }
    for (int i = nv * kVec + threadIdx.x; i < len; i += kThreads) {
      float mi = 0.f, vi = 0.f;
      if (m && !fresh) mi = m[i];
      if (v && !fresh) vi = v[i];
      p[i] = step_element<VARIANT>(p[i], g[i], mi, vi, fresh, lr, h);
      if (m) m[i] = mi;
      if (v) v[i] = vi;
    }
  }
}

template <int VARIANT>
__global__ __launch_bounds__(kThreads) void qat_quant_kernel(const QatQuant* __restrict__ quants, int nquants,
                                                             int32_t* __restrict__ bits, int stage, int first_fix,
                                                             Hyper h, int min_wt, int max_wt, int min_act,
                                                             int max_act) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= nquants) return;
  const QatQuant e = quants[i];
  if (!e.s[0] || !e.s[1] || !e.mom) return;
  // the fixed bit width comes from the scalars as the step finds them (get_bitwidth_dict runs before the update,
  // geta.py:932-940); rint: half to even, Python's round
  if (stage == QVIT_QAT_FIX && first_fix) {
    const double d0 = (double)*e.s[0], q0 = (double)*e.s[1], t0 = e.s[2] ? (double)*e.s[2] : 1.0;
    double b = rint(log2(exp(t0 * log(fabs(q0))) / fabs(d0) + 1.0) + 1.0);
    b = b >= 0.0 ? (b <= 64.0 ? b : 64.0) : 0.0;   // (a NaN gives 0)
    bits[i] = (int32_t)b;
  }
  // In the range stage the weight pass steps everything that is no weight-side scalar at lr, the activation
  // scalars among it, and the activation pass then steps those again at lr_quant from the same grad_variant
  // (geta.py:598-630, :667-697). Kept as it is: the trained scalars are the product's input.
  const bool twice = stage == QVIT_QAT_RANGE && e.side == 1;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    if (!e.s[s] || !e.g[s]) continue;
    const bool fresh = h.first_step || ((e.flags >> s) & 1);
    float m = 0.f, v = 0.f;
    if (!fresh) {
      m = e.mom[s];
      v = e.mom[3 + s];
    }
    float p = *e.s[s];
    const float gv = grad_variant<VARIANT>(p, *e.g[s], m, v, fresh, h);
    if (twice) p = descend<VARIANT>(p, gv, h.lr, h);
    p = descend<VARIANT>(p, gv, h.lr_quant, h);
    *e.s[s] = p;
    e.mom[s] = m;
    e.mom[3 + s] = v;
  }
  if (stage == QVIT_QAT_WARMUP) return;
  const double qm = (double)*e.s[1], t = e.s[2] ? (double)*e.s[2] : 1.0;
  const float d = *e.s[0];
  if (stage == QVIT_QAT_RANGE) {
    const float lo = (float)d_of_bits(e.side ? max_act : max_wt, qm, t);
    const float hi = (float)d_of_bits(e.side ? min_act : min_wt, qm, t);
    *e.s[0] = clamp_keep_nan(d, lo, hi);
  } else {
    const float fix = (float)d_of_bits(bits[i], qm, t);
    *e.s[0] = clamp_keep_nan(d, fix, fix);
  }
}

}  // namespace

extern "C" {

int qvit_qat_step(const void* tensors, int ntensors, const void* chunks, int64_t nchunks, int variant,
                  int first_step, float lr, float lr_quant, float first_momentum, float second_momentum,
                  float alpha1, float alpha2, float weight_decay, float bias_correction1, float bias_correction2,
                  float clip_lo, float clip_hi, hipStream_t stream) {
  if (!tensors || !chunks) return QVIT_ENULL;
  if (qvit_misaligned(7, tensors, chunks)) return QVIT_EALIGN;
  if (ntensors < 0 || nchunks < 0 || nchunks > kMaxChunks) return QVIT_EINVAL;
  if (variant_status(variant)) return QVIT_EINVAL;
  if (ntensors == 0 || nchunks == 0) return QVIT_OK;
  const Hyper h = make_hyper(variant, first_step, lr, lr_quant, first_momentum, second_momentum, alpha1, alpha2,
                             weight_decay, bias_correction1, bias_correction2, clip_lo, clip_hi);
  const dim3 grid(stream_grid(nchunks * kChunk, kChunk / kThreads));   // a workgroup per chunk up to kGridCap
  const QatTensor* tt = static_cast<const QatTensor*>(tensors);
  const QatChunk* cc = static_cast<const QatChunk*>(chunks);
  if (variant == QVIT_QAT_SGD)
    hipLaunchKernelGGL(qat_dense_kernel<QVIT_QAT_SGD>, grid, dim3(kThreads), 0, stream, tt, ntensors, cc, nchunks, h);
  else if (variant == QVIT_QAT_ADAM)
    hipLaunchKernelGGL(qat_dense_kernel<QVIT_QAT_ADAM>, grid, dim3(kThreads), 0, stream, tt, ntensors, cc, nchunks, h);
  else
    hipLaunchKernelGGL(qat_dense_kernel<QVIT_QAT_ADAMW>, grid, dim3(kThreads), 0, stream, tt, ntensors, cc, nchunks,
                       h);
  return qvit_launch_status();
}

int qvit_qat_quant_step(const void* quants, int nquants, int32_t* bits, int stage, int first_fix, int variant,
                        int first_step, float lr, float lr_quant, float first_momentum, float second_momentum,
                        float alpha1, float alpha2, float weight_decay, float bias_correction1,
                        float bias_correction2, float clip_lo, float clip_hi, int min_bit_wt, int max_bit_wt,
                        int min_bit_act, int max_bit_act, hipStream_t stream) {
  if (!quants || !bits) return QVIT_ENULL;
  if (qvit_misaligned(7, quants) || qvit_misaligned(3, bits)) return QVIT_EALIGN;
  if (nquants < 0) return QVIT_EINVAL;
  if (variant_status(variant)) return QVIT_EINVAL;
  if (stage != QVIT_QAT_WARMUP && stage != QVIT_QAT_RANGE && stage != QVIT_QAT_FIX) return QVIT_EINVAL;
  // a bit range d(b) is defined on: 2 <= min <= max <= 32 (2^(b-1) - 1 > 0)
  if (min_bit_wt < 2 || max_bit_wt < min_bit_wt || max_bit_wt > 32 || min_bit_act < 2 || max_bit_act < min_bit_act ||
      max_bit_act > 32)
    return QVIT_EINVAL;
  if (nquants == 0) return QVIT_OK;
  const Hyper h = make_hyper(variant, first_step, lr, lr_quant, first_momentum, second_momentum, alpha1, alpha2,
                             weight_decay, bias_correction1, bias_correction2, clip_lo, clip_hi);
  const dim3 grid((unsigned)cdiv(nquants, kThreads));
  const QatQuant* qq = static_cast<const QatQuant*>(quants);
#define QVIT_QQ(V)                                                                                                  \
  hipLaunchKernelGGL(qat_quant_kernel<V>, grid, dim3(kThreads), 0, stream, qq, nquants, bits, stage, first_fix, h, \
                     min_bit_wt, max_bit_wt, min_bit_act, max_bit_act)
  if (variant == QVIT_QAT_SGD) QVIT_QQ(QVIT_QAT_SGD);
  else if (variant == QVIT_QAT_ADAM) QVIT_QQ(QVIT_QAT_ADAM);
  else QVIT_QQ(QVIT_QAT_ADAMW);
#undef QVIT_QQ
  return qvit_launch_status();
}

}  // extern "C"
