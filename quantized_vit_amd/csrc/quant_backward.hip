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
#include "qvit_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGridCap = 1024;   // 4 blocks per CU; a grid-stride loop covers the rest
constexpr int kVec = 4;          // floats per 16-byte access

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline int backward_grid(int64_t n) {
  const int64_t g = cdiv(n / kVec, kThreads);
  return (int)(g < 1 ? 1 : (g < kGridCap ? g : kGridCap));
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
  if (threadIdx.x == 0) {
    double* out = partials + (int64_t)blockIdx.x * 3;
    out[0] = sd; out[1] = sq; out[2] = st;
  }
}

// Second stage, one block: thread i adds the partials of blocks i, i + 256, ... in that order, then the block
// reduces as above. nblocks == 0 writes three zeros.
__global__ __launch_bounds__(kThreads) void quant_backward_finish_kernel(const double* partials, int nblocks,
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

extern "C" {

int64_t qvit_quant_backward_workspace_bytes(int64_t n) {
  if (n < 0) return QVIT_EINVAL;
  return (int64_t)backward_grid(n) * 3 * (int64_t)sizeof(double);
}

int qvit_quant_backward(const float* x, const float* grad_out, int64_t n, int qtype, const float* d_quant,
                        const float* q_m, const float* t_quant, float clip_lo, float clip_hi, float dge_k,
                        float* grad_x, float* grad_scalars, void* workspace, int64_t workspace_bytes,
                        hipStream_t stream) {
  if (!x || !grad_out || !grad_x || !grad_scalars || !d_quant || !q_m || !workspace) return QVIT_ENULL;
  const int qt = qtype & 0xff;
  if ((qtype & ~(0xff | QVIT_QT_FORCE_CAREFUL)) != 0 || (qt != QVIT_QT_LINEAR && qt != QVIT_QT_NONLINEAR))
    return QVIT_EINVAL;
  const bool nonlinear = qt == QVIT_QT_NONLINEAR;
  if (nonlinear && !t_quant) return QVIT_ENULL;
  if (n < 0 || !(dge_k >= 0.f) || (dge_k > 0.f && nonlinear)) return QVIT_EINVAL;
  if (workspace_bytes < qvit_quant_backward_workspace_bytes(n)) return QVIT_EINVAL;
  if ((((uintptr_t)x) | ((uintptr_t)grad_out) | ((uintptr_t)grad_x)) & 15) return QVIT_EALIGN;
  if ((uintptr_t)workspace & 7) return QVIT_EALIGN;

  double* partials = static_cast<double*>(workspace);
  int grid = 0;
  if (n > 0) {
    grid = backward_grid(n);
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
  hipLaunchKernelGGL(quant_backward_finish_kernel, dim3(1), dim3(kThreads), 0, stream, partials, grid,
                     grad_scalars);
  return qvit_hip_status(hipGetLastError());
}

}  // extern "C"
