// Input gradient of QuantizeConv2d behind its im2col lowering (libqvit_hip.so, gfx950): col2im of the patch-row
// gradient P = G2 @ (d_wt k_w) and the activation quantizer's backward in one pass over the NCHW image.
//
//   grad_xq[b][c][y][x] = sum over ky ascending, inside it kx ascending, of P[(b OH + oy) OW + ox][(c kh + ky) kw + kx]
//                         for the taps with (y + ph - ky dh) % sh == 0, oy = (y + ph - ky dh) / sh in [0, OH)
//                         and (x + pw - kx dw) % sw == 0, ox = (x + pw - kx dw) / sw in [0, OW).
//
// A gather: every image element sums its own taps in that fixed order in fp32 from 0.f (no atomics, two calls give
// the same bits); an element no output position reads sums nothing and is exactly 0; a zero-padding tap has no image
// element and so contributes nowhere. The element then goes through backward_element (quant_bwd_common.h) exactly as
// qvit_quant_backward applies it to (x, grad_xq), and the three sums leave through the same two-stage reduction.
// With x == NULL (fold only) grad_xq itself is written and nothing is reduced.
//
// Two arms, identical bits where both apply:
//   vec    : one thread per aligned group of four consecutive x. Taken when pw == 0, dw == 1, kw % 4 == 0,
//            sw % 4 == 0 and sw >= kw (no two kernel columns reach the same x, so x has the single tap
//            ox = x / sw, kx = x % sw when kx < kw), W % 4 == 0, ldp % 4 == 0 and P, x, grad_x 16-byte aligned: the
//            group reads one 16-byte chunk of one row of P per ky tap. The patch embedding (k == s, p == 0) is here.
//   scalar : one thread per element, any geometry and any 4-byte alignment.
// I is the type of the flat offsets into P and the image (int while M ldp and B C H W are below 2^31); coordinates
// are ints in both (the host bounds them).
#include "quant_bwd_common.h"

namespace {

struct FoldGeo {
  int C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, OH, OW;
};

enum FoldMode { kFoldOnly = 0, kFoldLinear = 1, kFoldNonlinear = 2 };

// (ky, oy) taps of image row y in ascending ky: calls f(ky, oy)
template <typename F>
QVIT_DEV void for_row_taps(const FoldGeo& g, int y, F f) {
  const int ty = y + g.ph;
  for (int ky = 0; ky < g.kh; ++ky) {
    const int ry = ty - ky * g.dh;
    if (ry < 0) break;   // ry only falls from here on
    const int oy = ry / g.sh;
    if (oy * g.sh == ry && oy < g.OH) f(ky, oy);
  }
}

template <typename I>
QVIT_DEV float fold_element(const float* __restrict__ P, I ldp, const FoldGeo& g, I img_row0, int c, int y, int x) {
  float acc = 0.f;
  const int tx = x + g.pw;
  for_row_taps(g, y, [&](int ky, int oy) {
    const float* prow = P + (img_row0 + (I)oy * g.OW) * ldp + (c * g.kh + ky) * g.kw;
    for (int kx = 0; kx < g.kw; ++kx) {
      const int rx = tx - kx * g.dw;
      if (rx < 0) break;
      const int ox = rx / g.sw;
      if (ox * g.sw == rx && ox < g.OW) acc += prow[(I)ox * ldp + kx];
    }
  });
  return acc;
}

// the four elements x0 .. x0 + 3 (x0 % 4 == 0) of one image row on the vec arm's geometry
template <typename I>
QVIT_DEV float4 fold_vec(const float* __restrict__ P, I ldp, const FoldGeo& g, I img_row0, int c, int y, int x0) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int ox = x0 / g.sw, kx0 = x0 - ox * g.sw;
  if (kx0 >= g.kw || ox >= g.OW) return acc;
  for_row_taps(g, y, [&](int ky, int oy) {
    const float4 v = *reinterpret_cast<const float4*>(P + (img_row0 + (I)oy * g.OW + ox) * ldp +
                                                      (c * g.kh + ky) * g.kw + kx0);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  });
  return acc;
}

template <int MODE>
QVIT_DEV float finish_element(float x, float gq, const BwdParams& b, double& sd, double& sq, double& st) {
  if (MODE == kFoldOnly) return gq;
  return backward_element<MODE == kFoldNonlinear, false>(x, gq, b, sd, sq, st);
}

// `total` work items (groups of four on the vec arm, elements on the scalar one), grid-stride
template <typename I, int MODE, bool VEC>
__global__ __launch_bounds__(kThreads) void col2im_quant_backward_kernel(
    const float* __restrict__ P, int64_t ldp_, const float* __restrict__ x, FoldGeo g, int64_t total, int qtype,
    const float* d, const float* qm, const float* t, float clip_lo, float clip_hi, float* __restrict__ grad_x,
    double* partials) {
  __shared__ double lds[kWaves][3];
  BwdParams b;
  if (MODE != kFoldOnly) b = load_bwd_params<MODE == kFoldNonlinear>(qtype, d, qm, t, clip_lo, clip_hi, 0.f);
  double sd = 0.0, sq = 0.0, st = 0.0;
  const I ldp = (I)ldp_;
  const int wq = VEC ? g.W / kVec : g.W;   // work items per image row
  const I rows_per_img = (I)g.OH * g.OW;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < total; i += stride) {
    const I e = (I)i;
    const I r = e / wq;                    // image row (b, c, y)
    const int xi = (int)(e - r * wq);
    const I bc = r / g.H;
    const int y = (int)(r - bc * g.H);
    const I bi = bc / g.C;
    const int c = (int)(bc - bi * g.C);
    const I img_row0 = bi * rows_per_img;
    if (VEC) {
      float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (MODE != kFoldOnly) xv = reinterpret_cast<const float4*>(x)[e];
      const float4 gq = fold_vec<I>(P, ldp, g, img_row0, c, y, xi * kVec);
      float4 o;
      o.x = finish_element<MODE>(xv.x, gq.x, b, sd, sq, st);
      o.y = finish_element<MODE>(xv.y, gq.y, b, sd, sq, st);
      o.z = finish_element<MODE>(xv.z, gq.z, b, sd, sq, st);
      o.w = finish_element<MODE>(xv.w, gq.w, b, sd, sq, st);
      reinterpret_cast<float4*>(grad_x)[e] = o;
    } else {
      const float xv = (MODE != kFoldOnly) ? x[e] : 0.f;
      const float gq = fold_element<I>(P, ldp, g, img_row0, c, y, xi);
      grad_x[e] = finish_element<MODE>(xv, gq, b, sd, sq, st);
    }
  }
  if (MODE != kFoldOnly) {
    block_sum3(sd, sq, st, lds);
    if (threadIdx.x == 0) store_partial3(partials, sd, sq, st);   // folded by scalar_finish_kernel
  }
}

// n = B C H W, the image elements; false: a size the kernel does not take
bool col2im_geo(int64_t B, int64_t C, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                int dw, FoldGeo* geo, ConvShape* cs, int64_t* n) {
  // (the upper bounds first: they bound what qvit_conv_shape and the products below multiply; a size below its range
  // passes them and fails in qvit_conv_shape)
  const int64_t lim = 1 << 20, ext = 1 << 16, tot = (int64_t)1 << 40;
  if (B > lim || C > lim || H > ext || W > ext || kh > 1024 || kw > 1024 || sh > ext || sw > ext || ph > ext ||
      pw > ext || dh > 1024 || dw > 1024)
    return false;
  if (qvit_conv_shape(B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, *cs)) return false;
  if (C * H * W >= tot || B * (C * H * W) >= tot || cs->K > ((int64_t)1 << 24) || cs->M >= tot) return false;
  *n = B * C * H * W;
  *geo = FoldGeo{(int)C, (int)H, (int)W, kh, kw, sh, sw, ph, pw, dh, dw, (int)cs->OH, (int)cs->OW};
  return true;
}

template <typename I, int MODE>
void launch_fold(bool vec, int grid, hipStream_t stream, const float* P, int64_t ldp, const float* x,
                 const FoldGeo& g, int64_t total, int qtype, const float* d, const float* qm, const float* t,
                 float clip_lo, float clip_hi, float* grad_x, double* partials) {
  if (vec)
    hipLaunchKernelGGL((col2im_quant_backward_kernel<I, MODE, true>), dim3(grid), dim3(kThreads), 0, stream, P, ldp,
                       x, g, total, qtype, d, qm, t, clip_lo, clip_hi, grad_x, partials);
  else
    hipLaunchKernelGGL((col2im_quant_backward_kernel<I, MODE, false>), dim3(grid), dim3(kThreads), 0, stream, P, ldp,
                       x, g, total, qtype, d, qm, t, clip_lo, clip_hi, grad_x, partials);
}

}  // namespace

extern "C" {

int64_t qvit_col2im_quant_backward_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int kh, int kw,
                                                   int sh, int sw, int ph, int pw, int dh, int dw) {
  FoldGeo g;
  ConvShape cs;
  int64_t n = 0;
  if (!col2im_geo(B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &cs, &n)) return QVIT_EINVAL;
  return (int64_t)stream_grid(n, 1) * 3 * (int64_t)sizeof(double);   // the scalar arm's grid: never below the vec arm's
}

int qvit_col2im_quant_backward(const float* P, int64_t ldp, const float* x, int64_t B, int64_t C, int64_t H,
                               int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int qtype,
                               const float* d_quant, const float* q_m, const float* t_quant, float clip_lo,
                               float clip_hi, float* grad_x, float* grad_scalars, void* workspace,
                               int64_t workspace_bytes, hipStream_t stream) {
  const bool fused = x != nullptr;
  if (!P || !grad_x) return QVIT_ENULL;
  if (fused && (!grad_scalars || !d_quant || !q_m || !workspace)) return QVIT_ENULL;
  bool nonlinear = false;
  if (fused) {
    if (qvit_backward_qtype_status(qtype, nonlinear)) return QVIT_EINVAL;
    if (nonlinear && !t_quant) return QVIT_ENULL;
  }
  FoldGeo g;
  ConvShape cs;
  int64_t n = 0;
  if (!col2im_geo(B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, &g, &cs, &n)) return QVIT_EINVAL;
  const int64_t tot = (int64_t)1 << 40;
  if (ldp < cs.K || ldp > ((int64_t)1 << 24) || cs.M * ldp >= tot) return QVIT_EINVAL;
  if (fused && workspace_bytes < (int64_t)stream_grid(n, 1) * 3 * (int64_t)sizeof(double)) return QVIT_EINVAL;
  if (qvit_misaligned(3, P, x, grad_x) || (fused && qvit_misaligned(7, workspace))) return QVIT_EALIGN;

  if (n == 0 && !fused) return QVIT_OK;

  double* partials = static_cast<double*>(workspace);
  int grid = 0;
  if (n > 0) {
    const bool vec = pw == 0 && dw == 1 && kw % kVec == 0 && sw % kVec == 0 && sw >= kw && W % kVec == 0 &&
                     ldp % kVec == 0 && !qvit_misaligned(15, P, x, grad_x);
    const int64_t total = vec ? n / kVec : n;
    grid = stream_grid(n, vec ? kVec : 1);
    const int64_t lim32 = (int64_t)1 << 31;
    const bool narrow = cs.M * ldp < lim32 && n < lim32;
    const int mode = !fused ? kFoldOnly : (nonlinear ? kFoldNonlinear : kFoldLinear);
#define QVIT_FOLD_LAUNCH(I, MODE) \
  launch_fold<I, MODE>(vec, grid, stream, P, ldp, x, g, total, qtype, d_quant, q_m, t_quant, clip_lo, clip_hi, \
                       grad_x, partials)
    if (narrow) {
      if (mode == kFoldOnly) QVIT_FOLD_LAUNCH(int, kFoldOnly);
      else if (mode == kFoldLinear) QVIT_FOLD_LAUNCH(int, kFoldLinear);
      else QVIT_FOLD_LAUNCH(int, kFoldNonlinear);
    } else {
      if (mode == kFoldOnly) QVIT_FOLD_LAUNCH(int64_t, kFoldOnly);
      else if (mode == kFoldLinear) QVIT_FOLD_LAUNCH(int64_t, kFoldLinear);
      else QVIT_FOLD_LAUNCH(int64_t, kFoldNonlinear);
    }
#undef QVIT_FOLD_LAUNCH
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qvit_hip_status(e);
  }
  if (fused)
    hipLaunchKernelGGL(scalar_finish_kernel, dim3(1), dim3(kThreads), 0, stream, partials, grid, grad_scalars);
  return qvit_launch_status();
}

}  // extern "C"
