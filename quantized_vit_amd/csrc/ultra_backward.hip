// UltraNet training: the straight-through backward of the reference's `4-bit quantization/quant_ultra.py`
// quantizers (uniform_quantize.backward :23-25 passes the gradient through the rounding) and the weight gradient
// of Conv2d_Q (:85-89) against the activation quantizer's integer codes.
//
// qvit_ultra_weight_quant_backward  weight_quantize_fn (:50-55): t = tanh(w), m = max|t|, u = t / m, w_q = ste(u).
//     g_u = g;  g_t = g / m - sgn(t) [|t| == m] S / (m^2 c),  S = sum_i g_i t_i,  c = #{i : |t_i| == m}
//     (torch's full-reduction max hands its gradient to the tied elements in equal shares);  g_w = g_t (1 - t^2).
//   t and m are ultra_quant_common.h's, the forward's routines: the tie set is the one the forward saw. S and c
//   leave the streaming pass through reduce_common.h's scheme: per-thread double accumulation, the fixed-order
//   wave / block tree, one partial pair per block in the caller's workspace, a one-block fold in index order. No
//   float atomics: two calls give the same bits. Masks select, they never multiply: a NaN in g_i is in g_w[i] and,
//   through S, in every tied element; a NaN w_i is in g_w[i] (and in S).
// qvit_ultra_act_quant_backward  activation_quantize_fn (:71): g_x = g where 0 <= x <= 1, else 0 (torch's clamp
//   mask: both boundaries pass, a NaN x gives 0). One streaming pass, 16 B per lane, scalar tail; g_x may be g.
// qvit_conv_wgrad  dWq[n][c][ky][kx] = (1 / levels) sum_{b,oy,ox} G[b][n][oy][ox] k_x[b][c][iy][ix],
//   iy = oy sh - ph + ky dh, ix = ox sw - pw + kx dw, k_x = rint(X levels) the codes of X = k / levels (the
//   output of activation_quantize_fn, max-pooled or not), out-of-image taps zero.
//   Arithmetic (bf16x3.h): G = g1 + g2 + g3 exactly, three truncated bf16 terms; a code (<= 127) is a bf16
//   exactly; every product is exact in fp32 and v_mfma_f32_16x16x32_bf16 accumulates in fp32; one multiply by
//   1 / levels ends it. A NaN / inf in G[b][n][.][.] makes row n of dWq NaN (NaN times a zero code is NaN) and no
//   other row.
//   Geometry: an implicit GEMM with the contraction index m = (b, oy, ox) of length M = B OH OW; the patch matrix
//   is never formed. One WAVE owns a 64 (n) x 64 (k = (c kh + ky) kw + kx) tile of one M-split: 4 x 4 MFMA tiles,
//   16 accumulators of 4 fp32. MFMA A = codes^T (row k), B = G (column n): lane (fr, fq) needs 8 consecutive m of
//   ONE k and of ONE n. In NCHW those are 8 consecutive pixels of one channel of G (two 16-B loads when OH OW % 4
//   == 0, else 8 scalar loads) and 8 gathered pixels of one tap of X, each bounds-checked: both operands go from
//   global memory (L1 / L2: neighbouring waves of a workgroup own the k tiles of the same n tile and split, so they
//   read the same G and the same X window) straight into MFMA registers. No LDS, no barrier, no inline assembly.
//   Rows m >= M, columns n >= N and k >= K are not loaded (zero operands); a lane ends with dWq[n = fr][4 fq + j].
//   Split / fold: the M range (in stages of 32) is dealt to `splits` waves per tile, each writing its raw fp32
//   partial tile to the workspace [split][npad][kpad] (N, K rounded up to 64); split_fold_kernel (reduce_common.h)
//   sums them in ascending split order and multiplies by 1 / levels. No atomics: the same call gives the same bits.
//   splits = max(1, min(256, ceil(M / 32), ceil(2048 / tiles))): two waves per SIMD on 256 CUs.
#include "bf16x3.h"
#include "reduce_common.h"
#include "ultra_quant_common.h"

namespace {

// ---- weight quantizer backward --------------------------------------------------------------------------------
// workspace: [0] the bits of m (unsigned), [8] the tie term's coefficient S / (m^2 c) (float), from byte 16 one
// (S, c) pair of doubles per block
struct WqWorkspace {
  unsigned* maxbits;
  float* coef;
  double* partials;
};

inline WqWorkspace wq_workspace(void* ws) {
  char* p = static_cast<char*>(ws);
  return {reinterpret_cast<unsigned*>(p), reinterpret_cast<float*>(p + 8), reinterpret_cast<double*>(p + 16)};
}

__global__ __launch_bounds__(kThreads) void ultra_wq_sums_kernel(const float* __restrict__ w,
                                                                 const float* __restrict__ g, int64_t n,
                                                                 const unsigned* __restrict__ maxbits,
                                                                 double* __restrict__ partials) {
  __shared__ double lds[kWaves][3];
  const float m = __uint_as_float(*maxbits);
  double s = 0.0, c = 0.0, unused = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float t = ultra_tanh(w[i]);
    s += (double)g[i] * (double)t;
    if (fabsf(t) == m) c += 1.0;
  }
  block_sum3(s, c, unused, lds);
  if (threadIdx.x == 0) store_partial2(partials, blockIdx.x, s, c);
}

// one block: thread i adds the partials of blocks i, i + 256, ... in that order, then the block tree
__global__ __launch_bounds__(kThreads) void ultra_wq_finish_kernel(const double* __restrict__ partials, int nblocks,
                                                                   const unsigned* __restrict__ maxbits,
                                                                   float* __restrict__ coef) {
  __shared__ double lds[kWaves][3];
  // (fold_partials2's loop, kept here: through the helper the compiler swaps the registers of the two sums)
  double s = 0.0, c = 0.0, unused = 0.0;
  for (int j = threadIdx.x; j < nblocks; j += kThreads) {
    s += partials[2 * (int64_t)j];
    c += partials[2 * (int64_t)j + 1];
  }
  block_sum3(s, c, unused, lds);
  if (threadIdx.x == 0) {
    const double m = (double)__uint_as_float(*maxbits);
    *coef = (float)(s / (m * m * c));
  }
}

// g_w may be g: a thread reads its element of g before it writes the same element of g_w
__global__ __launch_bounds__(kThreads) void ultra_wq_apply_kernel(const float* __restrict__ w, const float* g,
                                                                  int64_t n, const unsigned* __restrict__ maxbits,
                                                                  const float* __restrict__ coef, float* g_w) {
  const float m = __uint_as_float(*maxbits);
  const float cf = *coef;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float t = ultra_tanh(w[i]);
    const float tie = (fabsf(t) == m) ? (t > 0.f ? cf : (t < 0.f ? -cf : 0.f)) : 0.f;   // sgn(t) coef, selected
    const float gt = g[i] / m - tie;
    g_w[i] = gt * (1.f - t * t);
  }
}

// ---- activation quantizer backward ----------------------------------------------------------------------------
QVIT_DEV float act_mask(float x, float g) { return (x >= 0.f && x <= 1.f) ? g : 0.f; }

__global__ __launch_bounds__(kThreads) void ultra_act_backward_kernel(const float* __restrict__ x, const float* g,
                                                                      int64_t n, float* gx) {
  const int64_t nvec = n / kVec;
  const int64_t tid = blockIdx.x * (int64_t)kThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* o4 = reinterpret_cast<float4*>(gx);
  for (int64_t i = tid; i < nvec; i += stride) {
    const float4 xv = x4[i], gv = g4[i];
    o4[i] = make_float4(act_mask(xv.x, gv.x), act_mask(xv.y, gv.y), act_mask(xv.z, gv.z), act_mask(xv.w, gv.w));
  }
  const int64_t e = nvec * kVec + tid;   // scalar tail: the last n % 4 elements
  if (e < n) gx[e] = act_mask(x[e], g[e]);
}

// ---- conv weight gradient -------------------------------------------------------------------------------------
constexpr int CW_TN = 64;            // dWq rows (output channels) per wave tile
constexpr int CW_TK = 64;            // dWq columns (c, ky, kx) per wave tile
constexpr int CW_BM = 32;            // m per stage: one MFMA contraction
constexpr int CW_MAX_SPLITS = 256;
constexpr int CW_TARGET_WAVES = 2048;
constexpr int CW_FAR = -(1 << 29);   // row base of a stage row m >= M: every tap of it fails the image test

struct ConvGeo {
  int B, C, H, W, N, kh, kw, sh, sw, ph, pw, dh, dw, OH, OW, K, M;
};

// part[sp][n][k] (n < npad, k < kpad) = sum over the split's m of G[m][n] code[m][k]
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const float* __restrict__ G, const float* __restrict__ X,
                                                         ConvGeo geo, float levels, int splits, int npad, int kpad,
                                                         int gvec, float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int fr = lane & 15, fq = lane >> 4;
  // unit = (split, n tile, k tile), k tiles fastest: the four waves of a workgroup share G and the X window
  const int nb_n = npad / CW_TN, nb_k = kpad / CW_TK;
  const int64_t total = (int64_t)splits * nb_n * nb_k;
  const int64_t u = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (u >= total) return;   // (the whole wave)
  const int tk = (int)(u % nb_k), tn = (int)((u / nb_k) % nb_n), sp = (int)(u / ((int64_t)nb_k * nb_n));
  const int n0 = tn * CW_TN, k0 = tk * CW_TK;
  const int ntl = min(4, (geo.N - n0 + 15) >> 4), ktl = min(4, (geo.K - k0 + 15) >> 4);   // live 16-wide sub-tiles
  const int nst = (geo.M + CW_BM - 1) / CW_BM;
  const int s0 = (int)((int64_t)sp * nst / splits), s1 = (int)((int64_t)(sp + 1) * nst / splits);
  const int P = geo.OH * geo.OW;
  const int64_t HW = (int64_t)geo.H * geo.W;

  // this lane's tap per k sub-tile: channel offset, row / column offsets; a dead column (k >= K) fails every test
  int kyo[4], kxo[4];
  int64_t coff[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    const int kk = k0 + 16 * kt + fr;
    const bool ok = kk < geo.K;
    const int kc = ok ? kk : 0;
    const int c = kc / (geo.kh * geo.kw), r = kc - c * (geo.kh * geo.kw);
    const int ky = r / geo.kw, kx = r - ky * geo.kw;
    kyo[kt] = ok ? ky * geo.dh - geo.ph : CW_FAR;
    kxo[kt] = kx * geo.dw - geo.pw;
    coff[kt] = (int64_t)c * HW;
  }

  f4 acc[4][4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[kt][nt] = f4{0.f, 0.f, 0.f, 0.f};

  for (int st = s0; st < s1; ++st) {
    // this lane's 8 contraction rows m8 .. m8 + 7 as (image, output row, output column)
    const int m8 = st * CW_BM + 8 * fq;
    int b = m8 / P;
    int p = m8 - b * P;
    int oy = p / geo.OW, ox = p - oy * geo.OW;
    int iyb[8], ixb[8];
    int64_t xb[8], gb[8];   // offsets of image b in X, of pixel (b, channel 0, p) in G
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool live = m8 + j < geo.M;
      iyb[j] = live ? oy * geo.sh : CW_FAR;
      ixb[j] = ox * geo.sw;
      xb[j] = live ? (int64_t)b * geo.C * HW : 0;
      gb[j] = live ? (int64_t)b * geo.N * P + p : -1;
      ++p;
      if (++ox == geo.OW) {
        ox = 0;
        if (++oy == geo.OH) {
          oy = 0;
          p = 0;
          ++b;
        }
      }
    }

    // codes^T operands: 8 gathered taps per live k sub-tile
    bf8 cf[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (kt < ktl) {
        float k[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int iy = iyb[j] + kyo[kt], ix = ixb[j] + kxo[kt];
          const bool in = (unsigned)iy < (unsigned)geo.H && (unsigned)ix < (unsigned)geo.W;
          const float x = in ? X[xb[j] + coff[kt] + (int64_t)iy * geo.W + ix] : 0.f;
          k[j] = rintf(x * levels);   // an integer <= 127: a bf16 exactly
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = hi16(k[2 * e], k[2 * e + 1]);
      }
      cf[kt] = as_bf8(w[0], w[1], w[2], w[3]);
    }

#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      if (nt < ntl) {
        const int n = n0 + 16 * nt + fr;
        float gv[8];
        if (n < geo.N) {
          const int64_t noff = (int64_t)n * P;
          if (gvec) {   // OH OW % 4 == 0: m8 and m8 + 4 start 16-byte groups inside one channel image
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const f4 v = gb[4 * h] >= 0 ? *reinterpret_cast<const f4*>(G + gb[4 * h] + noff) : f4{0.f, 0.f, 0.f, 0.f};
              gv[4 * h] = v[0]; gv[4 * h + 1] = v[1]; gv[4 * h + 2] = v[2]; gv[4 * h + 3] = v[3];
            }
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) gv[j] = gb[j] >= 0 ? G[gb[j] + noff] : 0.f;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) gv[j] = 0.f;
        }
        uint32_t p1[4], p2[4], p3[4];
#pragma unroll
        for (int e = 0; e < 8; e += 2) split_bf16x3(gv[e], gv[e + 1], p1[e >> 1], p2[e >> 1], p3[e >> 1]);
        const bf8 g1 = as_bf8(p1[0], p1[1], p1[2], p1[3]);
        const bf8 g2 = as_bf8(p2[0], p2[1], p2[2], p2[3]);
        const bf8 g3 = as_bf8(p3[0], p3[1], p3[2], p3[3]);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          if (kt < ktl) {
            acc[kt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cf[kt], g1, acc[kt][nt], 0, 0, 0);
            acc[kt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cf[kt], g2, acc[kt][nt], 0, 0, 0);
            acc[kt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cf[kt], g3, acc[kt][nt], 0, 0, 0);
          }
        }
      }
    }
  }

  // the whole tile, dead sub-tiles included (zeros): the fold reads n < N, k < K
  float* pb = part + ((int64_t)sp * npad + n0 + fr) * kpad + k0 + 4 * fq;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) *reinterpret_cast<f4*>(pb + (int64_t)16 * nt * kpad + 16 * kt) = acc[kt][nt];
}

int64_t round64(int64_t v) { return (v + 63) / 64 * 64; }

// fills geo; false: a size the kernel does not take
bool conv_wgrad_geo(int64_t B, int64_t C, int64_t H, int64_t W, int64_t N, int kh, int kw, int sh, int sw, int ph,
                    int pw, int dh, int dw, ConvGeo* geo) {
  const int64_t lim = 1 << 20;
  // (the upper bounds first: they bound what qvit_conv_shape multiplies; a size below its range fails there)
  if (C > lim || H > lim || W > lim || N > lim || kh > 1024 || kw > 1024 || sh > lim || sw > lim || ph > lim ||
      pw > lim || dh > 1024 || dw > 1024)
    return false;
  ConvShape cs;
  if (N < 1 || qvit_conv_shape(B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, cs)) return false;
  const int64_t OH = cs.OH, OW = cs.OW, K = cs.K, M = cs.M;
  if (K > lim || OH * OW > (1 << 30) || M > (int64_t)INT32_MAX - 64) return false;
  if ((round64(N) / CW_TN) * (round64(K) / CW_TK) > (1 << 20)) return false;   // (grid and unit counts fit int32)
  *geo = ConvGeo{(int)B, (int)C, (int)H, (int)W, (int)N, kh, kw, sh, sw, ph, pw, dh, dw, (int)OH, (int)OW, (int)K, (int)M};
  return true;
}

int64_t conv_wgrad_splits(const ConvGeo& g) {
  const int64_t tiles = (round64(g.N) / CW_TN) * (round64(g.K) / CW_TK);
  const int64_t nst = ((int64_t)g.M + CW_BM - 1) / CW_BM;
  return split_count(tiles, nst, CW_MAX_SPLITS, CW_TARGET_WAVES);
}

}  // namespace

extern "C" {

int64_t qvit_ultra_weight_quant_backward_workspace_bytes(int64_t n) {
  if (n < 0) return QVIT_EINVAL;
  return 16 + (int64_t)stream_grid(n, 1) * 2 * (int64_t)sizeof(double);
}

int qvit_ultra_weight_quant_backward(const float* w, const float* grad_out, int64_t n, int w_bit, float* grad_w,
                                     void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  if (!w || !grad_out || !grad_w || !workspace) return QVIT_ENULL;
  if (n < 0 || w_bit < 2 || w_bit > 8) return QVIT_EINVAL;   // quant_ultra.py:33 (1 and 32 are not this quantizer)
  if (workspace_bytes < qvit_ultra_weight_quant_backward_workspace_bytes(n)) return QVIT_EINVAL;
  if (qvit_misaligned(3, w, grad_out, grad_w) || qvit_misaligned(7, workspace)) return QVIT_EALIGN;
  if (n == 0) return QVIT_OK;
  const WqWorkspace ws = wq_workspace(workspace);
  const hipError_t e = hipMemsetAsync(ws.maxbits, 0, sizeof(unsigned), stream);
  if (e != hipSuccess) return qvit_hip_status(e);
  const int grid = stream_grid(n, 1);
  hipLaunchKernelGGL(ultra_wmax_kernel, dim3(grid), dim3(kThreads), 0, stream, w, n, ws.maxbits);
  hipLaunchKernelGGL(ultra_wq_sums_kernel, dim3(grid), dim3(kThreads), 0, stream, w, grad_out, n, ws.maxbits,
                     ws.partials);
  hipLaunchKernelGGL(ultra_wq_finish_kernel, dim3(1), dim3(kThreads), 0, stream, ws.partials, grid, ws.maxbits,
                     ws.coef);
  hipLaunchKernelGGL(ultra_wq_apply_kernel, dim3(grid), dim3(kThreads), 0, stream, w, grad_out, n, ws.maxbits,
                     ws.coef, grad_w);
  return qvit_launch_status();
}

int qvit_ultra_act_quant_backward(const float* x, const float* grad_out, int64_t n, float* grad_x,
                                  hipStream_t stream) {
  if (!x || !grad_out || !grad_x) return QVIT_ENULL;
  if (n < 0) return QVIT_EINVAL;
  if (qvit_misaligned(15, x, grad_out, grad_x)) return QVIT_EALIGN;
  if (n == 0) return QVIT_OK;
  hipLaunchKernelGGL(ultra_act_backward_kernel, dim3(stream_grid(n, kVec)), dim3(kThreads), 0, stream, x, grad_out,
                     n, grad_x);
  return qvit_launch_status();
}

int64_t qvit_conv_wgrad_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t N, int kh, int kw,
                                        int sh, int sw, int ph, int pw, int dh, int dw) {
  ConvGeo g;
  if (!conv_wgrad_geo(B, C, H, W, N, kh, kw, sh, sw, ph, pw, dh, dw, &g)) return QVIT_EINVAL;
  return conv_wgrad_splits(g) * round64(g.N) * round64(g.K) * 4;
}

int qvit_conv_wgrad(const float* G, const float* X, int64_t B, int64_t C, int64_t H, int64_t W, int64_t N, int kh,
                    int kw, int sh, int sw, int ph, int pw, int dh, int dw, int levels, float* dW, void* workspace,
                    int64_t workspace_bytes, hipStream_t stream) {
  if (!G || !X || !dW || !workspace) return QVIT_ENULL;
  ConvGeo g;
  if (!conv_wgrad_geo(B, C, H, W, N, kh, kw, sh, sw, ph, pw, dh, dw, &g)) return QVIT_EINVAL;
  if (levels < 1 || levels > 127) return QVIT_EINVAL;
  if (qvit_misaligned(3, G, X, dW) || qvit_misaligned(15, workspace)) return QVIT_EALIGN;
  const int64_t npad = round64(g.N), kpad = round64(g.K);
  const int64_t splits = g.M == 0 ? 0 : conv_wgrad_splits(g);
  if (workspace_bytes < conv_wgrad_splits(g) * npad * kpad * 4) return QVIT_EINVAL;
  float* part = reinterpret_cast<float*>(workspace);
  if (splits > 0) {
    const int64_t total = splits * (npad / CW_TN) * (kpad / CW_TK);
    const int gvec = ((int64_t)g.OH * g.OW) % 4 == 0 && !qvit_misaligned(15, G);
    hipLaunchKernelGGL(conv_wgrad_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, stream, G, X, g,
                       (float)levels, (int)splits, (int)npad, (int)kpad, gvec, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qvit_hip_status(e);
  }
  hipLaunchKernelGGL(split_fold_kernel<float>, dim3((unsigned)(((int64_t)g.N * g.K + 255) / 256)), dim3(256), 0,
                     stream, part, (int)splits, g.N, g.K, (int)npad, (int)kpad, 1.f / (float)levels, dW);
  return qvit_launch_status();
}

}  // extern "C"
