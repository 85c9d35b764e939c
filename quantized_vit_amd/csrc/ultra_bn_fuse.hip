// UltraNet training: BatchNorm2d on batch statistics -> activation_quantize_fn -> optional MaxPool2d(2, 2) as one
// autograd node over NCHW fp32 (reference `4-bit quantization/mymodel.py:71-124`, the run between two Conv2d_Q).
//
// qvit_bn_stats  per channel c over M = B H W values: mean, biased variance, invstd = 1 / sqrt(var + eps), and
//   nn.BatchNorm2d's running update r = (1 - f) r + f new (new = mean, resp. the unbiased var M / (M - 1)).
//   Accumulation is in double on data shifted by K_c = x[0][c][0][0]: s = sum (x - K), ss = sum (x - K)^2,
//   mean = K + s / M, var = max(0, (ss - s s / M) / M). The shift keeps ss - s^2 / M free of the cancellation a
//   large |mean| / std would bring (the terms are of the size of the spread around one sample, not of the mean).
// qvit_bn_act_pool_forward  a = gamma invstd (fp32), y = fmaf(x - mean, a, beta), k = quant_code(y) of
//   qvit_common.h (QVIT_QT_ULTRA_ACT: rint(clamp(y, 0, 1) levels), NaN -> 0), pass = 0 <= y <= 1.
//   Unpooled: out = k / levels, flag byte = pass. Pooled (2 x 2, stride 2, floor): out = (max k) / levels, flag
//   byte = pass(winner) | winner << 1, winner = 2 dy + dx of the FIRST maximum in row-major order (ATen's
//   val > maxval walk: equal codes leave the earlier element the winner).
// qvit_bn_act_pool_backward_reduce  g_y = grad_out at the (winner's) position when its pass bit is set, else 0;
//   S1 = sum g_y, S2 = sum g_y xhat, xhat = (x - mean) invstd recomputed. Masks select: a NaN grad_out behind a
//   cleared pass bit is never read into a sum.
// qvit_bn_act_pool_backward_dx  dx = a (g_y - S1 / M - xhat S2 / M) at every element of x (a pooled-away element
//   and a dropped odd row / column have g_y = 0), dgamma = S2, dbeta = S1.
//
// Geometry, all four: streaming kernels, a workgroup of 256 threads owns one slice of one (b, c) plane, 8192
// elements of x (8 x 16 B per lane); every index inside a plane is int32, the plane's base int64. The 16-byte arm
// runs when the pointers are 16-byte aligned (flags: 4) and H W % 4 == 0 (pooled: W % 4 == 0, a lane then owns two
// adjacent windows: two float4 rows in, one float2 out); otherwise the scalar arm, same slices. Reductions:
// per-thread double accumulation, reduce_common.h's fixed-order wave / block tree, one partial pair per
// workgroup at [c][b][slice], one workgroup per channel folding its partials in index order. No atomics: two calls
// give the same bits, whatever the workspace held.
#include <initializer_list>

#include "reduce_common.h"

namespace {

constexpr int kChunk = 8192;   // x elements per workgroup

struct BnGeo {
  int B, C, H, W, HW, OH, OW, P;   // P = OH OW
  int S;                           // slices per plane of the kernel at hand
  int pool;
  double M;
};

// stats: always slices of the full plane; the other three: of the pooled plane when pool (2048 windows a slice)
bool bn_geo(int64_t B, int64_t C, int64_t H, int64_t W, int pool, bool stats, BnGeo* g) {
  const int64_t lim = INT32_MAX;
  if (B < 1 || C < 1 || H < 1 || W < 1 || B > lim || C > lim || H > lim || W > lim) return false;
  if (pool != 0 && pool != 1) return false;
  const int64_t HW = H * W;
  if (HW > lim - kChunk || B * C > lim) return false;   // in-plane indices and the plane count are int32
  if (B * HW < 2) return false;                         // batch statistics need two values per channel
  if (pool && (H < 2 || W < 2)) return false;           // an empty pooled map
  const int64_t OH = pool ? H / 2 : H, OW = pool ? W / 2 : W;
  const int64_t S = (pool && !stats) ? cdiv(OH * OW, kChunk / 4) : cdiv(HW, kChunk);
  if (B * C * S > lim) return false;                    // the grid
  *g = BnGeo{(int)B, (int)C, (int)H, (int)W, (int)HW, (int)OH, (int)OW, (int)(OH * OW), (int)S, pool,
             (double)B * (double)HW};
  return true;
}

struct Slot {
  int plane, sl, b, c;
};

QVIT_DEV Slot slot_of(const BnGeo& g) {
  Slot s;
  s.plane = (int)(blockIdx.x / (unsigned)g.S);
  s.sl = (int)(blockIdx.x - (unsigned)s.plane * (unsigned)g.S);
  s.b = s.plane / g.C;
  s.c = s.plane - s.b * g.C;
  return s;
}

QVIT_DEV int64_t partial_index(const BnGeo& g, const Slot& s) { return ((int64_t)s.c * g.B + s.b) * g.S + s.sl; }

// ---- statistics -----------------------------------------------------------------------------------------------
QVIT_DEV void stat_add(float v, double K, double& s, double& ss) {
  const double d = (double)v - K;
  s += d;
  ss = fma(d, d, ss);
}

__global__ __launch_bounds__(kThreads) void bn_stats_partial_kernel(const float* __restrict__ x, BnGeo g, int vec,
                                                                    double* __restrict__ partials) {
  __shared__ double lds[kWaves][3];
  const Slot sl = slot_of(g);
  const float* xp = x + (int64_t)sl.plane * g.HW;
  const double K = (double)x[(int64_t)sl.c * g.HW];
  const int e0 = sl.sl * kChunk, e1 = min(g.HW, e0 + kChunk);
  double s = 0.0, ss = 0.0, unused = 0.0;
  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(xp);
    for (int i = e0 / 4 + (int)threadIdx.x; i < e1 / 4; i += kThreads) {
      const float4 v = x4[i];
      stat_add(v.x, K, s, ss); stat_add(v.y, K, s, ss); stat_add(v.z, K, s, ss); stat_add(v.w, K, s, ss);
    }
  } else {
    for (int i = e0 + (int)threadIdx.x; i < e1; i += kThreads) stat_add(xp[i], K, s, ss);
  }
  block_sum3(s, ss, unused, lds);
  if (threadIdx.x == 0) store_partial2(partials, partial_index(g, sl), s, ss);
}

// one workgroup per channel folds the channel's partials (fold_partials2)
__global__ __launch_bounds__(kThreads) void bn_stats_finish_kernel(const double* __restrict__ partials,
                                                                   const float* __restrict__ x, BnGeo g, double eps,
                                                                   double factor, float* rmean, float* rvar,
                                                                   float* __restrict__ mean, float* __restrict__ var,
                                                                   float* __restrict__ invstd) {
  __shared__ double lds[kWaves][3];
  const int c = blockIdx.x, n = g.B * g.S;
  double s = 0.0, ss = 0.0;
  fold_partials2(partials + 2 * (int64_t)c * n, n, s, ss, lds);
  if (threadIdx.x == 0) {
    const double K = (double)x[(int64_t)c * g.HW];
    const double m = s / g.M;
    const double mu = K + m;
    double v = (ss - s * m) / g.M;
    v = v < 0.0 ? 0.0 : v;   // (a NaN stays)
    mean[c] = (float)mu;
    var[c] = (float)v;
    invstd[c] = (float)(1.0 / sqrt(v + eps));
    if (rmean) rmean[c] = (float)((1.0 - factor) * (double)rmean[c] + factor * mu);
    if (rvar) rvar[c] = (float)((1.0 - factor) * (double)rvar[c] + factor * (v * (g.M / (g.M - 1.0))));
  }
}

// ---- forward --------------------------------------------------------------------------------------------------
struct Chan {
  float mu, a, be, is;
};

QVIT_DEV Chan load_chan(int c, const float* mean, const float* invstd, const float* gamma, const float* beta) {
  Chan k;
  k.mu = mean[c];
  k.is = invstd[c];
  k.a = (gamma ? gamma[c] : 1.f) * k.is;
  k.be = beta ? beta[c] : 0.f;
  return k;
}

QVIT_DEV float bn_y(float x, const Chan& k) { return fmaf(x - k.mu, k.a, k.be); }
QVIT_DEV unsigned pass_bit(float y) { return (y >= 0.f && y <= 1.f) ? 1u : 0u; }   // both edges pass, NaN fails

QVIT_DEV float act_one(float x, const Chan& k, const QParams& q, unsigned& flag) {
  const float y = bn_y(x, k);
  flag = pass_bit(y);
  return quant_code(y, q) / q.levels;
}

// one 2 x 2 window (row-major x0 x1 / x2 x3): the value of the maximum code and the flag byte
QVIT_DEV float pool_one(float x0, float x1, float x2, float x3, const Chan& k, const QParams& q, unsigned& byte) {
  const float y0 = bn_y(x0, k), y1 = bn_y(x1, k), y2 = bn_y(x2, k), y3 = bn_y(x3, k);
  float best = quant_code(y0, q), yw = y0;
  unsigned idx = 0;
  const float k1 = quant_code(y1, q), k2 = quant_code(y2, q), k3 = quant_code(y3, q);
  if (k1 > best) { best = k1; yw = y1; idx = 1; }
  if (k2 > best) { best = k2; yw = y2; idx = 2; }
  if (k3 > best) { best = k3; yw = y3; idx = 3; }
  byte = pass_bit(yw) | (idx << 1);
  return best / q.levels;
}

__global__ __launch_bounds__(kThreads) void bn_act_forward_kernel(const float* __restrict__ x, BnGeo g, int vec,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, int levels,
                                                                  float* __restrict__ out,
                                                                  uint8_t* __restrict__ flags) {
  const Slot sl = slot_of(g);
  const Chan k = load_chan(sl.c, mean, invstd, gamma, beta);
  const QParams q = load_qparams(QVIT_QT_ULTRA_ACT, nullptr, nullptr, nullptr, levels);
  const int64_t base = (int64_t)sl.plane * g.HW;
  const int e0 = sl.sl * kChunk, e1 = min(g.HW, e0 + kChunk);
  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(x + base);
    float4* o4 = reinterpret_cast<float4*>(out + base);
    uint32_t* f4 = reinterpret_cast<uint32_t*>(flags + base);
    for (int i = e0 / 4 + (int)threadIdx.x; i < e1 / 4; i += kThreads) {
      const float4 v = x4[i];
      unsigned f0, f1, f2, f3;
      float4 o;
      o.x = act_one(v.x, k, q, f0); o.y = act_one(v.y, k, q, f1);
      o.z = act_one(v.z, k, q, f2); o.w = act_one(v.w, k, q, f3);
      o4[i] = o;
      f4[i] = f0 | (f1 << 8) | (f2 << 16) | (f3 << 24);
    }
  } else {
    for (int i = e0 + (int)threadIdx.x; i < e1; i += kThreads) {
      unsigned f;
      out[base + i] = act_one(x[base + i], k, q, f);
      flags[base + i] = (uint8_t)f;
    }
  }
}

// the pooled kernels' slice: windows [w0, w1) of the plane's P; the 16-byte arm walks them in pairs
QVIT_DEV void pool_slice(const BnGeo& g, int sl, int& w0, int& w1) {
  w0 = sl * (kChunk / 4);
  w1 = min(g.P, w0 + kChunk / 4);
}

__global__ __launch_bounds__(kThreads) void bn_act_pool_forward_kernel(const float* __restrict__ x, BnGeo g, int vec,
                                                                       const float* __restrict__ mean,
                                                                       const float* __restrict__ invstd,
                                                                       const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta, int levels,
                                                                       float* __restrict__ out,
                                                                       uint8_t* __restrict__ flags) {
  const Slot sl = slot_of(g);
  const Chan k = load_chan(sl.c, mean, invstd, gamma, beta);
  const QParams q = load_qparams(QVIT_QT_ULTRA_ACT, nullptr, nullptr, nullptr, levels);
  const float* xp = x + (int64_t)sl.plane * g.HW;
  const int64_t obase = (int64_t)sl.plane * g.P;
  int w0, w1;
  pool_slice(g, sl.sl, w0, w1);
  if (vec) {   // W % 4 == 0: OW even, P even, w0 even
    const float4* x4 = reinterpret_cast<const float4*>(xp);
    const int ow2 = g.OW / 2, w4 = g.W / 4;
    for (int t = w0 / 2 + (int)threadIdx.x; t < w1 / 2; t += kThreads) {
      const int oy = t / ow2, j = t - oy * ow2;
      const float4 r0 = x4[2 * oy * w4 + j], r1 = x4[(2 * oy + 1) * w4 + j];
      unsigned b0, b1;
      float2 o;
      o.x = pool_one(r0.x, r0.y, r1.x, r1.y, k, q, b0);
      o.y = pool_one(r0.z, r0.w, r1.z, r1.w, k, q, b1);
      *reinterpret_cast<float2*>(out + obase + 2 * t) = o;
      *reinterpret_cast<uint16_t*>(flags + obase + 2 * t) = (uint16_t)(b0 | (b1 << 8));
    }
  } else {
    for (int t = w0 + (int)threadIdx.x; t < w1; t += kThreads) {
      const int oy = t / g.OW, ox = t - oy * g.OW;
      const float* r = xp + 2 * oy * g.W + 2 * ox;
      unsigned b;
      out[obase + t] = pool_one(r[0], r[1], r[g.W], r[g.W + 1], k, q, b);
      flags[obase + t] = (uint8_t)b;
    }
  }
}

// ---- backward: the two sums -----------------------------------------------------------------------------------
QVIT_DEV void sums_add(float gy, float x, const Chan& k, double& s1, double& s2) {
  const float xhat = (x - k.mu) * k.is;
  s1 += (double)gy;
  s2 = fma((double)gy, (double)xhat, s2);
}

QVIT_DEV float pick4(unsigned idx, float x0, float x1, float x2, float x3) {
  return idx == 0 ? x0 : (idx == 1 ? x1 : (idx == 2 ? x2 : x3));
}

__global__ __launch_bounds__(kThreads) void bn_act_reduce_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ go,
                                                                 const uint8_t* __restrict__ flags, BnGeo g, int vec,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd,
                                                                 double* __restrict__ partials) {
  __shared__ double lds[kWaves][3];
  const Slot sl = slot_of(g);
  const Chan k = load_chan(sl.c, mean, invstd, nullptr, nullptr);
  const int64_t base = (int64_t)sl.plane * g.HW;
  const int e0 = sl.sl * kChunk, e1 = min(g.HW, e0 + kChunk);
  double s1 = 0.0, s2 = 0.0, unused = 0.0;
  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(x + base);
    const float4* g4 = reinterpret_cast<const float4*>(go + base);
    const uint32_t* f4 = reinterpret_cast<const uint32_t*>(flags + base);
    for (int i = e0 / 4 + (int)threadIdx.x; i < e1 / 4; i += kThreads) {
      const float4 v = x4[i], gv = g4[i];
      const uint32_t f = f4[i];
      if (f & 1u) sums_add(gv.x, v.x, k, s1, s2);
      if (f & 0x100u) sums_add(gv.y, v.y, k, s1, s2);
      if (f & 0x10000u) sums_add(gv.z, v.z, k, s1, s2);
      if (f & 0x1000000u) sums_add(gv.w, v.w, k, s1, s2);
    }
  } else {
    for (int i = e0 + (int)threadIdx.x; i < e1; i += kThreads)
      if (flags[base + i] & 1) sums_add(go[base + i], x[base + i], k, s1, s2);
  }
  block_sum3(s1, s2, unused, lds);
  if (threadIdx.x == 0) store_partial2(partials, partial_index(g, sl), s1, s2);
}

__global__ __launch_bounds__(kThreads) void bn_act_pool_reduce_kernel(const float* __restrict__ x,
                                                                      const float* __restrict__ go,
                                                                      const uint8_t* __restrict__ flags, BnGeo g,
                                                                      int vec, const float* __restrict__ mean,
                                                                      const float* __restrict__ invstd,
                                                                      double* __restrict__ partials) {
  __shared__ double lds[kWaves][3];
  const Slot sl = slot_of(g);
  const Chan k = load_chan(sl.c, mean, invstd, nullptr, nullptr);
  const float* xp = x + (int64_t)sl.plane * g.HW;
  const int64_t obase = (int64_t)sl.plane * g.P;
  int w0, w1;
  pool_slice(g, sl.sl, w0, w1);
  double s1 = 0.0, s2 = 0.0, unused = 0.0;
  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(xp);
    const int ow2 = g.OW / 2, w4 = g.W / 4;
    for (int t = w0 / 2 + (int)threadIdx.x; t < w1 / 2; t += kThreads) {
      const int oy = t / ow2, j = t - oy * ow2;
      const unsigned f = *reinterpret_cast<const uint16_t*>(flags + obase + 2 * t);
      if (!(f & 0x0101u)) continue;   // neither window passes: nothing to read
      const float4 r0 = x4[2 * oy * w4 + j], r1 = x4[(2 * oy + 1) * w4 + j];
      const float2 gv = *reinterpret_cast<const float2*>(go + obase + 2 * t);
      if (f & 1u) sums_add(gv.x, pick4((f >> 1) & 3u, r0.x, r0.y, r1.x, r1.y), k, s1, s2);
      if (f & 0x100u) sums_add(gv.y, pick4((f >> 9) & 3u, r0.z, r0.w, r1.z, r1.w), k, s1, s2);
    }
  } else {
    for (int t = w0 + (int)threadIdx.x; t < w1; t += kThreads) {
      const unsigned f = flags[obase + t];
      if (!(f & 1u)) continue;
      const int oy = t / g.OW, ox = t - oy * g.OW;
      const unsigned idx = (f >> 1) & 3u;
      const float xv = xp[(2 * oy + (int)(idx >> 1)) * g.W + 2 * ox + (int)(idx & 1u)];
      sums_add(go[obase + t], xv, k, s1, s2);
    }
  }
  block_sum3(s1, s2, unused, lds);
  if (threadIdx.x == 0) store_partial2(partials, partial_index(g, sl), s1, s2);
}

__global__ __launch_bounds__(kThreads) void bn_bwd_finish_kernel(const double* __restrict__ partials, BnGeo g,
                                                                 double* __restrict__ sums) {
  __shared__ double lds[kWaves][3];
  const int c = blockIdx.x, n = g.B * g.S;
  double s1 = 0.0, s2 = 0.0;
  fold_partials2(partials + 2 * (int64_t)c * n, n, s1, s2, lds);
  if (threadIdx.x == 0) {
    sums[c] = s1;
    sums[g.C + c] = s2;
  }
}

// ---- backward: dx ---------------------------------------------------------------------------------------------
struct DxChan {
  float mu, is, a, c1, c2;
};

QVIT_DEV DxChan load_dx_chan(int c, const BnGeo& g, const float* mean, const float* invstd, const float* gamma,
                             const double* sums) {
  DxChan k;
  k.mu = mean[c];
  k.is = invstd[c];
  k.a = (gamma ? gamma[c] : 1.f) * k.is;
  k.c1 = (float)(sums[c] / g.M);
  k.c2 = (float)(sums[g.C + c] / g.M);
  return k;
}

QVIT_DEV float dx_one(float gy, float x, const DxChan& k) {
  const float xhat = (x - k.mu) * k.is;
  return k.a * fmaf(-xhat, k.c2, gy - k.c1);
}

QVIT_DEV void write_param_grads(const Slot& sl, const BnGeo& g, const double* sums, float* dgamma, float* dbeta) {
  if (sl.b == 0 && sl.sl == 0 && threadIdx.x == 0) {
    if (dgamma) dgamma[sl.c] = (float)sums[g.C + sl.c];
    if (dbeta) dbeta[sl.c] = (float)sums[sl.c];
  }
}

__global__ __launch_bounds__(kThreads) void bn_act_dx_kernel(const float* __restrict__ x, const float* __restrict__ go,
                                                             const uint8_t* __restrict__ flags, BnGeo g, int vec,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma,
                                                             const double* __restrict__ sums, float* __restrict__ dx,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const Slot sl = slot_of(g);
  const DxChan k = load_dx_chan(sl.c, g, mean, invstd, gamma, sums);
  const int64_t base = (int64_t)sl.plane * g.HW;
  const int e0 = sl.sl * kChunk, e1 = min(g.HW, e0 + kChunk);
  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(x + base);
    const float4* g4 = reinterpret_cast<const float4*>(go + base);
    const uint32_t* f4 = reinterpret_cast<const uint32_t*>(flags + base);
    float4* d4 = reinterpret_cast<float4*>(dx + base);
    for (int i = e0 / 4 + (int)threadIdx.x; i < e1 / 4; i += kThreads) {
      const float4 v = x4[i], gv = g4[i];
      const uint32_t f = f4[i];
      float4 o;
      o.x = dx_one((f & 1u) ? gv.x : 0.f, v.x, k);
      o.y = dx_one((f & 0x100u) ? gv.y : 0.f, v.y, k);
      o.z = dx_one((f & 0x10000u) ? gv.z : 0.f, v.z, k);
      o.w = dx_one((f & 0x1000000u) ? gv.w : 0.f, v.w, k);
      d4[i] = o;
    }
  } else {
    for (int i = e0 + (int)threadIdx.x; i < e1; i += kThreads)
      dx[base + i] = dx_one((flags[base + i] & 1) ? go[base + i] : 0.f, x[base + i], k);
  }
  write_param_grads(sl, g, sums, dgamma, dbeta);
}

// g_y of element e (0..3, row-major) of a window with flag byte f and incoming gradient gv
QVIT_DEV float win_gy(unsigned f, unsigned e, float gv) { return ((f & 1u) && ((f >> 1) & 3u) == e) ? gv : 0.f; }

__global__ __launch_bounds__(kThreads) void bn_act_pool_dx_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ go,
                                                                  const uint8_t* __restrict__ flags, BnGeo g, int vec,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd,
                                                                  const float* __restrict__ gamma,
                                                                  const double* __restrict__ sums,
                                                                  float* __restrict__ dx, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta) {
  const Slot sl = slot_of(g);
  const DxChan k = load_dx_chan(sl.c, g, mean, invstd, gamma, sums);
  const float* xp = x + (int64_t)sl.plane * g.HW;
  float* dp = dx + (int64_t)sl.plane * g.HW;
  const int64_t obase = (int64_t)sl.plane * g.P;
  int w0, w1;
  pool_slice(g, sl.sl, w0, w1);
  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(xp);
    float4* d4 = reinterpret_cast<float4*>(dp);
    const int ow2 = g.OW / 2, w4 = g.W / 4;
    for (int t = w0 / 2 + (int)threadIdx.x; t < w1 / 2; t += kThreads) {
      const int oy = t / ow2, j = t - oy * ow2;
      const unsigned f = *reinterpret_cast<const uint16_t*>(flags + obase + 2 * t);
      const float2 gv = *reinterpret_cast<const float2*>(go + obase + 2 * t);
      const int i0 = 2 * oy * w4 + j, i1 = (2 * oy + 1) * w4 + j;
      const float4 r0 = x4[i0], r1 = x4[i1];
      const unsigned fa = f & 0xffu, fb = f >> 8;
      float4 o0, o1;
      o0.x = dx_one(win_gy(fa, 0, gv.x), r0.x, k); o0.y = dx_one(win_gy(fa, 1, gv.x), r0.y, k);
      o0.z = dx_one(win_gy(fb, 0, gv.y), r0.z, k); o0.w = dx_one(win_gy(fb, 1, gv.y), r0.w, k);
      o1.x = dx_one(win_gy(fa, 2, gv.x), r1.x, k); o1.y = dx_one(win_gy(fa, 3, gv.x), r1.y, k);
      o1.z = dx_one(win_gy(fb, 2, gv.y), r1.z, k); o1.w = dx_one(win_gy(fb, 3, gv.y), r1.w, k);
      d4[i0] = o0;
      d4[i1] = o1;
    }
  } else {
    for (int t = w0 + (int)threadIdx.x; t < w1; t += kThreads) {
      const int oy = t / g.OW, ox = t - oy * g.OW;
      const unsigned f = flags[obase + t];
      const float gv = go[obase + t];
      const int i0 = 2 * oy * g.W + 2 * ox;
      dp[i0] = dx_one(win_gy(f, 0, gv), xp[i0], k);
      dp[i0 + 1] = dx_one(win_gy(f, 1, gv), xp[i0 + 1], k);
      dp[i0 + g.W] = dx_one(win_gy(f, 2, gv), xp[i0 + g.W], k);
      dp[i0 + g.W + 1] = dx_one(win_gy(f, 3, gv), xp[i0 + g.W + 1], k);
    }
  }
  if (sl.sl == 0) {   // the floor mode's dropped last row and column: g_y = 0
    if (g.H & 1)
      for (int i = (g.H - 1) * g.W + (int)threadIdx.x; i < g.HW; i += kThreads) dp[i] = dx_one(0.f, xp[i], k);
    if (g.W & 1)
      for (int r = threadIdx.x; r < 2 * g.OH; r += kThreads) {
        const int i = r * g.W + g.W - 1;
        dp[i] = dx_one(0.f, xp[i], k);
      }
  }
  write_param_grads(sl, g, sums, dgamma, dbeta);
}

// the 16-byte arm: every plane base 16-byte aligned in the fp32 tensors (4 in the flag bytes) and rows that pair up
inline int vec_arm(const BnGeo& g, bool pooled_kernel, std::initializer_list<const void*> f32, const void* flags) {
  if (pooled_kernel ? (g.W % 4 != 0) : (g.HW % 4 != 0)) return 0;
  for (const void* p : f32)
    if (qvit_misaligned(15, p)) return 0;
  return qvit_misaligned(3, flags) ? 0 : 1;
}

}  // namespace

extern "C" {

int64_t qvit_bn_stats_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W) {
  BnGeo g;
  if (!bn_geo(B, C, H, W, 0, true, &g)) return QVIT_EINVAL;
  return (int64_t)g.C * g.B * g.S * 2 * (int64_t)sizeof(double);
}

int qvit_bn_stats(const float* x, int64_t B, int64_t C, int64_t H, int64_t W, double eps, double factor,
                  float* running_mean, float* running_var, float* mean, float* var, float* invstd, void* workspace,
                  int64_t workspace_bytes, hipStream_t stream) {
  if (!x || !mean || !var || !invstd || !workspace) return QVIT_ENULL;
  BnGeo g;
  if (!bn_geo(B, C, H, W, 0, true, &g)) return QVIT_EINVAL;
  if (!(eps >= 0.0) || workspace_bytes < qvit_bn_stats_workspace_bytes(B, C, H, W)) return QVIT_EINVAL;
  if (qvit_misaligned(3, x, mean, var, invstd, running_mean, running_var) || qvit_misaligned(7, workspace))
    return QVIT_EALIGN;
  double* partials = static_cast<double*>(workspace);
  const int vec = vec_arm(g, false, {x}, nullptr);
  hipLaunchKernelGGL(bn_stats_partial_kernel, dim3((unsigned)((int64_t)g.B * g.C * g.S)), dim3(kThreads), 0, stream,
                     x, g, vec, partials);
  hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((unsigned)g.C), dim3(kThreads), 0, stream, partials, x, g, eps,
                     factor, running_mean, running_var, mean, var, invstd);
  return qvit_launch_status();
}

int qvit_bn_act_pool_forward(const float* x, int64_t B, int64_t C, int64_t H, int64_t W, const float* mean,
                             const float* invstd, const float* gamma, const float* beta, int levels, int pool,
                             float* out, uint8_t* flags, hipStream_t stream) {
  if (!x || !mean || !invstd || !out || !flags) return QVIT_ENULL;
  BnGeo g;
  if (!bn_geo(B, C, H, W, pool, false, &g)) return QVIT_EINVAL;
  if (levels < 1 || levels > 127) return QVIT_EINVAL;
  if (qvit_misaligned(3, x, mean, invstd, gamma, beta, out)) return QVIT_EALIGN;
  const dim3 grid((unsigned)((int64_t)g.B * g.C * g.S));
  const int vec = vec_arm(g, pool != 0, {x, out}, flags);
  if (pool)
    hipLaunchKernelGGL(bn_act_pool_forward_kernel, grid, dim3(kThreads), 0, stream, x, g, vec, mean, invstd, gamma,
                       beta, levels, out, flags);
  else
    hipLaunchKernelGGL(bn_act_forward_kernel, grid, dim3(kThreads), 0, stream, x, g, vec, mean, invstd, gamma, beta,
                       levels, out, flags);
  return qvit_launch_status();
}

int64_t qvit_bn_act_pool_backward_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int pool) {
  BnGeo g;
  if (!bn_geo(B, C, H, W, pool, false, &g)) return QVIT_EINVAL;
  return (int64_t)g.C * g.B * g.S * 2 * (int64_t)sizeof(double);
}

int qvit_bn_act_pool_backward_reduce(const float* x, const float* grad_out, const uint8_t* flags, int64_t B,
                                     int64_t C, int64_t H, int64_t W, const float* mean, const float* invstd,
                                     int pool, double* sums, void* workspace, int64_t workspace_bytes,
                                     hipStream_t stream) {
  if (!x || !grad_out || !flags || !mean || !invstd || !sums || !workspace) return QVIT_ENULL;
  BnGeo g;
  if (!bn_geo(B, C, H, W, pool, false, &g)) return QVIT_EINVAL;
  if (workspace_bytes < qvit_bn_act_pool_backward_workspace_bytes(B, C, H, W, pool)) return QVIT_EINVAL;
  if (qvit_misaligned(3, x, grad_out, mean, invstd) || qvit_misaligned(7, sums, workspace)) return QVIT_EALIGN;
  double* partials = static_cast<double*>(workspace);
  const dim3 grid((unsigned)((int64_t)g.B * g.C * g.S));
  const int vec = vec_arm(g, pool != 0, {x, grad_out}, flags);
  if (pool)
    hipLaunchKernelGGL(bn_act_pool_reduce_kernel, grid, dim3(kThreads), 0, stream, x, grad_out, flags, g, vec, mean,
                       invstd, partials);
  else
    hipLaunchKernelGGL(bn_act_reduce_kernel, grid, dim3(kThreads), 0, stream, x, grad_out, flags, g, vec, mean,
                       invstd, partials);
  hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((unsigned)g.C), dim3(kThreads), 0, stream, partials, g, sums);
  return qvit_launch_status();
}

int qvit_bn_act_pool_backward_dx(const float* x, const float* grad_out, const uint8_t* flags, int64_t B, int64_t C,
                                 int64_t H, int64_t W, const float* mean, const float* invstd, const float* gamma,
                                 const double* sums, int pool, float* dx, float* dgamma, float* dbeta,
                                 hipStream_t stream) {
  if (!x || !grad_out || !flags || !mean || !invstd || !sums || !dx) return QVIT_ENULL;
  BnGeo g;
  if (!bn_geo(B, C, H, W, pool, false, &g)) return QVIT_EINVAL;
  if (qvit_misaligned(3, x, grad_out, mean, invstd, gamma, dx, dgamma, dbeta) || qvit_misaligned(7, sums))
    return QVIT_EALIGN;
  const dim3 grid((unsigned)((int64_t)g.B * g.C * g.S));
  const int vec = vec_arm(g, pool != 0, {x, grad_out, dx}, flags);
  if (pool)
    hipLaunchKernelGGL(bn_act_pool_dx_kernel, grid, dim3(kThreads), 0, stream, x, grad_out, flags, g, vec, mean,
                       invstd, gamma, sums, dx, dgamma, dbeta);
  else
    hipLaunchKernelGGL(bn_act_dx_kernel, grid, dim3(kThreads), 0, stream, x, grad_out, flags, g, vec, mean, invstd,
                       gamma, sums, dx, dgamma, dbeta);
  return qvit_launch_status();
}

}  // extern "C"
