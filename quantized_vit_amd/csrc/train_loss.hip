// The training objective of the reference (QViT_with_GETA/utils.py, train_one_epoch :197-325 and evaluate :328-366)
// on the device, in two launches (qvit_train_loss): cross-entropy against the label-smoothed, mixed-up one-hot target
// (one_hot :120-130, mixup_func :142-154 on the targets, cross_entropy_onehot_target :133-139), the distillation term
// kl_div(log_softmax(pred / T), softmax(teacher / T), 'batchmean') T^2 blended as (1 - alpha) CE + alpha KD
// (:268-280), the correct-prediction count (:261-262), and the gradient with respect to the logits. No [B, C]
// temporary exists: the target is two labels and a weight, never a tensor.
//
// Work split: one workgroup of 256 threads owns one row of C logits. The batches the reference trains with (128,
// 256) then give about one workgroup per CU, a thread of a 1000-class row holds one 16-byte vector of it, and the
// row's reductions cost two to four barriers. A wave per row would save the barriers but leaves three quarters of the CUs
// idle at those batches and multiplies the loads a lane issues back to back by four; rows short enough for it to pay
// (CIFAR's 10 classes) are bounded by the launch either way.
//
// Data movement: thread t takes the 4-element vectors t, t + 256, ... of the row, kTile = 4 of them per step, all
// loads of a step issued before the first is used. A row of at most kResident = 4096 classes is one step: it stays
// in registers (16 student and 16 teacher values per thread) from the reductions to the gradient, so it is read once.
// A longer row (the 21843 classes of the in21k heads) is read twice: one online pass (running maximum, sums rescaled
// when it moves), one pass for the gradient. Bytes per row: 4C student + 4C teacher read and 4C gradient written,
// plus 4C + 4C for the second read beyond kResident.
//
// A vector is one 16-byte access when the row bases and strides allow it and the vector lies inside the row, else
// four 4-byte accesses; both feed the same per-element function, thread and order, so the arm changes no bit.
//
// Reductions: fp32 per thread (at most 88 elements at C = 21843), rescaled to the row maximum, then double through
// the fixed-order wave / workgroup tree of reduce_common.h; thread 0 finishes the row in double and leaves
// (ce_row, kd_row, correct, bad label) in the workspace. A second launch of one workgroup folds the rows in index
// order in double. No atomics: the same call gives the same bits, with or without the gradient.
//
// Argmax: the lowest index attaining the maximum, -0 equal to +0, a NaN above everything (the first NaN wins):
// torch.max(pred, dim=1)[1]. A label outside [0, C) never indexes memory: it matches no class, adds nothing to the
// target, makes the row incorrect and is counted.
#include <math.h>

#include "reduce_common.h"

namespace {

constexpr int kTile = 4;                               // vectors of a thread per step
constexpr int kResident = kThreads * kTile * kVec;     // classes of a row held in registers: 4096
constexpr int64_t kMaxRows = (int64_t)1 << 24;         // the counts leave as fp32: exact up to here
constexpr int64_t kMaxCols = (int64_t)1 << 30;
constexpr int kRowSlots = 4;                           // doubles per row in the workspace

struct LossArgs {
  const float* s;        // student logits [B][lds]
  const float* t;        // teacher logits [B][ldt] (KD only)
  const int64_t* la;     // hard labels [B]
  const int64_t* lb;     // mixup partners [B], or NULL
  float* g;              // dlogits [B][ldg], or NULL
  int64_t lds, ldt, ldg;
  int C;
  int vec;               // every row base and stride 16-byte aligned
  float gamma, v0, dv;   // target: v0 + dv (gamma [c == a] + (1 - gamma) [c == b])
  float inv_t;           // 1 / T
  float w_ce, w_kd;      // (1 - alpha) / B (or 1 / B), alpha T / B
  double T;
};

// per-thread state of the row pass
struct Acc {
  float m, z1, z2, sum;       // running max of s; sum exp(s - m), sum exp((s - m) / T), sum s
  float mt, zt, a;            // running max of t; sum exp((t - mt) / T), sum exp((t - mt) / T) (t - s)
  unsigned long long key;     // (ordered bits of the largest s so far, ~index): the maximum is the argmax
};

// x as an unsigned key that orders like torch.max: -0 == +0, NaN on top
QVIT_DEV uint32_t order_key(float x) {
  const uint32_t b = __float_as_uint(x + 0.f);
  const uint32_t k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (x != x) ? 0xffffffffu : k;
}

// One element of the row: the per-element function of both arms.
template <bool KD>
QVIT_DEV void acc_element(Acc& r, float s, float t, int c, float inv_t) {
  const unsigned long long key = ((unsigned long long)order_key(s) << 32) | (uint32_t)~(uint32_t)c;
  r.key = key > r.key ? key : r.key;
  r.sum += s;
  if (s > r.m) {   // the maximum moved: bring the sums to it (rare after a thread's first few elements)
    r.z1 *= expf(r.m - s);
    r.z2 *= expf((r.m - s) * inv_t);
    r.m = s;
  }
  r.z1 += expf(s - r.m);
  r.z2 += expf((s - r.m) * inv_t);
  if (KD) {
    if (t > r.mt) {
      const float f = expf((r.mt - t) * inv_t);
      r.zt *= f;
      r.a *= f;
      r.mt = t;
    }
    const float e = expf((t - r.mt) * inv_t);
    r.zt += e;
    r.a = fmaf(e, t - s, r.a);
  }
}

// what the gradient pass needs of the finished row, the same in every thread
struct RowStats {
  float m, inv_z1, inv_z2, mt, inv_zt;
  int a, b;   // the labels, -1 where out of range
};

template <bool KD>
QVIT_DEV float grad_element(const LossArgs& p, const RowStats& q, float s, float t, int c) {
  const float y = p.v0 + p.dv * ((c == q.a ? p.gamma : 0.f) + (c == q.b ? 1.f - p.gamma : 0.f));
  float g = p.w_ce * (expf(s - q.m) * q.inv_z1 - y);
  if (KD) g += p.w_kd * (expf((s - q.m) * p.inv_t) * q.inv_z2 - expf((t - q.mt) * p.inv_t) * q.inv_zt);
  return g;
}

// The 4 elements from column c0 of a row: one 16-byte load, or the in-row elements one by one (the others stay 0
// and are never used).
QVIT_DEV float4 load_vec(const float* row, int c0, int C, bool vec) {
  if (vec && c0 + kVec <= C) return *reinterpret_cast<const float4*>(row + c0);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c0 < C) v.x = row[c0];
  if (c0 + 1 < C) v.y = row[c0 + 1];
  if (c0 + 2 < C) v.z = row[c0 + 2];
  if (c0 + 3 < C) v.w = row[c0 + 3];
  return v;
}
QVIT_DEV void store_vec(float* row, int c0, int C, bool vec, float4 v) {
  if (vec && c0 + kVec <= C) {
    *reinterpret_cast<float4*>(row + c0) = v;
    return;
  }
  if (c0 < C) row[c0] = v.x;
  if (c0 + 1 < C) row[c0 + 1] = v.y;
  if (c0 + 2 < C) row[c0 + 2] = v.z;
  if (c0 + 3 < C) row[c0 + 3] = v.w;
}

// one step of a thread: the vectors j0, j0 + 256, ... (kTile of them) of the student and teacher rows
template <bool KD>
QVIT_DEV void load_tile(const LossArgs& p, const float* srow, const float* trow, int j0, float4 (&sv)[kTile],
                        float4 (&tv)[kTile]) {
#pragma unroll
  for (int u = 0; u < kTile; ++u) {
    const int c0 = (j0 + u * kThreads) * kVec;
    sv[u] = load_vec(srow, c0, p.C, p.vec);
    tv[u] = KD ? load_vec(trow, c0, p.C, p.vec) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

template <bool KD>
QVIT_DEV void acc_tile(const LossArgs& p, Acc& r, int j0, const float4 (&sv)[kTile], const float4 (&tv)[kTile]) {
#pragma unroll
  for (int u = 0; u < kTile; ++u) {
    const int c0 = (j0 + u * kThreads) * kVec;
    if (c0 < p.C) acc_element<KD>(r, sv[u].x, tv[u].x, c0, p.inv_t);
    if (c0 + 1 < p.C) acc_element<KD>(r, sv[u].y, tv[u].y, c0 + 1, p.inv_t);
    if (c0 + 2 < p.C) acc_element<KD>(r, sv[u].z, tv[u].z, c0 + 2, p.inv_t);
    if (c0 + 3 < p.C) acc_element<KD>(r, sv[u].w, tv[u].w, c0 + 3, p.inv_t);
  }
}

template <bool KD>
QVIT_DEV void grad_tile(const LossArgs& p, const RowStats& q, float* grow, int j0, const float4 (&sv)[kTile],
                        const float4 (&tv)[kTile]) {
#pragma unroll
  for (int u = 0; u < kTile; ++u) {
    const int c0 = (j0 + u * kThreads) * kVec;
    if (c0 >= p.C) continue;
    float4 g;   // (columns >= C of the last vector are computed from zeros and never stored)
    g.x = grad_element<KD>(p, q, sv[u].x, tv[u].x, c0);
    g.y = grad_element<KD>(p, q, sv[u].y, tv[u].y, c0 + 1);
    g.z = grad_element<KD>(p, q, sv[u].z, tv[u].z, c0 + 2);
    g.w = grad_element<KD>(p, q, sv[u].w, tv[u].w, c0 + 3);
    store_vec(grow, c0, p.C, p.vec, g);
  }
}

// wave64 maximum, every lane holds it
QVIT_DEV float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
QVIT_DEV unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

template <bool KD>
__global__ __launch_bounds__(kThreads) void train_loss_row_kernel(LossArgs p, double* __restrict__ rows) {
  __shared__ float lds_m[kWaves][2];
  __shared__ unsigned long long lds_key[kWaves];
  __shared__ double lds_a[kWaves][3], lds_b[kWaves][3];
  __shared__ RowStats lds_q;
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* srow = p.s + row * p.lds;
  const float* trow = KD ? p.t + row * p.ldt : nullptr;
  const int nvec = (p.C + kVec - 1) / kVec;
  const bool resident = p.C <= kResident;

  Acc r;
  r.m = r.mt = -INFINITY;
  r.z1 = r.z2 = r.sum = r.zt = r.a = 0.f;
  r.key = 0ull;
  float4 sv[kTile], tv[kTile];
  for (int j0 = tid; j0 < nvec; j0 += kThreads * kTile) {
    load_tile<KD>(p, srow, trow, j0, sv, tv);
    acc_tile<KD>(p, r, j0, sv, tv);
  }

  // the row's maxima and argmax, in every thread
  const float wm = wave_max(r.m), wmt = KD ? wave_max(r.mt) : 0.f;
  const unsigned long long wkey = wave_max(r.key);
  if (lane == 0) {
    lds_m[wave][0] = wm;
    lds_m[wave][1] = wmt;
    lds_key[wave] = wkey;
  }
  __syncthreads();
  float M = lds_m[0][0], Mt = lds_m[0][1];
  unsigned long long key = lds_key[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    M = fmaxf(M, lds_m[w][0]);
    Mt = fmaxf(Mt, lds_m[w][1]);
    key = lds_key[w] > key ? lds_key[w] : key;
  }
  // the thread's sums against the row maxima (a thread without elements holds zeros; its -inf maximum must not
  // meet an infinite row maximum in a difference)
  const float d1 = r.m > -INFINITY ? r.m - M : -INFINITY;
  const float dt = (KD && r.mt > -INFINITY) ? r.mt - Mt : -INFINITY;
  const float ft = KD ? expf(dt * p.inv_t) : 0.f;
  double z1 = (double)(r.z1 * expf(d1)), z2 = (double)(r.z2 * expf(d1 * p.inv_t)), sum = (double)r.sum;
  double zt = (double)(r.zt * ft), a = (double)(r.a * ft), unused = 0.0;
  block_sum3(z1, z2, sum, lds_a);
  if (KD) block_sum3(zt, a, unused, lds_b);   // (its own slots: thread 0 may still be reading lds_a)

  if (tid == 0) {
    const int64_t la = p.la[row], lb = p.lb ? p.lb[row] : la;
    const bool a_ok = la >= 0 && la < p.C, b_ok = lb >= 0 && lb < p.C;
    const double sa = a_ok ? (double)srow[la] : 0.0, sb = b_ok ? (double)srow[lb] : 0.0;
    const double ga = a_ok ? (double)p.gamma : 0.0, gb = b_ok ? 1.0 - (double)p.gamma : 0.0;
    const double lse = (double)M + log(z1);
    const double ce = lse - ((double)p.v0 * sum + (double)p.dv * (ga * sa + gb * sb));
    double kd = 0.0;
    if (KD) kd = a / (zt * p.T) - ((double)Mt / p.T + log(zt)) + ((double)M / p.T + log(z2));
    const int argmax = (int)~(uint32_t)key;
    double* out = rows + row * kRowSlots;
    out[0] = ce;
    out[1] = kd;
    out[2] = (a_ok && argmax == (int)la) ? 1.0 : 0.0;
    out[3] = (a_ok && b_ok) ? 0.0 : 1.0;
    lds_q.m = M;
    lds_q.inv_z1 = (float)(1.0 / z1);
    lds_q.inv_z2 = (float)(1.0 / z2);
    lds_q.mt = Mt;
    lds_q.inv_zt = KD ? (float)(1.0 / zt) : 0.f;
    lds_q.a = a_ok ? (int)la : -1;
    lds_q.b = b_ok ? (int)lb : -1;
  }
  if (!p.g) return;   // the no-gradient form: the same reads and reductions, nothing more
  __syncthreads();
  const RowStats q = lds_q;
  float* grow = p.g + row * p.ldg;
  for (int j0 = tid; j0 < nvec; j0 += kThreads * kTile) {
    if (!resident) load_tile<KD>(p, srow, trow, j0, sv, tv);   // (resident: one trip, the registers of the first)
    grad_tile<KD>(p, q, grow, j0, sv, tv);
  }
}

// One workgroup folds the B rows in index order, in double: out = (loss, mean CE, KD, correct, bad labels).
__global__ __launch_bounds__(kThreads) void train_loss_finish_kernel(const double* __restrict__ rows, int B, int kd_on,
                                                                     double alpha, double T,
                                                                     float* __restrict__ out) {
  __shared__ double lds_a[kWaves][3], lds_b[kWaves][3];
  double ce = 0.0, kd = 0.0, ok = 0.0, bad = 0.0, u0 = 0.0, u1 = 0.0;
  for (int j = threadIdx.x; j < B; j += kThreads) {   // thread i: rows i, i + 256, ... in that order
    const double* r = rows + (int64_t)j * kRowSlots;
    ce += r[0];
    kd += r[1];
    ok += r[2];
    bad += r[3];
  }
  block_sum3(ce, kd, ok, lds_a);
  block_sum3(bad, u0, u1, lds_b);
  if (threadIdx.x == 0) {
    const double ce_mean = ce / (double)B, kd_mean = kd / (double)B * (T * T);   // 'batchmean', times T^2 (:274)
    out[0] = (float)(kd_on ? (1.0 - alpha) * ce_mean + alpha * kd_mean : ce_mean);   // :278, :280
    out[1] = (float)ce_mean;
    out[2] = (float)kd_mean;
    out[3] = (float)ok;
    out[4] = (float)bad;
  }
}

inline bool in_unit(float v) { return v >= 0.f && v <= 1.f; }   // (false for a NaN)

}  // namespace

extern "C" {

int64_t qvit_train_loss_workspace_bytes(int64_t B) {
  if (B < 0 || B > kMaxRows) return QVIT_EINVAL;
  return B * kRowSlots * (int64_t)sizeof(double);
}

int qvit_train_loss(const float* logits, int64_t B, int64_t C, int64_t lds, const float* teacher, int64_t ldt,
                    const int64_t* label_a, const int64_t* label_b, float gamma, float eps, float kd_alpha, float T,
                    float* dlogits, int64_t ldg, float* out, void* workspace, int64_t workspace_bytes,
                    hipStream_t stream) {
  if (!logits || !label_a || !out || !workspace) return QVIT_ENULL;
  if (B < 0 || B > kMaxRows || C < 1 || C > kMaxCols) return QVIT_EINVAL;
  if (lds < C || (teacher && ldt < C) || (dlogits && ldg < C)) return QVIT_EINVAL;
  if (!(T > 0.f) || !(T < INFINITY)) return QVIT_EINVAL;
  if (!in_unit(eps) || !in_unit(gamma) || !in_unit(kd_alpha)) return QVIT_EINVAL;
  if (workspace_bytes < qvit_train_loss_workspace_bytes(B)) return QVIT_EINVAL;
  if (qvit_misaligned(3, logits, teacher, dlogits, out) || qvit_misaligned(7, label_a, label_b) ||
      qvit_misaligned(7, workspace))
    return QVIT_EALIGN;
  if (B == 0) return QVIT_OK;

  const bool kd = teacher && kd_alpha > 0.f;
  LossArgs p;
  p.s = logits;
  p.t = kd ? teacher : nullptr;
  p.la = label_a;
  p.lb = label_b;
  p.g = dlogits;
  p.lds = lds;
  p.ldt = ldt;
  p.ldg = ldg;
  p.C = (int)C;
  p.vec = !qvit_misaligned(15, logits, p.t, dlogits) && lds % kVec == 0 && (!kd || ldt % kVec == 0) &&
          (!dlogits || ldg % kVec == 0);
  p.gamma = label_b ? gamma : 1.f;
  const double v0 = (double)eps / (double)C, v1 = 1.0 - (double)eps + v0;   // one_hot :127-128, in double as there
  p.v0 = (float)v0;
  p.dv = (float)(v1 - v0);                                                   // :129
  p.inv_t = 1.f / T;
  p.w_ce = (kd ? 1.f - kd_alpha : 1.f) / (float)B;
  p.w_kd = kd ? kd_alpha * T / (float)B : 0.f;
  p.T = (double)T;
  double* rows = static_cast<double*>(workspace);
  if (kd) hipLaunchKernelGGL(train_loss_row_kernel<true>, dim3((unsigned)B), dim3(kThreads), 0, stream, p, rows);
  else hipLaunchKernelGGL(train_loss_row_kernel<false>, dim3((unsigned)B), dim3(kThreads), 0, stream, p, rows);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return qvit_hip_status(e);
  hipLaunchKernelGGL(train_loss_finish_kernel, dim3(1), dim3(kThreads), 0, stream, rows, (int)B, (int)kd,
                     (double)kd_alpha, (double)T, out);
  return qvit_launch_status();
}

}  // extern "C"
