// Quantization error of one tensor under many candidate quantizers (qvit_quant_error), for an error-minimising
// clip search: err[c] = sum (p - fake_quant(x; d[c], q_m[c], t))^2 and nclip[c] = #{|x| >= q_m[c]} for up to 64
// candidates from one launch pair, instead of one qvit_fake_quant_f32 pass plus a torch reduction per candidate.
//
// Per element the kernel takes the careful power pw = p(|x|) once (it depends on t alone: |x| for the linear type,
// exp_cr(t * log_cr(|x|)) for the nonlinear one, the un-rounded input_pow of quant_layers.py:63) and the target
// sgn(x) pw (x itself for the linear type); per candidate it then costs one IEEE division, the masks, and three
// double operations (quant_code_from_pow, qvit_common.h: the forward's code for every x).
//
// Blocking: a workgroup scores kCandBlock = 16 candidates (16 double sums and 16 counts per thread stay in
// registers); grid.y walks the candidate blocks and re-reads x, which a second block finds in L2 / MALL. The work
// per element (about 25 instructions per candidate, plus the double-precision log and exp of the nonlinear target)
// outweighs the read by far, so the re-read is not what bounds the kernel.
//
// Reduction (reduce_common.h): per-thread double accumulation, the fixed-order wave / workgroup tree, one
// (err, count) pair per workgroup and candidate in the workspace as partial [candidate][workgroup], and a fold
// kernel of one workgroup per candidate that adds them in index order and applies `accumulate`. Counts travel as
// doubles (integers below 2^53: exact in any order). No atomics; the same call gives the same bits.
#include "reduce_common.h"

namespace {

constexpr int kCandBlock = 16;
constexpr int kMaxCand = 64;
constexpr int64_t kMaxExtent = (int64_t)1 << 48;   // rows * ldx: a thread's count then fits 32 bits, a sum's 53

// One element against the block's candidates.
template <bool NONLINEAR>
QVIT_DEV void score_element(float x, float t, const float (&cd)[kCandBlock], const float (&cq)[kCandBlock],
                            const float (&cl)[kCandBlock], double (&err)[kCandBlock], uint32_t (&cnt)[kCandBlock]) {
  const float a = fabsf(x);
  float pw = a, target = x;
  if (NONLINEAR) {
    pw = exp_cr(t * log_cr(a));
    const float sgn = (float)(x > 0.f) - (float)(x < 0.f);   // torch.sign: 0 at 0 and at NaN (0 * NaN stays NaN)
    target = sgn * pw;
  }
  const double tp = (double)target;
#pragma unroll
  for (int j = 0; j < kCandBlock; ++j) {
    QParams p;
    p.d = cd[j];
    p.qm = cq[j];
    p.L = cl[j];
    const float fq = p.d * quant_code_from_pow(x, pw, p);   // fake_quant_value's d * k
    const double dd = tp - (double)fq;
    err[j] = fma(dd, dd, err[j]);
    cnt[j] += (a >= p.qm) ? 1u : 0u;
  }
}

// One thread = 4 consecutive elements of the logical [rows][cols] tensor per step, in both arms: VEC reads them as
// one 16-byte load (cols % 4 == 0 keeps them in one row), the scalar arm finds each element's row by itself. The
// element-to-thread map, and so every bit of the result, is the same in both. I: the index type (int when
// rows * ldx fits, the rule of qvit_im2col_quant_i8).
template <bool NONLINEAR, bool VEC, typename I>
__global__ __launch_bounds__(kThreads) void quant_error_kernel(const float* __restrict__ x, int64_t rows_,
                                                               int64_t cols_, int64_t ldx_, int qtype,
                                                               const float* __restrict__ d,
                                                               const float* __restrict__ qm, const float* t,
                                                               int ncand, double* __restrict__ partials) {
  __shared__ double lds[kCandBlock][kWaves][3];
  __shared__ float sat[kCandBlock];
  const I rows = (I)rows_, cols = (I)cols_, ldx = (I)ldx_;
  const int c0 = blockIdx.y * kCandBlock;
  // the saturation codes, one thread per candidate (load_qparams: the forward's L); a block past ncand repeats
  // the last candidate and stores nothing for it
  if (threadIdx.x < kCandBlock) {
    const int c = min(c0 + (int)threadIdx.x, ncand - 1);
    sat[threadIdx.x] = load_qparams(qtype, d + c, qm + c, t, 0).L;
  }
  __syncthreads();
  const float tq = NONLINEAR ? *t : 1.f;
  float cd[kCandBlock], cq[kCandBlock], cl[kCandBlock];
  double err[kCandBlock];
  uint32_t cnt[kCandBlock];
#pragma unroll
  for (int j = 0; j < kCandBlock; ++j) {
    const int c = min(c0 + j, ncand - 1);
    cd[j] = d[c];
    cq[j] = qm[c];
    cl[j] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sat[j])));
    err[j] = 0.0;
    cnt[j] = 0u;
  }

  const I n = rows * cols;
  const I units = (n + (kVec - 1)) / kVec;
  for (I id = blockIdx.x * (I)kThreads + threadIdx.x; id < units; id += (I)gridDim.x * kThreads) {
    const I e0 = id * kVec;
    if (VEC) {
      const I r = e0 / cols, c = e0 - r * cols;
      const float4 f = *reinterpret_cast<const float4*>(x + (r * ldx + c));
      score_element<NONLINEAR>(f.x, tq, cd, cq, cl, err, cnt);
      score_element<NONLINEAR>(f.y, tq, cd, cq, cl, err, cnt);
      score_element<NONLINEAR>(f.z, tq, cd, cq, cl, err, cnt);
      score_element<NONLINEAR>(f.w, tq, cd, cq, cl, err, cnt);
    } else {
#pragma unroll 1
      for (int i = 0; i < kVec; ++i) {
        const I e = e0 + i;
        if (e < n) {
          const I r = e / cols, c = e - r * cols;
          score_element<NONLINEAR>(x[r * ldx + c], tq, cd, cq, cl, err, cnt);
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < kCandBlock; ++j) {
    double s = err[j], k = (double)cnt[j], unused = 0.0;
    block_sum3(s, k, unused, lds[j]);
    if (threadIdx.x == 0 && c0 + j < ncand)
      store_partial2(partials, (int64_t)(c0 + j) * gridDim.x + blockIdx.x, s, k);
  }
}

// One workgroup per candidate folds its nblocks partial pairs (fold_partials2) and writes or adds the totals.
__global__ __launch_bounds__(kThreads) void quant_error_fold_kernel(const double* __restrict__ partials, int nblocks,
                                                                    int accumulate, double* err, int64_t* nclip) {
  __shared__ double lds[kWaves][3];
  const int c = blockIdx.x;
  double s = 0.0, k = 0.0;
  fold_partials2(partials + 2 * (int64_t)c * nblocks, nblocks, s, k, lds);
  if (threadIdx.x == 0) {
    err[c] = accumulate ? err[c] + s : s;
    nclip[c] = (accumulate ? nclip[c] : (int64_t)0) + (int64_t)k;
  }
}

// the size rules shared by the entry point and its workspace query
inline bool quant_error_sizes_ok(int64_t rows, int64_t cols, int64_t ld, int ncand) {
  if (ncand < 1 || ncand > kMaxCand || rows < 0 || cols < 0 || ld < cols) return false;
  return rows == 0 || ld <= kMaxExtent / rows;
}

template <bool NONLINEAR, bool VEC, typename I>
void launch_quant_error(dim3 grid, hipStream_t stream, const float* x, int64_t rows, int64_t cols, int64_t ldx,
                        int qtype, const float* d, const float* qm, const float* t, int ncand, double* partials) {
  hipLaunchKernelGGL((quant_error_kernel<NONLINEAR, VEC, I>), grid, dim3(kThreads), 0, stream, x, rows, cols, ldx,
                     qtype, d, qm, t, ncand, partials);
}

}  // namespace

extern "C" {

int64_t qvit_quant_error_workspace_bytes(int64_t rows, int64_t cols, int ncand) {
  if (!quant_error_sizes_ok(rows, cols, cols, ncand)) return QVIT_EINVAL;
  return (int64_t)stream_grid(rows * cols, kVec) * ncand * 2 * (int64_t)sizeof(double);
}

int qvit_quant_error(const float* x, int64_t rows, int64_t cols, int64_t ldx, int qtype, const float* d,
                     const float* q_m, const float* t, int ncand, int accumulate, double* err, int64_t* nclip,
                     void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  if (!d || !q_m || !err || !nclip || !workspace) return QVIT_ENULL;
  // (a tensor quantizer: ULTRA_ACT, which has no d and no q_m to search, is none)
  if ((qtype & 0xff) == QVIT_QT_ULTRA_ACT || qvit_quant_status(qtype, d, q_m, 0)) return QVIT_EINVAL;
  const bool nonlinear = (qtype & 0xff) == QVIT_QT_NONLINEAR;
  if (nonlinear && !t) return QVIT_ENULL;
  if (!quant_error_sizes_ok(rows, cols, ldx, ncand)) return QVIT_EINVAL;
  if (workspace_bytes < qvit_quant_error_workspace_bytes(rows, cols, ncand)) return QVIT_EINVAL;
  const int64_t n = rows * cols;
  if (!x && n > 0) return QVIT_ENULL;
  if (qvit_misaligned(3, x, d, q_m, t) || qvit_misaligned(7, err, nclip) || qvit_misaligned(7, workspace))
    return QVIT_EALIGN;
  if (n == 0 && accumulate) return QVIT_OK;

  double* partials = static_cast<double*>(workspace);
  int nblocks = 0;
  if (n > 0) {
    nblocks = stream_grid(n, kVec);
    const dim3 grid(nblocks, (ncand + kCandBlock - 1) / kCandBlock);
    const bool vec = (cols % kVec == 0) && (ldx % kVec == 0) && !qvit_misaligned(15, x);
    const int64_t lim = (int64_t)INT32_MAX - 2 * (int64_t)kGridCap * kThreads * kVec;   // headroom: the grid stride
    const bool narrow = rows * ldx < lim;
#define QVIT_QE(NL, VEC)                                                                                       \
  do {                                                                                                         \
    if (narrow) launch_quant_error<NL, VEC, int>(grid, stream, x, rows, cols, ldx, qtype, d, q_m, t, ncand,    \
                                                 partials);                                                    \
    else launch_quant_error<NL, VEC, int64_t>(grid, stream, x, rows, cols, ldx, qtype, d, q_m, t, ncand,       \
                                              partials);                                                       \
  } while (0)
    if (nonlinear) {
      if (vec) QVIT_QE(true, true);
      else QVIT_QE(true, false);
    } else {
      if (vec) QVIT_QE(false, true);
      else QVIT_QE(false, false);
    }
#undef QVIT_QE
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return qvit_hip_status(e);
  }
  hipLaunchKernelGGL(quant_error_fold_kernel, dim3(ncand), dim3(kThreads), 0, stream, partials, nblocks, accumulate,
                     err, nclip);
  return qvit_launch_status();
}

}  // extern "C"
