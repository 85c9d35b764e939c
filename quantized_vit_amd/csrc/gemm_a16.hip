// Exact integer GEMM for activation codes of 9 to 16 bits (QuantizeLinear.forward, quant_layers.py:495-499, in
// WEIGHT_AND_ACTIVATION mode with 128 <= L_act <= 32767: the reference's default num_bits = 16 and every stage of a
// QAT run while a layer's activations are wider than int8):
//   Y[m][n] = d_act d_wt sum_k k_a[m][k] k_w[n][k] + bias[n]
// Both operands are integers, so both are contracted as int8 digits on v_mfma_i32_16x16x64_i8.
//   activations  k_a in [-32768, 32767] = 256 hi + lo + 128 with hi = k_a >> 8 (arithmetic) and lo = (k_a & 255) - 128,
//                both in [-128, 127] (balanced digits cannot hold 32767 = L at num_bits = 16): two int8 planes
//                [2][M][lda], hi first, written by qvit_quantize_act_i16;
//   weights      the plan's image as qvit_gemm_wonly takes it: D = 1 (QVIT_W8, QVIT_W4), 2 (QVIT_W16) or 3 (QVIT_W24)
//                balanced base-256 digits w_q in [-128, 127], most significant first, one QVIT_W8 image each. QVIT_W4
//                stays packed in LDS and is unpacked after the fragment read to the byte 16 w (the nibble in the high
//                half); 1 / 16 is folded into the scale.
//   S = sum_k k_a k_w = sum_c 256^c C_c + 128 sum_k k_w[n][k],   C_c = hi . w_(c-1) + lo . w_(c)   (c = 0 .. D,
//   w_(e) the digit of weight 256^e, a missing digit zero): D + 1 int32 accumulator sets, one per power of 256, each
//   taking at most two products per k: |C_c| <= 2 K 2^14 <= 2^30 for K <= A16_MAX_K = 32768. The last term is the
//   activation digits' offset; sum_k k_w[n][k] per output column comes from qvit_weight_code_sums (once per weight
//   image, int64). The epilogue combines S exactly in int64 (|S| < 2^54), converts it to fp64 (exact below 2^53,
//   which no layer's codes exceed; correctly rounded above), multiplies by the fp64 product d_act d_wt (exact: 48
//   bits), adds the bias in fp64 and rounds to fp32 once: |y - y_exact| <= 2^-24 |y| + 2^-52 (|d_act d_wt S| + |bias|).
//
// Geometry (gemm_wonly.hip's): one workgroup (4 waves) per 256 (weight rows) x BM (activation rows) tile, BM = 64, or
// 32 with three weight digits; wave w owns weight rows [64 w, 64 w + 64) and all BM activation rows: 4 x BM / 16 MFMA
// tiles per class, 128 (W4, W8, W24) or 192 (W16) accumulator registers (64 rows with four classes would need 256:
// measured at compile time, they spill).
// Pipeline (gemm_w4a8.hip's ring idiom): K advances in 64-deep stages through an LDS ring of 3 slots (2 for QVIT_W24:
// a slot is 2 BM * 64 B of activation digits + D * 16 KiB of weight digits). Everything goes HBM / L2 -> LDS with
// global_load_lds_dwordx4 issued from asm, RING - 1 stages ahead; one counted s_waitcnt vmcnt + barrier per stage.
// The packed weight tile of a (tile_n, stage) IS the LDS image (XOR-swizzled for conflict-free ds_read_b128), staged as
// contiguous 1-KiB pieces; the activation planes are swizzled through the per-lane source address (16-B chunk c of row
// r at c ^ (((r >> 2) & 1) << 1)). Per stage a wave reads its 4 D weight fragments once and, per 16 activation rows,
// the hi and the lo fragment once: every weight fragment meets both activation digits, every activation fragment
// every weight digit (8 D MFMAs per 2 activation reads).
// MFMA operands as in qvit_gemm: A = weights (16 packed rows), B = activations; lane (fr, fq) holds
// acc[c][r][s][j] = C_c[m0 + 16 s + fr][n0 + 64 w + 16 fq + 4 r + j] (the packed rows are pre-permuted).
// Rows past M are clamped to row M - 1 on the load and never stored. No atomics, a fixed order: the same call gives
// the same bits. Small M launches fewer tiles (no split-K).
#include "qvit_common.h"
#include "reduce_common.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int A16_BN = 256;                 // weight rows per tile (one packed tile_n)
constexpr int A16_BK = 64;                  // k per stage
constexpr int A16_MAX_K = 32768;            // |C_c| <= 2 K 2^14 stays below 2^31

template <int WFMT>
struct A16Geo {
  static constexpr int D = WFMT == QVIT_W24 ? 3 : WFMT == QVIT_W16 ? 2 : 1;   // weight digits
  static constexpr int SM = D == 3 ? 2 : 4;                  // 16-row activation tiles per wave: (D + 1) SM <= 12
  static constexpr int BM = 16 * SM;                         // activation rows per tile
  static constexpr int XPLANE = BM * A16_BK;                 // one activation digit plane of a stage
  static constexpr int XBYTES = 2 * XPLANE;
  static constexpr int MINB = D == 1 ? 2 : 1;                // workgroups per CU the registers must allow
  static constexpr int WROW = WFMT == QVIT_W4 ? 32 : 64;    // packed bytes per weight row per stage and image
  static constexpr int WBYTES = A16_BN * WROW;               // one image's stage
  static constexpr int STAGE = XBYTES + D * WBYTES;
  static constexpr int RING = D == 3 ? 2 : 3;                // 104 KiB (W24), 120 (W16), 72 (W8), 48 (W4)
  static constexpr int LEAD = RING - 1;                      // stages in flight ahead of the one being read
  static constexpr int XPIECES = XBYTES / 1024 / 4;          // 1-KiB DMA pieces per wave and stage: 2 (W24: 1)
  static constexpr int WPIECES = WBYTES / 1024 / 4;          // per image: 4 (W8) / 2 (W4)
  static constexpr int PIECES = XPIECES + D * WPIECES;       // <= 14: far below the 6-bit vmcnt
};

QVIT_DEV uint32_t a16_nib_lo(uint32_t p) { return (p << 4) & 0xF0F0F0F0u; }
QVIT_DEV uint32_t a16_nib_hi(uint32_t p) { return p & 0xF0F0F0F0u; }

// at most N of this wave's DMA pieces in flight, its LDS reads retired, then the barrier (gemm_w4a8.hip: stage_sync)
template <int N>
QVIT_DEV void a16_stage_sync() {
  __builtin_amdgcn_s_waitcnt(0xC07F);
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

template <int WFMT>
__global__ __launch_bounds__(256, A16Geo<WFMT>::MINB) void gemm_a16_kernel(
    const int8_t* __restrict__ A, int M, int K, int64_t lda, const int8_t* __restrict__ Wp, int N, int npad,
    const float* __restrict__ d_act, const float* __restrict__ d_wt, const float* __restrict__ bias,
    const int64_t* __restrict__ wsum, float* __restrict__ Y, int64_t ldy) {
  using G = A16Geo<WFMT>;
  constexpr int D = G::D, SM = G::SM, BM = G::BM;
  __shared__ __attribute__((aligned(16))) int8_t smem[G::RING * G::STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;

  // tile: XCD x (blocks x, x + 8, ...) walks a contiguous range, weight tiles fastest (one activation panel per L2)
  const int nb_n = npad / A16_BN;
  const int ntiles = nb_n * ((M + BM - 1) / BM);
  const int per = (ntiles + 7) >> 3;
  const int t = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (t >= ntiles) return;
  const int m0 = (t / nb_n) * BM, tn = t % nb_n, n0 = tn * A16_BN;
  const int nk = K / A16_BK;

  // ---- DMA sources (per lane). Activations: piece pi = XPIECES wave + j of the stage's 2 SM is plane pi / SM, rows
  // 16 (pi % SM) .. + 15; lane l stages row l >> 2, LDS chunk position l & 3 = source chunk (l & 3) ^ (row bit 2 << 1)
  // (row bit 2 = lane bit 4: the piece's first row is a multiple of 16). Weights: the packed (tile_n, stage) tile of
  // each digit image is its LDS image; wave w stages the image's pieces WPIECES w .. + WPIECES - 1.
  const int8_t* asrc[G::XPIECES];
#pragma unroll
  for (int j = 0; j < G::XPIECES; ++j) {
    const int pi = G::XPIECES * wave + j, plane = pi / SM;
    const int row = min(m0 + 16 * (pi % SM) + (lane >> 2), M - 1);   // the tail: a valid row, never stored
    asrc[j] = A + ((int64_t)plane * M + row) * lda + (((lane & 3) ^ (((lane >> 4) & 1) << 1)) << 4);
  }
  const int8_t* const wsrc = Wp + (int64_t)tn * nk * G::WBYTES + wave * (G::WPIECES * 1024) + lane * 16;
  const int64_t wpart = (int64_t)npad * K * G::WROW / 64;   // bytes of one digit image
  const uint32_t lds0 = lds_addr(smem);
  auto issue = [&](int kt, int slot) __attribute__((always_inline)) {
    const uint32_t sx = lds0 + (uint32_t)(slot * G::STAGE);
#pragma unroll
    for (int j = 0; j < G::XPIECES; ++j)
      dma16(asrc[j] + kt * A16_BK, __builtin_amdgcn_readfirstlane(sx + (G::XPIECES * wave + j) * 1024));
#pragma unroll
    for (int q = 0; q < D; ++q)
#pragma unroll
      for (int j = 0; j < G::WPIECES; ++j)
        dma16(wsrc + q * wpart + (int64_t)kt * G::WBYTES + j * 1024,
              __builtin_amdgcn_readfirstlane(sx + G::XBYTES + q * G::WBYTES + (G::WPIECES * wave + j) * 1024));
  };

  // fragment offsets inside a slot: weights as qvit_gemm's read_frags, activation planes row 16 s + fr
  const int woff = (WFMT == QVIT_W4) ? (64 * wave + fr) * G::WROW + ((fq ^ (((fr >> 3) & 1) << 1)) << 3)
                                     : (64 * wave + fr) * G::WROW + ((fq ^ (((fr >> 2) & 1) << 1)) << 4);
  const int xoff = fr * A16_BK + ((fq ^ (((fr >> 2) & 1) << 1)) << 4);

  v4i acc[D + 1][4][SM];
#pragma unroll
  for (int c = 0; c <= D; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < SM; ++s) acc[c][r][s] = v4i{0, 0, 0, 0};

#pragma unroll
  for (int j = 0; j < G::LEAD; ++j)
    if (j < nk) issue(j, j);
  for (int kt = 0; kt < nk; ++kt) {
    // stage kt has landed once only the pieces of the stages issued after it are in flight; near the end fewer
    // stages follow, so the count drops to zero. The barrier also retires every wave's reads of stage kt - 1, whose
    // slot the issue below overwrites.
    if (kt + G::LEAD <= nk) a16_stage_sync<G::PIECES * (G::LEAD - 1)>();
    else a16_stage_sync<0>();
    if (kt + G::LEAD < nk) issue(kt + G::LEAD, (kt + G::LEAD) % G::RING);
    const int8_t* sx = smem + (kt % G::RING) * G::STAGE;
    // the wave's weight fragments of this stage: wf[q][r] = digit q (most significant first), rows 16 r .. + 15
    v4i wf[D][4];
#pragma unroll
    for (int q = 0; q < D; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int8_t* wp = sx + G::XBYTES + q * G::WBYTES + woff + r * 16 * G::WROW;
        if (WFMT == QVIT_W4) {
          const uint2 p = *reinterpret_cast<const uint2*>(wp);
          wf[q][r] = v4i{(int)a16_nib_lo(p.x), (int)a16_nib_hi(p.x), (int)a16_nib_lo(p.y), (int)a16_nib_hi(p.y)};
        } else {
          wf[q][r] = *reinterpret_cast<const v4i*>(wp);
        }
      }
#pragma unroll
    for (int s = 0; s < SM; ++s) {
      const v4i xh = *reinterpret_cast<const v4i*>(sx + xoff + s * 16 * A16_BK);
      const v4i xl = *reinterpret_cast<const v4i*>(sx + G::XPLANE + xoff + s * 16 * A16_BK);
#pragma unroll
      for (int q = 0; q < D; ++q) {
        const int e = D - 1 - q;   // the digit's power of 256: lo . w -> class e, hi . w -> class e + 1
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[e][r][s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[q][r], xl, acc[e][r][s], 0, 0, 0);
          acc[e + 1][r][s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[q][r], xh, acc[e + 1][r][s], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: S exactly in int64, one rounding to fp32; 16 contiguous columns per lane and row
  const double alpha = (double)(*d_act) * (double)(*d_wt) * (WFMT == QVIT_W4 ? 0.0625 : 1.0);
  const int nb = n0 + 64 * wave + 16 * fq;   // (< npad: wsum and bias are padded to npad)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int64_t off[4];
    double bcol[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      off[j] = 128 * wsum[nb + 4 * r + j];
      bcol[j] = bias ? (double)bias[nb + 4 * r + j] : 0.0;
    }
    const int n = nb + 4 * r;
#pragma unroll
    for (int s = 0; s < SM; ++s) {
      const int m = m0 + 16 * s + fr;
      f4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int64_t S = off[j];
#pragma unroll
        for (int c = 0; c <= D; ++c) S += (int64_t)acc[c][r][s][j] * ((int64_t)1 << (8 * c));
        o[j] = (float)(alpha * (double)S + bcol[j]);
      }
      if (m >= M || n >= N) continue;
      float* yr = Y + (int64_t)m * ldy + n;
      if (n + 4 <= N) {
        *reinterpret_cast<f4*>(yr) = o;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (n + j < N) yr[j] = o[j];
      }
    }
  }
}

// sums[n] = sum_k k_w[n][k] of a packed image, as the GEMM reads it (QVIT_W4: of the bytes 16 w). Four threads per
// weight row, each summing a quarter of the row's bytes of every stage and digit image (the swizzle permutes the
// quarters of a row only), folded with two shuffles: integers, so any order gives the same bits.
template <int WFMT>
__global__ __launch_bounds__(256) void weight_code_sums_kernel(const int8_t* __restrict__ Wp, int npad, int K,
                                                               int64_t* __restrict__ sums) {
  using G = A16Geo<WFMT>;
  constexpr int QB = G::WROW / 4;   // bytes per thread, stage and image: 16 (W8) / 8 (W4)
  const int n = (int)blockIdx.x * 64 + ((int)threadIdx.x >> 2), c = (int)threadIdx.x & 3;
  // weight row n sits in packed row rho: bits [3:2] and [5:4] swapped (an involution)
  const int rho = (n & ~63) | (((n >> 2) & 3) << 4) | (((n >> 4) & 3) << 2) | (n & 3);
  const int nk = K / A16_BK;
  const int64_t wpart = (int64_t)npad * K * G::WROW / 64;
  const int8_t* row = Wp + (int64_t)(rho >> 8) * nk * G::WBYTES + (rho & 255) * G::WROW + c * QB;
  int64_t total = 0;
  for (int q = 0; q < G::D; ++q) {
    int64_t sq = 0;
    for (int st = 0; st < nk; ++st) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(row + q * wpart + (int64_t)st * G::WBYTES);
      int part = 0;
#pragma unroll
      for (int i = 0; i < QB / 4; ++i) {
        const uint32_t w = p[i];
        if (WFMT == QVIT_W4) {
          const uint32_t lo = a16_nib_lo(w), hi = a16_nib_hi(w);
#pragma unroll
          for (int b = 0; b < 4; ++b) part += (int)(int8_t)(lo >> (8 * b)) + (int)(int8_t)(hi >> (8 * b));
        } else {
#pragma unroll
          for (int b = 0; b < 4; ++b) part += (int)(int8_t)(w >> (8 * b));
        }
      }
      sq += part;
    }
    total = total * 256 + sq;   // most significant digit first
  }
  total += __shfl_xor(total, 1, 64);
  total += __shfl_xor(total, 2, 64);
  if (c == 0) sums[n] = total;
}

// ---- activation quantizer: one thread = 16 columns of one row -> one 16-byte store per digit plane ----------------
__global__ __launch_bounds__(kThreads) void rows_to_digits_kernel(const float* __restrict__ x, int64_t rows,
                                                                  int64_t cols, int64_t ldx, int qtype, const float* d,
                                                                  const float* qm, const float* t, int levels,
                                                                  int8_t* __restrict__ planes, int64_t ldc,
                                                                  int64_t kpad) {
  const QParams p = load_qparams(qtype, d, qm, t, levels);
  const int64_t chunks_per_row = kpad / 16;
  const int64_t total = rows * chunks_per_row;
  const bool vec = ((ldx & 3) == 0) && ((((uintptr_t)x) & 15) == 0);
  for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = id / chunks_per_row;
    const int64_t c0 = (id - r * chunks_per_row) * 16;
    const float* src = x + r * ldx + c0;
    float v[16];
    if (vec && c0 + 16 <= cols) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 f = *reinterpret_cast<const float4*>(src + 4 * i);
        v[4 * i + 0] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = (c0 + i < cols) ? src[i] : 0.f;
    }
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hi[i] = lo[i] = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int k = (int)fminf(fmaxf(quant_code(v[4 * i + b], p), -32768.f), 32767.f);
        hi[i] |= ((uint32_t)(k >> 8) & 0xffu) << (8 * b);
        lo[i] |= ((uint32_t)((k & 255) - 128) & 0xffu) << (8 * b);
      }
    }
    *reinterpret_cast<uint4*>(planes + r * ldc + c0) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    *reinterpret_cast<uint4*>(planes + (rows + r) * ldc + c0) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
}

int64_t a16_tiles(int64_t M, int wfmt, int64_t npad) {
  const int64_t bm = wfmt == QVIT_W24 ? A16Geo<QVIT_W24>::BM : A16Geo<QVIT_W8>::BM;
  return (npad / A16_BN) * ((M + bm - 1) / bm);
}

bool a16_wfmt_ok(int wfmt) { return wfmt == QVIT_W4 || wfmt == QVIT_W8 || wfmt == QVIT_W16 || wfmt == QVIT_W24; }

// the shapes the GEMM takes (rows and columns in int32, tiles in a 2^30 grid, K within the accumulators' range)
bool a16_sizes_ok(int64_t M, int64_t K, int wfmt, int64_t N, int64_t npad) {
  if (!a16_wfmt_ok(wfmt)) return false;
  if (M < 0 || M > (1 << 24) || K <= 0 || K % QVIT_TILE_K || K > A16_MAX_K) return false;
  if (N <= 0 || npad < N || npad % A16_BN || npad > (1 << 24)) return false;
  return a16_tiles(M, wfmt, npad) <= (1 << 30);
}

}  // namespace

extern "C" int qvit_quantize_act_i16(const float* x, int64_t rows, int64_t cols, int64_t ldx, int qtype,
                                     const float* d_quant, const float* q_m, const float* t_quant, int levels,
                                     int8_t* planes, int64_t ldc, int64_t kpad, hipStream_t stream) {
  if (!x || !planes) return QVIT_ENULL;
  if (qvit_quant_status(qtype, d_quant, q_m, levels)) return QVIT_EINVAL;
  if (rows < 0 || cols < 0 || ldx < cols || kpad < cols || kpad % 16 || ldc < kpad) return QVIT_EINVAL;
  if ((ldc % 16) || qvit_misaligned(15, planes)) return QVIT_EALIGN;
  if (rows == 0 || kpad == 0) return QVIT_OK;
  const int64_t work = rows * (kpad / 16);
  hipLaunchKernelGGL(rows_to_digits_kernel, dim3(grid_for(work, kThreads)), dim3(kThreads), 0, stream, x, rows, cols,
                     ldx, qtype, d_quant, q_m, t_quant, levels, planes, ldc, kpad);
  return qvit_launch_status();
}

extern "C" int qvit_weight_code_sums(const void* Wp, int wfmt, int64_t npad, int64_t K, int64_t* sums,
                                     hipStream_t stream) {
  if (!Wp || !sums) return QVIT_ENULL;
  if (!a16_sizes_ok(0, K, wfmt, 1, npad)) return QVIT_EINVAL;
  if (qvit_misaligned(15, Wp) || qvit_misaligned(7, sums)) return QVIT_EALIGN;
  const int8_t* w = reinterpret_cast<const int8_t*>(Wp);
#define QVIT_A16_SUMS(F)                                                                                   \
  hipLaunchKernelGGL(weight_code_sums_kernel<F>, dim3((unsigned)(npad / 64)), dim3(256), 0, stream, w, (int)npad, \
                     (int)K, sums)
  if (wfmt == QVIT_W4) QVIT_A16_SUMS(QVIT_W4);
  else if (wfmt == QVIT_W8) QVIT_A16_SUMS(QVIT_W8);
  else if (wfmt == QVIT_W16) QVIT_A16_SUMS(QVIT_W16);
  else QVIT_A16_SUMS(QVIT_W24);
#undef QVIT_A16_SUMS
  return qvit_launch_status();
}

extern "C" int qvit_gemm_a16_fits(int64_t M, int64_t K, int wfmt, int64_t N, int64_t npad) {
  return a16_sizes_ok(M, K, wfmt, N, npad) ? 1 : 0;
}

extern "C" int qvit_gemm_a16(const int8_t* A, int64_t M, int64_t K, int64_t lda, const void* Wp, int wfmt, int64_t N,
                             int64_t npad, const float* d_act, const float* d_wt, const float* bias,
                             const int64_t* wsum, float* Y, int64_t ldy, hipStream_t stream) {
  if (!A || !Wp || !Y || !d_act || !d_wt || !wsum) return QVIT_ENULL;
  if (!a16_sizes_ok(M, K, wfmt, N, npad) || lda < K || ldy < N) return QVIT_EINVAL;
  if ((lda % 16) || (ldy % 4) || qvit_misaligned(15, A, Wp, Y, bias) || qvit_misaligned(7, wsum)) return QVIT_EALIGN;
  if (M == 0) return QVIT_OK;
  const int64_t ntiles = a16_tiles(M, wfmt, npad);
  const unsigned grid = (unsigned)((ntiles + 7) / 8 * 8);
  const int8_t* w = reinterpret_cast<const int8_t*>(Wp);
#define QVIT_A16_LAUNCH(F)                                                                                        \
  hipLaunchKernelGGL(gemm_a16_kernel<F>, dim3(grid), dim3(256), 0, stream, A, (int)M, (int)K, lda, w, (int)N,     \
                     (int)npad, d_act, d_wt, bias, wsum, Y, ldy)
  if (wfmt == QVIT_W4) QVIT_A16_LAUNCH(QVIT_W4);
  else if (wfmt == QVIT_W8) QVIT_A16_LAUNCH(QVIT_W8);
  else if (wfmt == QVIT_W16) QVIT_A16_LAUNCH(QVIT_W16);
  else QVIT_A16_LAUNCH(QVIT_W24);
#undef QVIT_A16_LAUNCH
  return qvit_launch_status();
}
