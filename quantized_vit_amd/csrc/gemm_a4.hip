// int4 x int4 / int4 x int8 contraction on packed 4-bit activation codes (QVIT_ACT_P4), and the quantizer that writes
// them: QuantizeLinear.forward (quant_layers.py:495-499) in WEIGHT_AND_ACTIVATION mode with at most 7 activation
// levels (the reference's headline num_bits = 4 on both operands). Same operands, same exact int32 accumulation on
// v_mfma_i32_16x16x64_i8 and the same epilogue arithmetic as qvit_gemm: C is qvit_gemm's on the unpacked codes, byte
// for byte. gfx950 has no int4 MFMA, so both operands are unpacked in registers to the signed bytes 16 x (a nibble
// moved to the high half of its byte): the accumulators hold 256 acc (QVIT_W4R) or 16 acc (QVIT_W8) exactly, and the
// factor is folded into alpha (a power of two) or shifted away (QVIT_EPI_I32).
//   |16 w 16 a| <= 128 * 112, so K <= 65536 keeps |sum| <= 9.4e8 < 2^31 for both weight formats.
//
// QVIT_ACT_P4 (include/qvit_hip.h): per row and 128-column k-tile one 64-byte group; byte j holds column j in its low
// and column 64 + j in its high nibble. A lane's 16-byte fragment read at byte 16 fq of the group is its MFMA operand
// for BOTH 64-deep k-steps of the tile: (p << 4) & 0xF0F0F0F0 is step 0, p & 0xF0F0F0F0 step 1.
//
// Geometry: one workgroup (4 waves, 2 per CU) per 256 (weight rows) x 128 (activation rows) tile; wave w owns weight
// rows [64 w, 64 w + 64) and all 128 activation rows: acc[8][4], 128 accumulator registers. K advances in 128-deep
// k-tiles: 64 MFMAs per wave between two barriers (qvit_gemm: 32).
// Operands:
//   activations  HBM / L2 -> LDS with global_load_lds_dwordx4, a ring of 3 slots of 8 KiB (128 rows x 64 B): two 1-KiB
//                pieces per wave and k-tile, half of qvit_gemm's DMA instructions and bytes per MFMA. Swizzled through
//                the per-lane source address (16-B chunk c of row r at c ^ (((r >> 2) & 1) << 1)), so the ds_read_b128
//                fragment reads are conflict-free. One fragment read and 12 VALU operations feed 8 MFMAs.
//   weights      straight into registers from the image (QVIT_W4R: 4 loads of 16 B per lane and k-tile, unpacked
//                once per k-tile for all 8 row groups; QVIT_W8: 8 loads, the image's chunk swizzle undone through
//                the address), two register sets, the next k-tile's loads issued behind the barrier.
// Every global load of the main loop is issued from asm, so the compiler's wait-count model sees none of them and
// never drains the ring; the queue is in order, and one counted wait per k-tile covers both operands. Order of issue:
//   act(0) w(0) act(1) | step kt: wait, barrier, w(kt + 1), act(kt + 2), MFMAs of kt
// At step kt's wait only act(kt + 1) is younger than w(kt): vmcnt(2) (0 when no k-tile follows). The wait also drains
// lgkmcnt, so every wave's fragment reads of k-tile kt - 1 have retired before the barrier behind which act(kt + 2)
// overwrites that slot. The barrier asm takes the weight registers as operands: their first use cannot move above it.
// Epilogue: a lane's 16 accumulators of a row group are 16 consecutive columns of one row (qvit_pack_weight's row
// permutation), so nothing is staged: gemm_skinny.hip's epilogue, once per 16-row group.
// Rows past M are clamped to row M - 1 on the load and never stored. No atomics, a fixed order: same call, same bits.
#include <cstddef>
#include <type_traits>

#include "gemm_epi16.h"
#include "qvit_common.h"
#include "reduce_common.h"

namespace {

constexpr int A4_BN = 256;              // weight rows per tile (one packed tile_n)
constexpr int A4_BM = 128;              // activation rows per tile
constexpr int A4_SM = A4_BM / 16;       // 16-row groups per tile
constexpr int A4_GROUP = 64;            // packed bytes per row and k-tile
constexpr int A4_SLOT = A4_BM * A4_GROUP;
constexpr int A4_RING = 3;
constexpr int A4_XP = A4_SLOT / 1024 / 4;   // 1-KiB DMA pieces per wave and k-tile
constexpr int A4_MAX_K = 65536;

QVIT_DEV uint32_t nib16_lo(uint32_t p) { return (p << 4) & 0xF0F0F0F0u; }
QVIT_DEV uint32_t nib16_hi(uint32_t p) { return p & 0xF0F0F0F0u; }
QVIT_DEV v4i nib16_lo4(v4i p) {
  return v4i{(int)nib16_lo(p[0]), (int)nib16_lo(p[1]), (int)nib16_lo(p[2]), (int)nib16_lo(p[3])};
}
QVIT_DEV v4i nib16_hi4(v4i p) {
  return v4i{(int)nib16_hi(p[0]), (int)nib16_hi(p[1]), (int)nib16_hi(p[2]), (int)nib16_hi(p[3])};
}

// a wave's weight registers of one 128-deep k-tile, as loaded: QVIT_W4R w[2 s + i] = the 32-B slice of step s (four
// 8-B fragments), QVIT_W8 w[4 s + r] = the int8 operand of step s and rows 16 r .. + 15
template <int WFMT>
struct A4Weights {
  static constexpr int NW = WFMT == QVIT_W4R ? 4 : 8;
  v4i w[NW];
};

// one 16-B register load from a wave-uniform base + per-lane offset, invisible to the compiler's wait counts
template <int OFF>
QVIT_DEV void ldw16(v4i& a, const void* sbase, uint32_t voff) {
  asm volatile("; qvit_asm_load\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3"
               : "=&v"(a)
               : "v"(voff), "s"(sbase), "n"(OFF)
               : "memory");
}

// This wave's LDS reads retired and at most the next k-tile's activation pieces (none when `more` is false) in
// flight; then the barrier, ONE statement on every path, to which the weight registers that the wait made valid are
// tied: a register copy the compiler needs for them lands at that statement, behind the wait, never in front of it
// (two barrier statements on the two arms made it copy the registers in front of one arm's wait).
QVIT_DEV void a4_wait(bool more) {
  __builtin_amdgcn_s_waitcnt(0xC07F);
  if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A4_XP) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
QVIT_DEV void a4_barrier(v4i (&w)[4]) {
  asm volatile("s_barrier" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3])::"memory");
}
QVIT_DEV void a4_barrier(v4i (&w)[8]) {
  asm volatile("s_barrier"
               : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7])::"memory");
}

template <int WFMT, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_a4_kernel(const uint8_t* __restrict__ A, int M, int K, int64_t ldp,
                                                         const int8_t* __restrict__ Wp, int N, int npad,
                                                         void* __restrict__ C, int64_t ldc, Epi16Args ep) {
  constexpr bool W4 = WFMT == QVIT_W4R;
  constexpr bool I8OUT = (EPI == QVIT_EPI_I8 || EPI == QVIT_EPI_I8_GELU);
  constexpr int CHUNK = W4 ? 8192 : 16384;   // one (256-row tile, 64-deep stage) of the weight image
  constexpr int SHIFT = W4 ? 8 : 4;
  __shared__ __attribute__((aligned(16))) uint8_t smem[A4_RING * A4_SLOT];
  __shared__ QParams qp_l;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;

  // tile: XCD x (blocks x, x + 8, ...) walks a contiguous range, weight tiles fastest (one activation panel per L2)
  const int nb_n = npad / A4_BN;
  const int ntiles = nb_n * ((M + A4_BM - 1) / A4_BM);
  const int per = (ntiles + 7) >> 3;
  const int t = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (t >= ntiles) return;
  const int m0 = (t / nb_n) * A4_BM, tn = t % nb_n, n0 = tn * A4_BN;
  const int nkt = K / 128;

  Epi16Quant q{false, 0.f, 0.f, 0.f, {}};
  if constexpr (I8OUT) {
    if (ep.table != nullptr) {
      const EpiTableHdr h = *reinterpret_cast<const EpiTableHdr*>(ep.table);
      q.use_table = h.valid != 0 && h.nb >= 1 && h.nb <= QVIT_EPI_TABLE_MAX_NB;
      q.c0 = h.c0;
      q.inv_w = h.inv_w;
      q.top = epi_top(h.nb);
    }
    if (!q.use_table && tid == 0) qp_l = load_qparams(ep.out_qtype, ep.out_d, ep.out_qm, ep.out_t, ep.out_levels);
  }

  // ---- activation DMA: piece pi = A4_XP wave + j of a slot is rows 16 pi .. + 15; lane l stages row l >> 2, LDS chunk
  // position l & 3 = source chunk (l & 3) ^ (row bit 2 << 1) (row bit 2 = lane bit 4)
  const uint8_t* asrc[A4_XP];
#pragma unroll
  for (int j = 0; j < A4_XP; ++j) {
    const int row = min(m0 + 16 * (A4_XP * wave + j) + (lane >> 2), M - 1);   // the tail: a valid row, never stored
    asrc[j] = A + (int64_t)row * ldp + (((lane & 3) ^ (((lane >> 4) & 1) << 1)) << 4);
  }
  const uint32_t lds0 = lds_addr(smem);
  auto issue_act = [&](int kt, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < A4_XP; ++j)
      dma16(asrc[j] + kt * A4_GROUP,
            __builtin_amdgcn_readfirstlane(lds0 + slot * A4_SLOT + (A4_XP * wave + j) * 1024));
  };
  // fragment read: row 16 s + fr, source chunk fq
  const int xoff = fr * A4_GROUP + ((fq ^ (((fr >> 2) & 1) << 1)) << 4);

  // ---- weight registers: this tile_n's image, stage-major; per lane the wave's slice of a stage
  const int8_t* const wbase = Wp + (int64_t)tn * (K / 64) * CHUNK;
  const uint32_t woff = W4 ? 2048 * wave + 32 * lane : (64 * wave + fr) * 64 + ((fq ^ (((fr >> 2) & 1) << 1)) << 4);
  auto load_w = [&](A4Weights<WFMT>& f, int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint32_t vo = woff + (uint32_t)(2 * kt + s) * CHUNK;
      if constexpr (W4) {
        ldw16<0>(f.w[2 * s], wbase, vo);
        ldw16<16>(f.w[2 * s + 1], wbase, vo);
      } else {
        ldw16<0>(f.w[4 * s], wbase, vo);
        ldw16<1024>(f.w[4 * s + 1], wbase, vo);
        ldw16<2048>(f.w[4 * s + 2], wbase, vo);
        ldw16<3072>(f.w[4 * s + 3], wbase, vo);
      }
    }
  };

  // acc[s][r][j] = 2^SHIFT sum_k A[m0 + 16 s + fr][k] W[n0 + 64 w + 16 fq + 4 r + j][k]
  v4i acc[A4_SM][4];
#pragma unroll
  for (int s = 0; s < A4_SM; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[s][r] = v4i{0, 0, 0, 0};

  A4Weights<WFMT> wr[2];
  auto step = [&](auto bsel, int kt) __attribute__((always_inline)) {
    constexpr int B = decltype(bsel)::value;
    a4_wait(kt + 1 < nkt);
    a4_barrier(wr[B].w);
    if (kt + 1 < nkt) load_w(wr[B ^ 1], kt + 1);
    if (kt + 2 < nkt) issue_act(kt + 2, (kt + 2) % A4_RING);
    v4i wf[2][4];   // the MFMA operands of both k-steps
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if constexpr (W4) {
          const v4i p = wr[B].w[2 * s + (r >> 1)];
          const uint32_t px = (uint32_t)p[2 * (r & 1)], py = (uint32_t)p[2 * (r & 1) + 1];
          wf[s][r] = v4i{(int)nib16_lo(px), (int)nib16_hi(px), (int)nib16_lo(py), (int)nib16_hi(py)};
        } else {
          wf[s][r] = wr[B].w[4 * s + r];
        }
      }
    const uint8_t* sx = smem + (kt % A4_RING) * A4_SLOT + xoff;
#pragma unroll
    for (int s = 0; s < A4_SM; ++s) {
      const v4i p = *reinterpret_cast<const v4i*>(sx + s * 16 * A4_GROUP);
      const v4i x0 = nib16_lo4(p), x1 = nib16_hi4(p);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[s][r] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[0][r], x0, acc[s][r], 0, 0, 0);
        acc[s][r] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[1][r], x1, acc[s][r], 0, 0, 0);
      }
    }
  };

  issue_act(0, 0);
  load_w(wr[0], 0);
  if (nkt > 1) issue_act(1, 1);
  int kt = 0;
#pragma unroll 1
  for (; kt + 1 < nkt; kt += 2) {
    step(std::integral_constant<int, 0>{}, kt);
    step(std::integral_constant<int, 1>{}, kt + 1);
  }
  if (kt < nkt) step(std::integral_constant<int, 0>{}, kt);

  if constexpr (I8OUT) {
    __syncthreads();   // qp_l
    if (!q.use_table) q.qp = qp_l;
  }
  float alpha = 0.f;
  if constexpr (EPI != QVIT_EPI_I32) alpha = (*ep.d_act) * (*ep.d_wt) * (W4 ? 0.00390625f : 0.0625f);
  const int nb = n0 + 64 * wave + 16 * fq;
  if (nb >= N) return;
#pragma unroll
  for (int s = 0; s < A4_SM; ++s) {
    const int m = m0 + 16 * s + fr;
    if (m < M) epi16_row<EPI, SHIFT>(acc[s], m, nb, N, C, ldc, alpha, ep, q);
  }
}

// ---- activation quantizer: one thread = one byte group of 16: columns c .. c + 15 (low nibbles) and 64 + c .. (high
// nibbles) of a k-tile, two runs of 16-byte loads -> one 16-byte store
__global__ __launch_bounds__(kThreads) void rows_to_nibbles_kernel(const float* __restrict__ x, int64_t rows,
                                                                   int64_t cols, int64_t ldx, int qtype,
                                                                   const float* d, const float* qm, const float* t,
                                                                   int levels, uint8_t* __restrict__ packed,
                                                                   int64_t ldp, int64_t kpad) {
  const QParams p = load_qparams(qtype, d, qm, t, levels);
  const int64_t groups_per_row = kpad / 32;   // 4 per k-tile
  const int64_t total = rows * groups_per_row;
  const bool vec = ((ldx & 3) == 0) && ((((uintptr_t)x) & 15) == 0);
  for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = id / groups_per_row;
    const int64_t g = id - r * groups_per_row;
    const int64_t c0 = (g >> 2) * 128 + (g & 3) * 16;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int64_t c = c0 + 64 * half;
      const float* src = x + r * ldx + c;
      float v[16];
      if (vec && c + 16 <= cols) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4 f = *reinterpret_cast<const float4*>(src + 4 * i);
          v[4 * i + 0] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = (c + i < cols) ? src[i] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = (int)fminf(fmaxf(quant_code(v[i], p), -7.f), 7.f);
        w[i >> 2] |= ((uint32_t)k & 0xfu) << (8 * (i & 3) + 4 * half);
      }
    }
    *reinterpret_cast<uint4*>(packed + r * ldp + (g >> 2) * A4_GROUP + (g & 3) * 16) =
        make_uint4(w[0], w[1], w[2], w[3]);
  }
}

int64_t a4_tiles(int64_t M, int64_t npad) { return (npad / A4_BN) * ((M + A4_BM - 1) / A4_BM); }

// the shapes the GEMM takes: the two images gemm_skinny.hip reads, K within the accumulators' range, rows and
// columns in int32, tiles in a 2^30 grid
bool a4_sizes_ok(int64_t M, int64_t K, int wfmt, int64_t N, int64_t npad) {
  if (wfmt != QVIT_W4R && wfmt != QVIT_W8) return false;
  if (M < 0 || M > INT32_MAX / 2 || K <= 0 || K % QVIT_TILE_K || K > A4_MAX_K) return false;
  if (N <= 0 || npad < N || npad % QVIT_TILE_N || npad > INT32_MAX / 2) return false;
  return a4_tiles(M, npad) <= (1 << 30);
}

template <int WFMT, int EPI>
int launch(const uint8_t* A, int64_t M, int64_t K, int64_t ldp, const void* Wp, int64_t N, int64_t npad, void* C,
           int64_t ldc, const Epi16Args& ep, hipStream_t stream) {
  const unsigned grid = (unsigned)((a4_tiles(M, npad) + 7) / 8 * 8);
  hipLaunchKernelGGL((gemm_a4_kernel<WFMT, EPI>), dim3(grid), dim3(256), 0, stream, A, (int)M, (int)K, ldp,
                     reinterpret_cast<const int8_t*>(Wp), (int)N, (int)npad, C, ldc, ep);
  return qvit_launch_status();
}

template <int WFMT>
int dispatch_epi(int epilogue, const uint8_t* A, int64_t M, int64_t K, int64_t ldp, const void* Wp, int64_t N,
                 int64_t npad, void* C, int64_t ldc, const Epi16Args& ep, hipStream_t stream) {
  switch (epilogue) {
    case QVIT_EPI_F32: return launch<WFMT, QVIT_EPI_F32>(A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
    case QVIT_EPI_F32_RESID: return launch<WFMT, QVIT_EPI_F32_RESID>(A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
    case QVIT_EPI_I8_GELU: return launch<WFMT, QVIT_EPI_I8_GELU>(A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
    case QVIT_EPI_I8: return launch<WFMT, QVIT_EPI_I8>(A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
    case QVIT_EPI_I32: return launch<WFMT, QVIT_EPI_I32>(A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
    default: return QVIT_EINVAL;
  }
}

}  // namespace

extern "C" int qvit_quantize_act_i4(const float* x, int64_t rows, int64_t cols, int64_t ldx, int qtype,
                                    const float* d_quant, const float* q_m, const float* t_quant, int levels,
                                    uint8_t* packed, int64_t ldp, int64_t kpad, hipStream_t stream) {
  if (!x || !packed) return QVIT_ENULL;
  if (qvit_quant_status(qtype, d_quant, q_m, levels)) return QVIT_EINVAL;
  if (rows < 0 || cols < 0 || ldx < cols || kpad < cols || kpad % QVIT_TILE_K || ldp < kpad / 2) return QVIT_EINVAL;
  if ((ldp % 16) || qvit_misaligned(15, packed)) return QVIT_EALIGN;
  if (rows == 0 || kpad == 0) return QVIT_OK;
  const int64_t work = rows * (kpad / 32);
  hipLaunchKernelGGL(rows_to_nibbles_kernel, dim3(grid_for(work, kThreads)), dim3(kThreads), 0, stream, x, rows, cols,
                     ldx, qtype, d_quant, q_m, t_quant, levels, packed, ldp, kpad);
  return qvit_launch_status();
}

extern "C" int qvit_gemm_a4_fits(int64_t M, int64_t K, int wfmt, int64_t N, int64_t npad, int epilogue) {
  return a4_sizes_ok(M, K, wfmt, N, npad) && epilogue >= QVIT_EPI_F32 && epilogue <= QVIT_EPI_I32 ? 1 : 0;
}

extern "C" int qvit_gemm_a4(const uint8_t* A, int64_t M, int64_t K, int64_t ldp, const void* Wp, int wfmt, int64_t N,
                            int64_t npad, const float* d_act, const float* d_wt, const float* bias, int epilogue,
                            void* C, int64_t ldc, int out_qtype, const float* out_d, const float* out_qm,
                            const float* out_t, int out_levels, const void* epi_table, hipStream_t stream) {
  // qvit_gemm's checks, in its order, on this kernel's shapes
  if (!A || !Wp || !C) return QVIT_ENULL;
  if (!a4_sizes_ok(M, K, wfmt, N, npad) || ldp < K / 2) return QVIT_EINVAL;
  if ((ldp % 16) || qvit_misaligned(15, A, Wp)) return QVIT_EALIGN;
  if (epilogue < QVIT_EPI_F32 || epilogue > QVIT_EPI_I32) return QVIT_EINVAL;
  const bool i8out = epilogue == QVIT_EPI_I8 || epilogue == QVIT_EPI_I8_GELU;
  if (ldc < N) return QVIT_EINVAL;
  if (i8out) {
    if ((ldc % 4) || qvit_misaligned(3, C)) return QVIT_EALIGN;
    if (qvit_out_quant_status(out_qtype, out_d, out_qm, out_levels)) return QVIT_EINVAL;
  } else {
    if ((ldc % 4) || qvit_misaligned(15, C)) return QVIT_EALIGN;
  }
  if (epilogue != QVIT_EPI_I32 && (!d_act || !d_wt)) return QVIT_ENULL;
  if (qvit_misaligned(15, bias, epi_table)) return QVIT_EALIGN;
  if (M == 0) return QVIT_OK;
  const Epi16Args ep{d_act, d_wt, bias, out_qtype, out_d, out_qm, out_t, out_levels,
                  i8out ? reinterpret_cast<const int8_t*>(epi_table) : nullptr};
  if (wfmt == QVIT_W4R) return dispatch_epi<QVIT_W4R>(epilogue, A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
  return dispatch_epi<QVIT_W8>(epilogue, A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
}
