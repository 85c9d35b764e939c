// W4A4 contraction on the FP6 matrix instruction: QuantizeLinear.forward (quant_layers.py:495-499) in
// WEIGHT_AND_ACTIVATION mode with at most 7 levels on both operands (the reference's headline num_bits = 4), and the
// quantizer and weight packer that write its operands. Every integer in [-7, 7] is an FP6 E2M3 value (3 mantissa bits,
// bias 1, maximum 7.5), so v_mfma_f32_16x16x128_f8f6f4 with both operands E2M3 (cbsz 2, blgp 2, scale 1.0) multiplies
// the codes themselves, 128 K-columns in the 4 passes in which v_mfma_i32_16x16x64_i8 does 64, with no unpacking
// between the operand read and the MFMA. A product is an integer of magnitude <= 49, and with K <= 65536 every partial
// sum of a row has magnitude <= 3 211 264 < 2^24: the fp32 accumulator adds exact integers and holds qvit_gemm's
// int32 accumulator. It is converted to int32 (exact) before the epilogue, which is gemm_a4.hip's (gemm_epi16.h): C is
// qvit_gemm's on the same codes, byte for byte.
//
// Element: bit 5 the sign, magnitudes 0..7 = 0x00 0x08 0x10 0x14 0x18 0x1A 0x1C 0x1E, zero always +0. A lane's MFMA
// operand is 32 consecutive K-columns as 24 bytes, column j of the 32 at bits [6 j, 6 j + 6) (dense, little-endian):
// a 16-byte head and an 8-byte tail. Both operands use the same order, so products pair up column by column.
//
// QVIT_ACT_F6 (include/qvit_hip.h): per row and 128-column k-tile 96 bytes: the four 16-byte heads of the column
// groups 32 q .. 32 q + 31 (q = 0..3), then the four 8-byte tails.
// QVIT_W6F: per (256-row tile, k-tile) a chunk of 24 KiB; for the 16-row group g' = 0..15 of the tile (packed rows
// 16 g' .. 16 g' + 15 of qvit_pack_weight's order) 1536 bytes: lane l's head (row l & 15, column group l >> 4) at byte
// 16 l, its tail at byte 1024 + 8 l: every register load of a wave is one contiguous 1-KiB or 512-byte run.
//
// Geometry: one workgroup (4 waves, 2 per CU) per 256 (weight rows) x 128 (activation rows) tile, as gemm_a4.hip, but
// the wave tile is turned: wave w owns weight rows [128 (w & 1), + 128) and activation rows [64 (w >> 1), + 64), so a
// 24-byte activation fragment from LDS feeds 8 MFMAs (gemm_a4's tile at this instruction: 4) and the four waves ask
// the LDS for half the bytes per MFMA cycle. acc[4][8], 128 accumulator registers; 32 MFMAs per wave and k-tile.
// Operands:
//   activations  HBM / L2 -> LDS with global_load_lds_dwordx4, a ring of 3 slots of 12 KiB: heads [128 rows][64 B],
//                then tails [128 rows][32 B]; three 1-KiB pieces per wave and k-tile (two of heads, 16 rows each, one
//                of tails, 32 rows). Swizzled through the per-lane source address: head q of row r at chunk
//                q ^ (((r >> 2) & 1) << 1) (gemm_a4's), the tails' 16-byte halves swapped in rows with bit 3 set, so
//                the ds_read_b128 and the ds_read_b64 of a fragment are aligned and conflict-free.
//   weights      straight into registers from the image: 8 loads of 16 B and 8 of 8 B per lane and k-tile into ONE
//                register set (two sets and 128 accumulators do not fit 256 registers): group g's registers are
//                reloaded with the next k-tile right behind its four MFMAs, a whole k-tile of MFMAs ahead of their
//                next use. The two waves that share a weight half load the same lines.
// Every global load of the main loop is issued from asm (see gemm_a4.hip), the queue is in order, and the waits are
// counted: before group g's MFMAs at most 14 + 3 younger loads may be in flight (see the step). One barrier per
// k-tile, one asm statement on every path, behind a wait that drains lgkmcnt.
//   act(0) act(1) w(0) | step kt: barrier, act(kt + 2), fragments, per group g: wait, 4 MFMAs, w(kt + 1)[g]
// Rows past M are clamped to row M - 1 on the load and never stored. No atomics, a fixed order: same call, same bits.
#include <cstddef>
#include <type_traits>

#include "gemm_epi16.h"
#include "qvit_common.h"
#include "reduce_common.h"

namespace {

typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int F6_BN = 256;               // weight rows per tile (one packed tile_n)
constexpr int F6_BM = 128;               // activation rows per tile
constexpr int F6_GROUP = 96;             // bytes per row and k-tile
constexpr int F6_HEADS = F6_BM * 64;     // a slot's heads, then its tails
constexpr int F6_SLOT = F6_BM * F6_GROUP;
constexpr int F6_RING = 3;
constexpr int F6_XP = F6_SLOT / 1024 / 4;    // 1-KiB DMA pieces per wave and k-tile
constexpr int F6_CHUNK = F6_BN * F6_GROUP;   // one (256-row tile, k-tile) of the weight image
constexpr int F6_WGROUP = 1536;              // one 16-row group of a chunk: 64 heads, 64 tails
constexpr int F6_MAX_K = 65536;

// the E2M3 field of a code in [-7, 7]
QVIT_DEV uint32_t e2m3(int k) {
  const uint32_t m = (uint32_t)(k < 0 ? -k : k);
  return (uint32_t)((0x1E1C1A1814100800ull >> (8 * m)) & 0x3Fu) | (k < 0 ? 0x20u : 0u);
}

// 32 fields -> the 24 operand bytes, field j at bits [6 j, 6 j + 6)
QVIT_DEV void pack32(const uint32_t (&f)[32], uint4& head, uint2& tail) {
  uint64_t q[3] = {0ull, 0ull, 0ull};
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const int bit = 6 * j, w = bit >> 6, o = bit & 63;
    q[w] |= (uint64_t)f[j] << o;
    if (o > 58) q[w + 1] |= (uint64_t)f[j] >> (64 - o);
  }
  head = make_uint4((uint32_t)q[0], (uint32_t)(q[0] >> 32), (uint32_t)q[1], (uint32_t)(q[1] >> 32));
  tail = make_uint2((uint32_t)q[2], (uint32_t)(q[2] >> 32));
}

// a wave's weight registers of one k-tile: the operand of its 16-row group g is {h[g], t[g]}
struct F6Weights {
  v4i h[8];
  v2i t[8];
};

// register loads from a wave-uniform base + per-lane offset, invisible to the compiler's wait counts
template <int OFF>
QVIT_DEV void ldw16(v4i& a, const void* sbase, uint32_t voff) {
  asm volatile("; qvit_asm_load\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3"
               : "=&v"(a)
               : "v"(voff), "s"(sbase), "n"(OFF)
               : "memory");
}
template <int OFF>
QVIT_DEV void ldw8(v2i& a, const void* sbase, uint32_t voff) {
  asm volatile("; qvit_asm_load\n\tglobal_load_dwordx2 %0, %1, %2 offset:%3"
               : "=&v"(a)
               : "v"(voff), "s"(sbase), "n"(OFF)
               : "memory");
}

// Group g's operand of this k-tile has arrived when at most INFLIGHT younger loads are outstanding (the queue is in
// order); the registers are tied to the wait, so no copy of them can move in front of it (gemm_a4.hip's lesson).
template <int INFLIGHT>
QVIT_DEV void f6_wait_group(v4i& h, v2i& t) {
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(h), "+v"(t) : "n"(INFLIGHT) : "memory");
}

// a wave's activation fragments of one k-tile: row group s of its 64 rows
struct F6Frags {
  v4i h[4];
  v2i t[4];
};
template <int S>
QVIT_DEV void f6_read(F6Frags& x, uint32_t head_addr, uint32_t tail_addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(x.h[S]) : "v"(head_addr), "n"(S * 16 * 64) : "memory");
  asm volatile("ds_read_b64 %0, %1 offset:%2" : "=&v"(x.t[S]) : "v"(tail_addr), "n"(S * 16 * 32) : "memory");
}
QVIT_DEV void f6_wait_frags(F6Frags& x) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(x.h[0]), "+v"(x.h[1]), "+v"(x.h[2]), "+v"(x.h[3]), "+v"(x.t[0]), "+v"(x.t[1]), "+v"(x.t[2]),
                 "+v"(x.t[3])::"memory");
}

// the 6-register operand {head, tail}; the last two lanes of the builtin's type are not read at cbsz / blgp 2
QVIT_DEV v8i f6_operand(v4i h, v2i t) {
  const v8i hh = __builtin_shufflevector(h, h, 0, 1, 2, 3, -1, -1, -1, -1);
  const v8i tt = __builtin_shufflevector(t, t, 0, 1, -1, -1, -1, -1, -1, -1);
  return __builtin_shufflevector(hh, tt, 0, 1, 2, 3, 8, 9, -1, -1);
}

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_f6_kernel(const uint8_t* __restrict__ A, int M, int K, int64_t ldp,
                                                         const uint8_t* __restrict__ Wp, int N, int npad,
                                                         void* __restrict__ C, int64_t ldc, Epi16Args ep) {
  constexpr bool I8OUT = (EPI == QVIT_EPI_I8 || EPI == QVIT_EPI_I8_GELU);
  __shared__ __attribute__((aligned(16))) uint8_t smem[F6_RING * F6_SLOT];
  __shared__ QParams qp_l;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wh = wave & 1, ah = wave >> 1;
  const int fr = lane & 15, fq = lane >> 4;

  // tile: XCD x (blocks x, x + 8, ...) walks a contiguous range, weight tiles fastest (one activation panel per L2)
  const int nb_n = npad / F6_BN;
  const int ntiles = nb_n * ((M + F6_BM - 1) / F6_BM);
  const int per = (ntiles + 7) >> 3;
  const int t = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (t >= ntiles) return;
  const int m0 = (t / nb_n) * F6_BM, tn = t % nb_n, n0 = tn * F6_BN;
  const int nkt = K / 128;

  Epi16Quant q{false, 0.f, 0.f, 0.f, {}};
  if constexpr (I8OUT) {
    q = epi16_quant(ep.table);
    if (!q.use_table && tid == 0) qp_l = load_qparams(ep.out_qtype, ep.out_d, ep.out_qm, ep.out_t, ep.out_levels);
  }

  // ---- activation DMA. Pieces 2 wave, 2 wave + 1 of the heads: rows 16 pi .. + 15, lane l stages row l >> 2, LDS
  // chunk l & 3 = source head (l & 3) ^ (row bit 2 << 1). Piece `wave` of the tails: rows 32 wave .. + 31, lane l
  // stages row l >> 1, LDS half l & 1 = source half (l & 1) ^ row bit 3 (= lane bit 4).
  const uint8_t* asrc[F6_XP];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = min(m0 + 16 * (2 * wave + j) + (lane >> 2), M - 1);   // the tail: a valid row, never stored
    asrc[j] = A + (int64_t)row * ldp + (((lane & 3) ^ (((lane >> 4) & 1) << 1)) << 4);
  }
  {
    const int row = min(m0 + 32 * wave + (lane >> 1), M - 1);
    asrc[2] = A + (int64_t)row * ldp + 64 + (((lane & 1) ^ ((lane >> 4) & 1)) << 4);
  }
  const uint32_t lds0 = lds_addr(smem);
  auto issue_act = [&](int kt, int slot) __attribute__((always_inline)) {
    const uint32_t s0 = lds0 + slot * F6_SLOT;
    dma16(asrc[0] + kt * F6_GROUP, __builtin_amdgcn_readfirstlane(s0 + (2 * wave) * 1024));
    dma16(asrc[1] + kt * F6_GROUP, __builtin_amdgcn_readfirstlane(s0 + (2 * wave + 1) * 1024));
    dma16(asrc[2] + kt * F6_GROUP, __builtin_amdgcn_readfirstlane(s0 + F6_HEADS + wave * 1024));
  };
  // fragment reads of row 64 ah + 16 s + fr, column group fq
  const int xh = (64 * ah + fr) * 64 + ((fq ^ (((fr >> 2) & 1) << 1)) << 4);
  const int xt = F6_HEADS + (64 * ah + fr) * 32 + ((fq ^ (((fr >> 3) & 1) << 1)) << 3);

  // ---- weight registers: this tile_n's image, k-tile-major; per lane its fields of the wave's 8 row groups
  const uint8_t* const wbase = Wp + (int64_t)tn * nkt * F6_CHUNK;
  const uint32_t woffh = wh * 8 * F6_WGROUP + 16 * lane, wofft = wh * 8 * F6_WGROUP + 1024 + 8 * lane;
  auto load_w = [&](F6Weights& f, int kt, int g) __attribute__((always_inline)) {
    // (three groups per offset base: the instruction's offset field ends at 4095)
    const uint32_t vh = woffh + (uint32_t)kt * F6_CHUNK + (g / 3) * 3 * F6_WGROUP;
    const uint32_t vt = wofft + (uint32_t)kt * F6_CHUNK + (g / 3) * 3 * F6_WGROUP;
    if (g % 3 == 0) {
      ldw16<0>(f.h[g], wbase, vh);
      ldw8<0>(f.t[g], wbase, vt);
    } else if (g % 3 == 1) {
      ldw16<F6_WGROUP>(f.h[g], wbase, vh);
      ldw8<F6_WGROUP>(f.t[g], wbase, vt);
    } else {
      ldw16<2 * F6_WGROUP>(f.h[g], wbase, vh);
      ldw8<2 * F6_WGROUP>(f.t[g], wbase, vt);
    }
  };

  // acc[s][4 G + r][j] = sum_k A[m0 + 64 ah + 16 s + fr][k] W[n0 + 128 wh + 64 G + 16 fq + 4 r + j][k]
  v4f acc[4][8];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int g = 0; g < 8; ++g) acc[s][g] = v4f{0.f, 0.f, 0.f, 0.f};

  // One register set. Group g's registers are reloaded with k-tile kt + 1 right behind its four MFMAs of k-tile kt,
  // a whole k-tile of MFMAs ahead of their next use. In flight behind w(kt)[g] at its wait: w(kt)[g + 1 ..] (two loads
  // a group), act(kt + 2) (F6_XP pieces), w(kt + 1)[.. g - 1]: 14 + F6_XP with two k-tiles to follow (AHEAD 2), 14
  // with one (AHEAD 1), and the last k-tile (AHEAD 0) drains. act(kt) is older than w(kt - 1), which step kt - 1
  // waited for; step 0 drains the prologue. lgkmcnt(0) before the barrier: every wave's fragment reads of k-tile
  // kt - 1 have retired before act(kt + 2) overwrites that slot.
  F6Weights wr;
  auto step = [&](auto ahead, int kt) __attribute__((always_inline)) {
    constexpr int AHEAD = decltype(ahead)::value;
    constexpr int INFLIGHT = AHEAD == 2 ? 14 + F6_XP : AHEAD == 1 ? 14 : 0;
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (kt == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");
    if constexpr (AHEAD == 2) issue_act(kt + 2, (kt + 2) % F6_RING);
    // the four fragments, read from asm (left to itself the compiler pairs the 8-byte reads as ds_read2st64_b64 and
    // then moves the halves into the operand tuples); one wait, to which the registers are tied
    F6Frags x;
    const uint32_t xa = lds_addr(smem) + (kt % F6_RING) * F6_SLOT;
    f6_read<0>(x, xa + xh, xa + xt);
    f6_read<1>(x, xa + xh, xa + xt);
    f6_read<2>(x, xa + xh, xa + xt);
    f6_read<3>(x, xa + xh, xa + xt);
    f6_wait_frags(x);
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      f6_wait_group<INFLIGHT>(wr.h[g], wr.t[g]);
      const v8i w = f6_operand(wr.h[g], wr.t[g]);
#pragma unroll
      for (int s = 0; s < 4; ++s)
        acc[s][g] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, f6_operand(x.h[s], x.t[s]), acc[s][g], 2, 2, 0,
                                                                     0, 0, 0);
      if constexpr (AHEAD >= 1) load_w(wr, kt + 1, g);
    }
  };

  issue_act(0, 0);
  if (nkt > 1) issue_act(1, 1);
#pragma unroll
  for (int g = 0; g < 8; ++g) load_w(wr, 0, g);
  int kt = 0;
#pragma unroll 1
  for (; kt + 2 < nkt; ++kt) step(std::integral_constant<int, 2>{}, kt);
  if (kt + 1 < nkt) step(std::integral_constant<int, 1>{}, kt++);
  step(std::integral_constant<int, 0>{}, kt);

  if constexpr (I8OUT) {
    __syncthreads();   // qp_l
    if (!q.use_table) q.qp = qp_l;
  }
  float alpha = 0.f;
  if constexpr (EPI != QVIT_EPI_I32) alpha = (*ep.d_act) * (*ep.d_wt);
#pragma unroll
  for (int G = 0; G < 2; ++G) {
    const int nb = n0 + 128 * wh + 64 * G + 16 * fq;
    if (nb >= N) continue;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int m = m0 + 64 * ah + 16 * s + fr;
      if (m >= M) continue;
      v4i a[4];   // the int32 accumulator of qvit_gemm: every fp32 value is an integer below 2^24
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const v4f f = acc[s][4 * G + r];
        a[r] = v4i{(int)f[0], (int)f[1], (int)f[2], (int)f[3]};
      }
      epi16_row<EPI, 0>(a, m, nb, N, C, ldc, alpha, ep, q);
    }
  }
}

// ---- activation quantizer: one thread = one 32-column group: eight 16-byte loads -> its head and its tail
__global__ __launch_bounds__(kThreads) void rows_to_f6_kernel(const float* __restrict__ x, int64_t rows, int64_t cols,
                                                              int64_t ldx, int qtype, const float* d, const float* qm,
                                                              const float* t, int levels, uint8_t* __restrict__ out,
                                                              int64_t ldp, int64_t kpad) {
  const QParams p = load_qparams(qtype, d, qm, t, levels);
  const int64_t groups_per_row = kpad / 32;
  const int64_t total = rows * groups_per_row;
  const bool vec = ((ldx & 3) == 0) && ((((uintptr_t)x) & 15) == 0);
  for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < total;
       id += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = id / groups_per_row;
    const int64_t g = id - r * groups_per_row;
    const int64_t c = 32 * g;
    const float* src = x + r * ldx + c;
    uint32_t f[32];
    if (vec && c + 32 <= cols) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(src + 4 * i);
        f[4 * i + 0] = e2m3((int)fminf(fmaxf(quant_code(v.x, p), -7.f), 7.f));
        f[4 * i + 1] = e2m3((int)fminf(fmaxf(quant_code(v.y, p), -7.f), 7.f));
        f[4 * i + 2] = e2m3((int)fminf(fmaxf(quant_code(v.z, p), -7.f), 7.f));
        f[4 * i + 3] = e2m3((int)fminf(fmaxf(quant_code(v.w, p), -7.f), 7.f));
      }
    } else {
#pragma unroll
      for (int i = 0; i < 32; ++i)
        f[i] = e2m3((int)fminf(fmaxf(quant_code(c + i < cols ? src[i] : 0.f, p), -7.f), 7.f));
    }
    uint4 head;
    uint2 tail;
    pack32(f, head, tail);
    uint8_t* dst = out + r * ldp + (g >> 2) * F6_GROUP;
    *reinterpret_cast<uint4*>(dst + 16 * (g & 3)) = head;
    *reinterpret_cast<uint2*>(dst + 64 + 8 * (g & 3)) = tail;
  }
}

// ---- weight packer: one thread = one packed row's 32-column group of the QVIT_W4 image. There, per (256-row block,
// 64-deep stage), row r holds 32 bytes: its 16-column chunk c (two uint32; byte b of a word covering k0 .. k0 + 7 holds
// k0 + b in its low and k0 + 4 + b in its high nibble) at position c ^ (2 if r & 8 else 0): a column group is the
// 16-byte half (q & 1) ^ (r bit 3) of its stage's row.
__global__ __launch_bounds__(kThreads) void pack_w6f_kernel(const uint8_t* __restrict__ packed, int64_t npad,
                                                            int64_t kpad, uint8_t* __restrict__ out,
                                                            int32_t* __restrict__ bad) {
  const int64_t groups_per_row = kpad / 32;
  const int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (id >= npad * groups_per_row) return;
  const int64_t row = id / groups_per_row;
  const int64_t g = id - row * groups_per_row;
  const int64_t tn = row / F6_BN, kt = g >> 2;
  const int rr = (int)(row % F6_BN);
  const uint4 u = *reinterpret_cast<const uint4*>(packed + ((tn * (kpad / 64) + (g >> 1)) * F6_BN + rr) * 32 +
                                                  (((int)(g & 1) ^ ((rr >> 3) & 1)) << 4));
  const uint32_t wds[4] = {u.x, u.y, u.z, u.w};
  uint32_t f[32];
  int nbad = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = ((int)(wds[w] << (28 - (8 * (i & 3) + 4 * (i >> 2))))) >> 28;   // the nibble, sign-extended
      nbad += k == -8;
      f[8 * w + i] = e2m3(k == -8 ? 0 : k);
    }
  if (nbad) atomicAdd(bad, nbad);
  uint4 head;
  uint2 tail;
  pack32(f, head, tail);
  const int ln = (rr & 15) + 16 * (int)(g & 3);
  uint8_t* dst = out + (tn * (kpad / 128) + kt) * F6_CHUNK + (rr >> 4) * F6_WGROUP;
  *reinterpret_cast<uint4*>(dst + 16 * ln) = head;
  *reinterpret_cast<uint2*>(dst + 1024 + 8 * ln) = tail;
}

int64_t f6_tiles(int64_t M, int64_t npad) { return (npad / F6_BN) * ((M + F6_BM - 1) / F6_BM); }

// the shapes the GEMM takes: K within the fp32 accumulator's exact range, rows and columns in int32, tiles in a 2^30
// grid
bool f6_sizes_ok(int64_t M, int64_t K, int64_t N, int64_t npad) {
  if (M < 0 || M > INT32_MAX / 2 || K <= 0 || K % QVIT_TILE_K || K > F6_MAX_K) return false;
  if (N <= 0 || npad < N || npad % QVIT_TILE_N || npad > INT32_MAX / 2) return false;
  return f6_tiles(M, npad) <= (1 << 30);
}

template <int EPI>
int launch(const uint8_t* A, int64_t M, int64_t K, int64_t ldp, const void* Wp, int64_t N, int64_t npad, void* C,
           int64_t ldc, const Epi16Args& ep, hipStream_t stream) {
  const unsigned grid = (unsigned)((f6_tiles(M, npad) + 7) / 8 * 8);
  hipLaunchKernelGGL((gemm_f6_kernel<EPI>), dim3(grid), dim3(256), 0, stream, A, (int)M, (int)K, ldp,
                     reinterpret_cast<const uint8_t*>(Wp), (int)N, (int)npad, C, ldc, ep);
  return qvit_launch_status();
}

}  // namespace

extern "C" int qvit_quantize_act_f6(const float* x, int64_t rows, int64_t cols, int64_t ldx, int qtype,
                                    const float* d_quant, const float* q_m, const float* t_quant, int levels,
                                    uint8_t* out, int64_t ldp, int64_t kpad, hipStream_t stream) {
  if (!x || !out) return QVIT_ENULL;
  if (qvit_quant_status(qtype, d_quant, q_m, levels)) return QVIT_EINVAL;
  if (rows < 0 || cols < 0 || ldx < cols || kpad < cols || kpad % QVIT_TILE_K || ldp < kpad / 4 * 3) return QVIT_EINVAL;
  if ((ldp % 16) || qvit_misaligned(15, out)) return QVIT_EALIGN;
  if (rows == 0 || kpad == 0) return QVIT_OK;
  const int64_t work = rows * (kpad / 32);
  hipLaunchKernelGGL(rows_to_f6_kernel, dim3(grid_for(work, kThreads)), dim3(kThreads), 0, stream, x, rows, cols, ldx,
                     qtype, d_quant, q_m, t_quant, levels, out, ldp, kpad);
  return qvit_launch_status();
}

extern "C" int qvit_pack_weight_f6(const void* packed, int64_t npad, int64_t kpad, void* out, int32_t* bad_codes,
                                   hipStream_t stream) {
  if (!packed || !out || !bad_codes) return QVIT_ENULL;
  if (npad <= 0 || npad % QVIT_TILE_N || kpad <= 0 || kpad % QVIT_TILE_K || npad > INT32_MAX / 2 || kpad > F6_MAX_K)
    return QVIT_EINVAL;
  if (qvit_misaligned(15, packed, out) || qvit_misaligned(3, bad_codes)) return QVIT_EALIGN;
  if (packed == out) return QVIT_EINVAL;   // not in place
  const int64_t work = npad * (kpad / 32);
  hipLaunchKernelGGL(pack_w6f_kernel, dim3((unsigned)((work + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                     reinterpret_cast<const uint8_t*>(packed), npad, kpad, reinterpret_cast<uint8_t*>(out), bad_codes);
  return qvit_launch_status();
}

extern "C" int qvit_gemm_f6_fits(int64_t M, int64_t K, int64_t N, int64_t npad, int epilogue) {
  return f6_sizes_ok(M, K, N, npad) && epilogue >= QVIT_EPI_F32 && epilogue <= QVIT_EPI_I32 ? 1 : 0;
}

extern "C" int qvit_gemm_f6(const uint8_t* A, int64_t M, int64_t K, int64_t ldp, const void* Wp, int64_t N,
                            int64_t npad, const float* d_act, const float* d_wt, const float* bias, int epilogue,
                            void* C, int64_t ldc, int out_qtype, const float* out_d, const float* out_qm,
                            const float* out_t, int out_levels, const void* epi_table, hipStream_t stream) {
  // qvit_gemm_a4's checks, in its order, on this kernel's shapes
  if (!A || !Wp || !C) return QVIT_ENULL;
  if (!f6_sizes_ok(M, K, N, npad) || ldp < K / 4 * 3) return QVIT_EINVAL;
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
  switch (epilogue) {
    case QVIT_EPI_F32: return launch<QVIT_EPI_F32>(A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
    case QVIT_EPI_F32_RESID: return launch<QVIT_EPI_F32_RESID>(A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
    case QVIT_EPI_I8_GELU: return launch<QVIT_EPI_I8_GELU>(A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
    case QVIT_EPI_I8: return launch<QVIT_EPI_I8>(A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
    default: return launch<QVIT_EPI_I32>(A, M, K, ldp, Wp, N, npad, C, ldc, ep, stream);
  }
}
