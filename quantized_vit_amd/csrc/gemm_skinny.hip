// Skinny-M split-K schedule of the quantized contraction (quant_layers.py:495-499), for the row counts at which
// qvit_gemm's 128 x 256 persistent tiles leave most of the machine idle (M = 197 .. ~1600: single-image and
// small-batch ViT inference, the class-token tail of the last block). Same operands, same exact int32 accumulation on
// v_mfma_i32_16x16x64_i8 and the same epilogue arithmetic as gemm_kernel (gemm_w4a8.hip): the results are qvit_gemm's
// byte for byte, a split-K sum of int32 partials being exact in any order.
//
// Work split: one workgroup (4 waves) = 64 activation rows x 64 weight rows x one K-slice; grid = ceil(M / 64) x
//   npad / 64 x S. S splits K into slices of whole 128-deep k-tiles (the first K/128 % S slices hold one more), chosen
//   on the host so that the grid covers the CUs about twice. Wave w owns rows 16 w .. 16 w + 15 and all 64 weight rows:
//   4 MFMAs per 64-deep k-step, 16 accumulator registers.
// Operands: no LDS and no barrier in the main loop. A 64-row weight tile is one "wave quarter" of the QVIT_W4R image
//   (lane l: 32 contiguous bytes at 2048 q + 32 l of every (256-row tile, stage) chunk = its four 8-B fragments), or 64
//   rows of the QVIT_W8 image (four 16-B fragments per lane, the image's chunk swizzle undone through the address);
//   every wave loads the tile's weights (the three repeats hit the CU's vector cache) and 16 B of its own activation
//   rows per k-step. Loads are plain (compiler-counted) global loads, a ring of RING k-tiles deep in registers:
//   RING = 4 k-tiles = 8 k-steps = 64 + 32 VGPRs on W4R (128 + 32 on W8), so a slice of up to 4 k-tiles (every slice
//   of the automatic split) has all of its loads in flight before the first MFMA; a longer slice reloads each ring
//   entry behind its MFMAs in a rolled loop.
// Reduce and epilogue in the same launch (S > 1): a workgroup stores its 64 x 64 int32 partial into its workspace slot
//   [tile][slice], arrives at the tile's counter, and the last arriver adds the other S - 1 slots to its registers,
//   resets the counter and runs the epilogue. The ordering argument is at `reduce` below.
// Epilogue: a lane's 16 accumulators are 16 consecutive columns of one row (the weight-row permutation of
//   qvit_pack_weight), so it needs no staging: 64 B of fp32 / int32 or one 16-B code store per lane and row.
#include <cstddef>

#include "qvit_common.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int TM = 64;          // activation rows per workgroup
constexpr int TN = 64;          // weight rows per workgroup
constexpr int BK = 64;          // k per MFMA step
constexpr int KTILE = 128;      // the API's K granularity (QVIT_TILE_K): two steps
constexpr int RING = 4;         // k-tiles in flight per wave
constexpr int MAX_SPLITS = 16;
constexpr int64_t MAX_M = 4096;
constexpr int64_t MAX_TILES = 16384;                  // 64 KiB of arrival counters at the head of the workspace
constexpr int64_t CNT_BYTES = MAX_TILES * 4;
constexpr int64_t PART_BYTES = TM * TN * 4;           // one partial: 16 KiB
constexpr int64_t MAX_SLOTS = (int64_t(1) << 31) / PART_BYTES - 1;   // the partials are addressed through one buffer

// int4 codes as the signed bytes 16 w (a nibble in the high half of its byte), as in gemm_w4a8.hip: the accumulators
// hold 16 acc exactly and the epilogue folds the 1/16 into alpha (or shifts it away for QVIT_EPI_I32)
QVIT_DEV uint32_t nib16_lo(uint32_t p) { return (p << 4) & 0xF0F0F0F0u; }
QVIT_DEV uint32_t nib16_hi(uint32_t p) { return p & 0xF0F0F0F0u; }

struct SkinnyArgs {
  const float* d_act;
  const float* d_wt;
  const float* bias;
  int out_qtype;
  const float* out_d;
  const float* out_qm;
  const float* out_t;
  int out_levels;
  const int8_t* table;   // optional code table of the int8 epilogues (qvit_epi_table_build)
  int* counters;         // S > 1: one arrival counter per output tile (zero between launches)
  int8_t* parts;         // S > 1: partial slots [tile][slice], PART_BYTES each
  int parts_bytes;
};

// One 128-deep k-tile of a wave's operands: two steps of 16 B of activations and the weight fragments as loaded
template <int WFMT>
struct KTileRegs {
  static constexpr int NW = (WFMT == QVIT_W4R) ? 2 : 4;
  v4i x[2];
  v4i w[2][NW];
};

template <int WFMT, int EPI>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(const int8_t* __restrict__ A, int M, int K, int64_t lda,
                                                          const int8_t* __restrict__ Wp, int N, int npad,
                                                          void* __restrict__ C, int64_t ldc, int S, SkinnyArgs ep) {
  constexpr bool W4 = WFMT == QVIT_W4R;
  constexpr bool I8OUT = (EPI == QVIT_EPI_I8 || EPI == QVIT_EPI_I8_GELU);
  __shared__ QParams qp_l;
  __shared__ int last_l;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;

  // ---- this workgroup's (tile_m, slice, tile_n) ------------------------------------------------------------------
  // workgroups are dispatched round-robin over the 8 XCDs: XCD x takes the contiguous range [lo_x, lo_x + cnt_x) of
  // the logical ids, tile_m fastest, then the slice, so the workgroups that share a weight slice, and the slices of
  // one tile, mostly share an L2
  const int total = gridDim.x;
  const int xcd = blockIdx.x & 7, per = total >> 3, rem = total & 7;
  const int id = xcd * per + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);
  const int tiles_m = (M + TM - 1) / TM;
  const int tm = id % tiles_m;
  const int rest = id / tiles_m;
  const int slice = rest % S, tn = rest / S;
  const int tile = tn * tiles_m + tm;
  const int m0 = tm * TM, n0 = tn * TN;
  const int nkt_all = K / KTILE;
  const int kbase = nkt_all / S, krem = nkt_all % S;
  const int kt0 = slice * kbase + (slice < krem ? slice : krem);   // first k-tile of the slice
  const int nkt = kbase + (slice < krem ? 1 : 0);                  // >= 1 (S <= K / 128)

  // the direct quantizer's scalars (double-precision exp / log) once per workgroup, when no valid table is passed
  bool use_table = false;
  float t_c0 = 0.f, t_invw = 0.f, t_top = 0.f;
  if constexpr (I8OUT) {
    if (ep.table != nullptr) {
      const EpiTableHdr h = *reinterpret_cast<const EpiTableHdr*>(ep.table);
      use_table = h.valid != 0 && h.nb >= 1 && h.nb <= QVIT_EPI_TABLE_MAX_NB;
      t_c0 = h.c0;
      t_invw = h.inv_w;
      t_top = epi_top(h.nb);
    }
    if (!use_table && tid == 0) qp_l = load_qparams(ep.out_qtype, ep.out_d, ep.out_qm, ep.out_t, ep.out_levels);
  }

  // ---- operand addresses -------------------------------------------------------------------------------------------
  // activations: lane l reads 16 B of row m0 + 16 w + (l & 15) at k offset 16 (l >> 4) of every step; rows past M read
  // row M - 1 (never stored)
  int arow = m0 + 16 * wave + fr;
  arow = arow < M ? arow : M - 1;
  const int8_t* ap = A + (int64_t)arow * lda + 16 * fq;
  // weights: the (256-row tile, stage) chunks of this tile's image, stage-major; inside a chunk the tile's quarter
  const int nk = K / BK;
  constexpr int CHUNK = W4 ? 8192 : 16384;
  const int q = tn & 3;
  const int8_t* wp = Wp + (int64_t)(tn >> 2) * nk * CHUNK +
                     (W4 ? 2048 * q + 32 * lane : (64 * q + fr) * 64 + ((fq ^ (((fr >> 2) & 1) << 1)) << 4));

  auto load_ktile = [&](KTileRegs<WFMT>& f, int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int st = 2 * kt + s;
      f.x[s] = *reinterpret_cast<const v4i*>(ap + st * BK);
      const int8_t* ws = wp + (int64_t)st * CHUNK;
#pragma unroll
      for (int i = 0; i < KTileRegs<WFMT>::NW; ++i)
        f.w[s][i] = *reinterpret_cast<const v4i*>(ws + (W4 ? 16 * i : 1024 * i));   // W8: rows 16 i further
    }
  };

  // acc[r][j] = sum over the slice of A[m0 + 16 w + fr][k] W[n0 + 16 fq + 4 r + j][k]  (x 16 on W4R; the packed rows
  // 16 r + 4 fq + j of the tile hold those weight rows: qvit_pack_weight's permutation)
  v4i acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = v4i{0, 0, 0, 0};
  auto mfma_ktile = [&](const KTileRegs<WFMT>& f) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v4i wf;
        if constexpr (W4) {
          const v4i p = f.w[s][r >> 1];
          const uint32_t px = (uint32_t)p[2 * (r & 1)], py = (uint32_t)p[2 * (r & 1) + 1];
          wf = v4i{(int)nib16_lo(px), (int)nib16_hi(px), (int)nib16_lo(py), (int)nib16_hi(py)};
        } else {
          wf = f.w[s][r];
        }
        acc[r] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf, f.x[s], acc[r], 0, 0, 0);
      }
  };

  // ---- main loop: RING k-tiles of loads ahead of the MFMAs (all conditions are workgroup-uniform) -------------------
  KTileRegs<WFMT> ring[RING];
#pragma unroll
  for (int j = 0; j < RING; ++j)
    if (j < nkt) load_ktile(ring[j], kt0 + j);
#pragma unroll 1
  for (int base = 0; base < nkt; base += RING) {
#pragma unroll
    for (int j = 0; j < RING; ++j) {
      if (base + j < nkt) {
        mfma_ktile(ring[j]);
        if (base + j + RING < nkt) load_ktile(ring[j], kt0 + base + j + RING);
      }
    }
  }

  // ---- reduce (S > 1) --------------------------------------------------------------------------------------------
  // The MI355X's eight XCDs have L2s that are not coherent with each other, and the slices of a tile may run on any of
  // them. Ordering, as at ln_after_tile (gemm_w4a8.hip):
  //   1. every wave writes its part of the partial through its L2 (sc1 stores) and waits for vmcnt(0): the stores
  //      have been acknowledged by memory;
  //   2. the workgroup barrier: all four waves are past their wait;
  //   3. thread 0 arrives at the tile's counter with one agent-scope atomic (performed at memory, past every L2);
  //      arrivals are totally ordered there, so exactly one workgroup reads S - 1: every other workgroup's step 1
  //      precedes its own arrival, which precedes this one;
  //   4. the last arriver's loads are issued after the atomic returned (they sit behind the barrier that publishes
  //      the flag) and read past its own L2 (sc1 loads), so they see what step 1 wrote, not a stale line of an
  //      earlier launch.
  // The last arriver resets the counter (nobody else touches it any more in this launch): the workspace is left as it
  // was found, counters zero, and needs no clearing launch before the next call on the same stream.
  if (S > 1) {
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(ep.parts, (short)0, ep.parts_bytes, 0x00020000);
    const int lane_off = tid * 16;   // slot image: accumulator r of thread t at 4096 r + 16 t (coalesced)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      __builtin_amdgcn_raw_buffer_store_b128(acc[r], rs, (tile * S + slice) * (int)PART_BYTES + 4096 * r + lane_off, 0,
                                             16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      const int old = __hip_atomic_fetch_add(ep.counters + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last_l = old == S - 1 ? 1 : 0;
      if (old == S - 1) __hip_atomic_store(ep.counters + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (last_l == 0) return;   // workgroup-uniform
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
      if (s == slice) continue;
      v4i p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        p[r] = __builtin_amdgcn_raw_buffer_load_b128(rs, (tile * S + s) * (int)PART_BYTES + 4096 * r + lane_off, 0, 16);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] += p[r];
    }
  } else if constexpr (I8OUT) {
    __syncthreads();   // qp_l
  }

  // ---- epilogue: row m, columns nb + 4 r + j (the arithmetic of gemm_kernel's epilogues) ----------------------------
  const int m = m0 + 16 * wave + fr;
  const int nb = n0 + 16 * fq;
  if (m >= M || nb >= N) return;
  if constexpr (EPI == QVIT_EPI_I32) {
    int32_t* dst = reinterpret_cast<int32_t*>(C) + (int64_t)m * ldc + nb;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v4i a = acc[r];
      if constexpr (W4) a = v4i{a[0] >> 4, a[1] >> 4, a[2] >> 4, a[3] >> 4};   // 16 acc -> acc (exact)
      if (nb + 4 * r + 4 <= N) {
        *reinterpret_cast<v4i*>(dst + 4 * r) = a;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (nb + 4 * r + j < N) dst[4 * r + j] = a[j];
      }
    }
    return;
  }
  const float alpha = (*ep.d_act) * (*ep.d_wt) * (W4 ? 0.0625f : 1.f);
  float v[16];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ep.bias != nullptr) b = *reinterpret_cast<const float4*>(ep.bias + nb + 4 * r);
    v[4 * r + 0] = fmaf(alpha, (float)acc[r][0], b.x);
    v[4 * r + 1] = fmaf(alpha, (float)acc[r][1], b.y);
    v[4 * r + 2] = fmaf(alpha, (float)acc[r][2], b.z);
    v[4 * r + 3] = fmaf(alpha, (float)acc[r][3], b.w);
  }
  if constexpr (EPI == QVIT_EPI_F32 || EPI == QVIT_EPI_F32_RESID) {
    float* dst = reinterpret_cast<float*>(C) + (int64_t)m * ldc + nb;
    float4 old[4];
    if constexpr (EPI == QVIT_EPI_F32_RESID) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (nb + 4 * r + 4 <= N) old[r] = *reinterpret_cast<const float4*>(dst + 4 * r);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (nb + 4 * r + 4 <= N) {
        float4 o = make_float4(v[4 * r], v[4 * r + 1], v[4 * r + 2], v[4 * r + 3]);
        if constexpr (EPI == QVIT_EPI_F32_RESID) {
          o.x += old[r].x; o.y += old[r].y; o.z += old[r].z; o.w += old[r].w;
        }
        *reinterpret_cast<float4*>(dst + 4 * r) = o;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (nb + 4 * r + j < N)
            dst[4 * r + j] = (EPI == QVIT_EPI_F32_RESID) ? dst[4 * r + j] + v[4 * r + j] : v[4 * r + j];
      }
    }
  } else {
    // int8 codes: the table's entry {thr, lo | hi << 8} of v's bucket (read from memory: 16 entries per lane), or the
    // quantizer itself; both give the same code for every v (the table is built from this very function)
    uint32_t wd[4] = {0u, 0u, 0u, 0u};
    if (use_table) {
      const int8_t* ent = ep.table + sizeof(EpiTableHdr);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint2 e = *reinterpret_cast<const uint2*>(ent + 8 * epi_bucket(v[i], t_c0, t_invw, t_top));
        const uint32_t code = (v[i] >= __uint_as_float(e.x)) ? ((e.y >> 8) & 0xffu) : (e.y & 0xffu);
        wd[i >> 2] |= code << (8 * (i & 3));
      }
    } else {
      const QParams qp = qp_l;
#pragma unroll 1
      for (int i = 0; i < 16; ++i) {
        const float x = (EPI == QVIT_EPI_I8_GELU) ? gelu_ref(v[i]) : v[i];
        const uint32_t code = (uint32_t)(uint8_t)to_i8_sat(quant_code(x, qp));
        // (a rolled loop: one copy of the quantizer; the word index is dynamic, so select it without indexing)
        const uint32_t sh = code << (8 * (i & 3));
        wd[0] |= (i >> 2) == 0 ? sh : 0u;
        wd[1] |= (i >> 2) == 1 ? sh : 0u;
        wd[2] |= (i >> 2) == 2 ? sh : 0u;
        wd[3] |= (i >> 2) == 3 ? sh : 0u;
      }
    }
    int8_t* dst = reinterpret_cast<int8_t*>(C) + (int64_t)m * ldc + nb;
    const bool fast16 = ((ldc & 15) == 0) && ((((uintptr_t)C) & 15) == 0) && ((N & 15) == 0);
    if (fast16) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (nb + 4 * r + 4 <= N) {
          *reinterpret_cast<uint32_t*>(dst + 4 * r) = wd[r];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (nb + 4 * r + j < N) dst[4 * r + j] = (int8_t)((wd[r] >> (8 * j)) & 0xff);
        }
      }
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
int64_t tiles_of(int64_t M, int64_t npad) { return ((M + TM - 1) / TM) * (npad / TN); }

// S = clamp(2 CUs / tiles, 1, min(K / 128, 16)): the grid covers the CUs about twice
int auto_splits(int64_t M, int64_t K, int64_t npad) {
  const int64_t tiles = tiles_of(M, npad);
  int64_t s = tiles > 0 ? 2 * (int64_t)qvit_device_cus() / tiles : 1;
  const int64_t cap = K / KTILE < MAX_SPLITS ? K / KTILE : MAX_SPLITS;
  s = s > cap ? cap : s;
  return (int)(s < 1 ? 1 : s);
}

// the shapes shared by the three entry points
bool shape_ok(int64_t M, int64_t K, int64_t npad) {
  return M >= 0 && M <= MAX_M && K > 0 && K % KTILE == 0 && K <= (1 << 24) && npad > 0 && npad % QVIT_TILE_N == 0 &&
         tiles_of(M, npad) <= MAX_TILES;
}

// splits -> S (0: the automatic rule), or 0 when the forced value is out of range
int resolve_splits(int64_t M, int64_t K, int64_t npad, int splits) {
  if (splits < 0 || splits > MAX_SPLITS || splits > K / KTILE) return 0;
  const int S = splits > 0 ? splits : auto_splits(M, K, npad);
  return tiles_of(M, npad) * S <= MAX_SLOTS ? S : 0;
}

template <int WFMT, int EPI>
int launch(const int8_t* A, int64_t M, int64_t K, int64_t lda, const void* Wp, int64_t N, int64_t npad, void* C,
           int64_t ldc, int S, const SkinnyArgs& ep, hipStream_t stream) {
  const int64_t grid = tiles_of(M, npad) * S;
  hipLaunchKernelGGL((gemm_skinny_kernel<WFMT, EPI>), dim3((unsigned)grid), dim3(256), 0, stream, A, (int)M, (int)K,
                     lda, reinterpret_cast<const int8_t*>(Wp), (int)N, (int)npad, C, ldc, S, ep);
  return qvit_launch_status();
}

template <int WFMT>
int dispatch_epi(int epilogue, const int8_t* A, int64_t M, int64_t K, int64_t lda, const void* Wp, int64_t N,
                 int64_t npad, void* C, int64_t ldc, int S, const SkinnyArgs& ep, hipStream_t stream) {
  switch (epilogue) {
    case QVIT_EPI_F32: return launch<WFMT, QVIT_EPI_F32>(A, M, K, lda, Wp, N, npad, C, ldc, S, ep, stream);
    case QVIT_EPI_F32_RESID: return launch<WFMT, QVIT_EPI_F32_RESID>(A, M, K, lda, Wp, N, npad, C, ldc, S, ep, stream);
    case QVIT_EPI_I8_GELU: return launch<WFMT, QVIT_EPI_I8_GELU>(A, M, K, lda, Wp, N, npad, C, ldc, S, ep, stream);
    case QVIT_EPI_I8: return launch<WFMT, QVIT_EPI_I8>(A, M, K, lda, Wp, N, npad, C, ldc, S, ep, stream);
    case QVIT_EPI_I32: return launch<WFMT, QVIT_EPI_I32>(A, M, K, lda, Wp, N, npad, C, ldc, S, ep, stream);
    default: return QVIT_EINVAL;
  }
}

}  // namespace

extern "C" int qvit_gemm_skinny_fits(int64_t M, int64_t K, int wfmt, int64_t N, int64_t npad, int epilogue) {
  if (wfmt != QVIT_W4R && wfmt != QVIT_W8) return 0;
  if (M < 1 || !shape_ok(M, K, npad) || N <= 0 || npad < N) return 0;
  if (wfmt != QVIT_W8 && K > 65536) return 0;
  return epilogue >= QVIT_EPI_F32 && epilogue <= QVIT_EPI_I32;
}

extern "C" int qvit_gemm_skinny_workspace(int64_t M, int64_t K, int64_t npad, int splits, size_t* bytes) {
  if (!bytes) return QVIT_ENULL;
  if (!shape_ok(M, K, npad)) return QVIT_EINVAL;
  const int S = resolve_splits(M, K, npad, splits);
  if (S == 0) return QVIT_EINVAL;
  *bytes = S > 1 ? (size_t)(CNT_BYTES + tiles_of(M, npad) * S * PART_BYTES) : 0;
  return QVIT_OK;
}

extern "C" int qvit_gemm_skinny(const int8_t* A, int64_t M, int64_t K, int64_t lda, const void* Wp, int wfmt, int64_t N,
                                int64_t npad, const float* d_act, const float* d_wt, const float* bias, int epilogue,
                                void* C, int64_t ldc, int out_qtype, const float* out_d, const float* out_qm,
                                const float* out_t, int out_levels, const void* epi_table, int splits, void* workspace,
                                size_t workspace_bytes, hipStream_t stream) {
  // qvit_gemm's checks, in its order
  if (!A || !Wp || !C) return QVIT_ENULL;
  if (wfmt != QVIT_W4 && wfmt != QVIT_W4R && wfmt != QVIT_W8R && wfmt != QVIT_W8) return QVIT_EINVAL;
  if (M < 0 || K <= 0 || K % KTILE || lda < K || N <= 0 || npad < N || npad % QVIT_TILE_N) return QVIT_EINVAL;
  if (M > INT32_MAX / 2 || npad > INT32_MAX / 2 || K > (1 << 24)) return QVIT_EINVAL;
  if (wfmt != QVIT_W8 && K > 65536) return QVIT_EINVAL;  // 16x-scaled int32 accumulation bound
  if ((lda % 16) || qvit_misaligned(15, A, Wp)) return QVIT_EALIGN;
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
  if (qvit_misaligned(15, bias)) return QVIT_EALIGN;
  // this schedule's own: the two weight images it reads, its row limit, the split and the workspace
  if (wfmt != QVIT_W4R && wfmt != QVIT_W8) return QVIT_EINVAL;
  if (!shape_ok(M, K, npad)) return QVIT_EINVAL;
  if (splits < 0 || splits > MAX_SPLITS || splits > K / KTILE) return QVIT_EINVAL;
  if (M == 0) return QVIT_OK;
  if (qvit_misaligned(15, epi_table)) return QVIT_EALIGN;
  const int S = resolve_splits(M, K, npad, splits);
  if (S == 0) return QVIT_EINVAL;
  const int64_t parts = tiles_of(M, npad) * S * PART_BYTES;
  if (S > 1) {
    if (!workspace) return QVIT_ENULL;
    if (workspace_bytes < (size_t)(CNT_BYTES + parts)) return QVIT_EINVAL;
    if (qvit_misaligned(15, workspace)) return QVIT_EALIGN;
  }
  SkinnyArgs ep{d_act, d_wt, bias, out_qtype, out_d, out_qm, out_t, out_levels,
                (i8out ? reinterpret_cast<const int8_t*>(epi_table) : nullptr),
                reinterpret_cast<int*>(workspace),
                S > 1 ? reinterpret_cast<int8_t*>(workspace) + CNT_BYTES : nullptr, (int)(S > 1 ? parts : 0)};
  if (wfmt == QVIT_W4R) return dispatch_epi<QVIT_W4R>(epilogue, A, M, K, lda, Wp, N, npad, C, ldc, S, ep, stream);
  return dispatch_epi<QVIT_W8>(epilogue, A, M, K, lda, Wp, N, npad, C, ldc, S, ep, stream);
}
