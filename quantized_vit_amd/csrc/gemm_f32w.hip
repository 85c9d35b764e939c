// fp32 activations x frozen fp32 weights at fp32-GEMM accuracy on bf16 MFMA: the nn.Linear calls of a model that is
// built once and never trained, the distillation teacher of the reference's driver (train.py:290-316 builds
// create_model(...), leaves it unquantized, puts it in eval() and freezes it; utils.py:268-274 runs it once per step
// under no_grad). gemm_f32.hip splits both operands into bf16 terms on every stage; a frozen weight is split ONCE,
// into an image that already has the GEMM's LDS stage layout, and the GEMM copies it to LDS without touching it.
//   C[m][n] = epi(sum_k A[m][k] W[n][k] + bias[n])     A fp32 [M][K], W the QVIT_WB3 image of fp32 [N][K]
//
// QVIT_WB3 (qvit_pack_weight_b3): per (128-row weight tile tn, 32-deep stage st) `planes` planes of [128][32] bf16,
// 8 KiB each, the terms b1, b2 (, b3) of split_bf16x3; in a plane, 16-byte chunk c of row r at 64 r + 16 (c ^ ((r >> 2)
// & 3)) (gemm_f32.hip's NT swizzle). Planes contiguous, stages contiguous within a tile: stage (tn, st) starts at
// ((tn nst + st) planes) 8 KiB, nst = ceil(K / 32). Rows past N and columns past K hold zero.
//
// Arithmetic (TERMS): 6 is gemm_f32.hip's: a3b1, a1b3, a2b2, a2b1, a1b2, a1b1 into one fp32 accumulator per 32-deep
// stage, in that order, on a three-plane image: its bound (4 K + 9) 2^-24 (|A||W|) holds unchanged. 3 keeps a2b1,
// a1b2, a1b1 on a two-plane image with the activations split into two terms: it drops a2b2 (< 2^-14 |a||w|),
// a1b3 + a3b1 (< 2^-14) and the rest (< 2^-20), so it adds (2^-13 + 2^-20) (|A||W|) to the bound.
// No atomics, a fixed stage order, no split of K: the same call gives the same bits. A NaN or Inf in A[m][k] makes
// row m of C NaN and changes no other bit (the zeros of the image's padding stand in columns that are never stored).
//
// Schedule: gemm_f32.hip's tile (128 x 128, 4 waves 2 x 2, a wave owns 64 x 64, XCD-contiguous walk with n tiles
// fastest). LDS holds TWO weight stage buffers and ONE activation stage buffer:
//   weights      a stage's planes are one contiguous run of 24 KiB (16 KiB with two planes) in LDS order: every wave
//                copies its quarter with global_load_lds_dwordx4 (1-KiB pieces). No register, no VALU.
//   activations  4 float4 per thread and stage into registers (half of gemm_f32.hip's staging), split, ds_write.
//   step st      wait (own DMA pieces of st landed, own ds_writes of st retired), barrier, the activation loads of
//                st + 1 and then the DMA of st + 1 (into the other weight buffer) issued, fragments and MFMAs of st,
//                barrier (the activation buffer's readers are done), the activations of st + 1 split and written.
// Behind the first barrier of st every wave has finished reading the other weight buffer (stage st - 1), so the DMA
// of st + 1 may overwrite it while st computes: the weight stream is a whole stage ahead and never waits for a
// barrier. The DMA is issued from asm: the compiler does not count it, so the wait in front of the first barrier is
// an explicit s_waitcnt vmcnt(0) lgkmcnt(0); nothing else is in flight there (the activation registers of that stage
// were consumed by the split before it). The activation loads are plain loads: the counter is in order, so the DMA
// pieces around them can only make the compiler's own waits stronger, never weaker. They stand in front of the DMA
// because the compiler waits for vmcnt(0) before it overwrites their registers: there the wait finds nothing in
// flight, behind the DMA it would drain the stage just requested (seen in the assembly).
// LDS and registers (compiler's report): TERMS 6 nine planes = 72 KiB and 172 VGPRs, two workgroups per CU; TERMS 3
// six planes = 48 KiB and 146 VGPRs, three per CU. A second activation buffer (one barrier per stage) was built and measured:
// TERMS 6 then needs 96 KiB, ONE workgroup per CU, and ran 137 to 168 TFLOP/s against 183 to 207 with this layout on
// the eight ViT-B / ViT-L shapes; TERMS 3 (64 KiB, two per CU) ran 280 to 364 against 311 to 372. Dropped.
#include "gemm_f32_common.h"

namespace {

constexpr int FW_MAX_EXTENT = 1 << 24;
constexpr int FW_MAX_K = 1 << 30;

// own DMA pieces landed, own LDS writes and reads retired
QVIT_DEV void fw_drain() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }

template <int EPI>
QVIT_DEV float fw_epi(float v, float old) {
  if constexpr (EPI == QVIT_EPI_F32_GELU) return gelu_ref(v);
  if constexpr (EPI == QVIT_EPI_F32_RESID) return old + v;
  return v;
}

template <int TERMS, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_f32w_kernel(
    const float* __restrict__ A, int M, int K, int64_t lda, const int8_t* __restrict__ Wimg, int N,
    const float* __restrict__ bias, float* C, int64_t ldc, int nb_n, int total) {
  constexpr int PL = TERMS == 6 ? 3 : 2;          // planes per operand
  constexpr int WRUN = PL * FG_PLANE;             // a stage of the image: the DMA run
  constexpr int AOFF = 2 * WRUN;                  // two weight buffers, then the activation buffer
  constexpr int NP = WRUN / 1024 / 4;             // 1-KiB DMA pieces per wave and stage
  __shared__ __attribute__((aligned(16))) int8_t smem[3 * WRUN];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int u = xcd_unit(total);
  if (u >= total) return;
  const int tn = u % nb_n;
  const int m0 = (u / nb_n) * FG_BT, n0 = tn * FG_BT;
  const int nst = (K + FG_BK - 1) / FG_BK;

  // ---- weights: this wave's pieces NP wave .. NP wave + NP - 1 of stage st, 16 bytes per lane. The source is a
  // scalar base plus one loop-invariant lane offset: the DMA section writes no vector register, so the compiler has
  // no reason to put a wait of its own between the pieces.
  const int8_t* const wsrc = Wimg + (int64_t)tn * nst * WRUN + (NP * wave) * 1024;
  const uint32_t lds0 = lds_addr(smem), lane16 = 16 * lane;
  auto dma = [&](int st, int buf) __attribute__((always_inline)) {
    const int8_t* src = wsrc + (int64_t)st * WRUN;
#pragma unroll
    for (int p = 0; p < NP; ++p)
      dma16s(src + 1024 * p, lane16, __builtin_amdgcn_readfirstlane(lds0 + buf * WRUN + (NP * wave + p) * 1024));
  };

  // ---- activations: rows lr + 32 j (clamped), k = 4 lq .. 4 lq + 3 of the stage
  const int lr = tid >> 3, lq = tid & 7;
  const float* arow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) arow[j] = A + (int64_t)min(m0 + lr + 32 * j, M - 1) * lda + 4 * lq;
  f4 av[4];
  auto load = [&](int st) __attribute__((always_inline)) {
    const int kk = st * FG_BK + 4 * lq;   // kk < K and lda >= K rounded up to 4: the float4 stays in its row
#pragma unroll
    for (int j = 0; j < 4; ++j)
      av[j] = kk < K ? *reinterpret_cast<const f4*>(arow[j] + st * FG_BK) : f4{0.f, 0.f, 0.f, 0.f};
  };
  int8_t* const wr = smem + AOFF + nt_off(lr, lq >> 1) + 8 * (lq & 1);   // row lr + 32 j: + 2048 j
  auto stash = [&](int st) __attribute__((always_inline)) {
    if (st * FG_BK + FG_BK > K) {   // the ragged last stage (uniform): what lies past K may be anything
      const int kk = st * FG_BK + 4 * lq;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 1; e < 4; ++e)
          if (kk + e >= K) av[j][e] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint2 p1, p2, p3;
      split4(av[j], p1, p2, p3);
      int8_t* d = wr + 2048 * j;
      *reinterpret_cast<uint2*>(d) = p1;
      *reinterpret_cast<uint2*>(d + FG_PLANE) = p2;
      if constexpr (PL == 3) *reinterpret_cast<uint2*>(d + 2 * FG_PLANE) = p3;
    }
  };
  // fragments: row 16 t + fr of the wave's 64, k = 8 fq .. 8 fq + 7 (tile t: + 1024)
  const int8_t* const bfrag = smem + nt_off(64 * wn + fr, fq);
  const int8_t* const afrag = smem + AOFF + nt_off(64 * wm + fr, fq);

  f4 acc[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};

  load(0);
  dma(0, 0);
  stash(0);
#pragma unroll 1
  for (int st = 0; st < nst; ++st) {
    const int buf = st & 1;
    fw_drain();
    __syncthreads();
    if (st + 1 < nst) {
      load(st + 1);   // in front of the DMA: the compiler's wait for the registers it overwrites finds nothing in flight
      dma(st + 1, buf ^ 1);
    }
    bf8 bf[4][PL];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int p = 0; p < PL; ++p)
        bf[nt][p] = *reinterpret_cast<const bf8*>(bfrag + buf * WRUN + p * FG_PLANE + 1024 * nt);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      bf8 af[PL];
#pragma unroll
      for (int p = 0; p < PL; ++p)
        af[p] = *reinterpret_cast<const bf8*>(afrag + p * FG_PLANE + 1024 * mt);
      // MFMA rows = W's rows n, columns = A's rows m: lane (fr, fq) holds C[m = 16 mt + fr][n = 16 nt + 4 fq + e]
      if constexpr (PL == 3) mma6(acc[mt], bf, af);
      else mma3(acc[mt], bf, af);
    }
    __syncthreads();   // the activation buffer's readers are done
    if (st + 1 < nst) stash(st + 1);
  }

#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int m = m0 + 64 * wm + 16 * mt + fr;
    if (m >= M) continue;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int n = n0 + 64 * wn + 16 * nt + 4 * fq;
      if (n >= N) continue;
      f4 v = acc[mt][nt];
      float* dst = C + (int64_t)m * ldc + n;
      if (n + 4 <= N) {
        if (bias) v += f4{bias[n], bias[n + 1], bias[n + 2], bias[n + 3]};
        f4 old = {0.f, 0.f, 0.f, 0.f};
        if constexpr (EPI == QVIT_EPI_F32_RESID) old = *reinterpret_cast<const f4*>(dst);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fw_epi<EPI>(v[e], old[e]);
        *reinterpret_cast<f4*>(dst) = v;
      } else {
        for (int e = 0; e < N - n; ++e) dst[e] = fw_epi<EPI>(v[e] + (bias ? bias[n + e] : 0.f), dst[e]);
      }
    }
  }
}

// one thread = 4 consecutive k of one image row: the split of gemm_f32.hip's stash, written once
__global__ __launch_bounds__(256) void pack_b3_kernel(const float* __restrict__ W, int N, int K, int64_t ldw,
                                                       int planes, int nst, int8_t* __restrict__ img,
                                                       int64_t groups) {
  for (int64_t id = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; id < groups;
       id += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(id / (8 * nst));
    const int g = (int)(id - (int64_t)r * (8 * nst));
    const int st = g >> 3, lq = g & 7;
    const int kk = st * FG_BK + 4 * lq;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < N && kk < K) {   // ldw >= K rounded up to 4: the float4 stays in its row
      v = *reinterpret_cast<const f4*>(W + (int64_t)r * ldw + kk);
#pragma unroll
      for (int e = 1; e < 4; ++e)
        if (kk + e >= K) v[e] = 0.f;
    }
    uint2 p1, p2, p3;
    split4(v, p1, p2, p3);
    int8_t* d = img + ((int64_t)(r >> 7) * nst + st) * planes * FG_PLANE + nt_off(r & 127, lq >> 1) + 8 * (lq & 1);
    *reinterpret_cast<uint2*>(d) = p1;
    *reinterpret_cast<uint2*>(d + FG_PLANE) = p2;
    if (planes == 3) *reinterpret_cast<uint2*>(d + 2 * FG_PLANE) = p3;
  }
}

bool b3_sizes_ok(int64_t N, int64_t K, int planes) {
  return (planes == 2 || planes == 3) && N >= 1 && N <= FW_MAX_EXTENT && K >= 1 && K <= FW_MAX_K;
}
int64_t b3_bytes(int64_t N, int64_t K, int planes) {
  return (round128(N) / FG_BT) * ((K + FG_BK - 1) / FG_BK) * planes * FG_PLANE;
}

template <int TERMS>
int launch_epi(int epilogue, const float* A, int64_t M, int64_t K, int64_t lda, const int8_t* Wimg, int64_t N,
               const float* bias, float* C, int64_t ldc, hipStream_t stream) {
  const int64_t nb_n = round128(N) / FG_BT, total = tiles128(M, N);
  const dim3 grid((unsigned)((total + 7) / 8 * 8)), block(256);
#define FW_LAUNCH(E)                                                                                             \
  hipLaunchKernelGGL((gemm_f32w_kernel<TERMS, E>), grid, block, 0, stream, A, (int)M, (int)K, lda, Wimg, (int)N, \
                     bias, C, ldc, (int)nb_n, (int)total)
  switch (epilogue) {
    case QVIT_EPI_F32: FW_LAUNCH(QVIT_EPI_F32); break;
    case QVIT_EPI_F32_RESID: FW_LAUNCH(QVIT_EPI_F32_RESID); break;
    default: FW_LAUNCH(QVIT_EPI_F32_GELU); break;
  }
#undef FW_LAUNCH
  return qvit_launch_status();
}

}  // namespace

extern "C" int64_t qvit_pack_weight_b3_bytes(int64_t N, int64_t K, int planes) {
  return b3_sizes_ok(N, K, planes) ? b3_bytes(N, K, planes) : (int64_t)QVIT_EINVAL;
}

extern "C" int qvit_pack_weight_b3(const float* W, int64_t N, int64_t K, int64_t ldw, int planes, void* image,
                                   int64_t image_bytes, hipStream_t stream) {
  if (!W || !image) return QVIT_ENULL;
  if (!b3_sizes_ok(N, K, planes) || ldw < K || image_bytes < b3_bytes(N, K, planes)) return QVIT_EINVAL;
  if ((ldw % 4) || qvit_misaligned(15, W, image)) return QVIT_EALIGN;
  const int64_t nst = (K + FG_BK - 1) / FG_BK, groups = round128(N) * nst * 8;
  const unsigned grid = (unsigned)((groups + 255) / 256 < 65536 ? (groups + 255) / 256 : 65536);
  hipLaunchKernelGGL(pack_b3_kernel, dim3(grid), dim3(256), 0, stream, W, (int)N, (int)K, ldw, planes, (int)nst,
                     reinterpret_cast<int8_t*>(image), groups);
  return qvit_launch_status();
}

extern "C" int qvit_gemm_f32w(const float* A, int64_t M, int64_t K, int64_t lda, const void* Wimg, int planes,
                              int64_t image_bytes, int64_t N, int terms, const float* bias, int epilogue, float* C,
                              int64_t ldc, hipStream_t stream) {
  if (!A || !Wimg || !C) return QVIT_ENULL;
  if (!b3_sizes_ok(N, K, planes) || (terms != 6 && terms != 3) || (terms == 6) != (planes == 3)) return QVIT_EINVAL;
  if (epilogue != QVIT_EPI_F32 && epilogue != QVIT_EPI_F32_RESID && epilogue != QVIT_EPI_F32_GELU) return QVIT_EINVAL;
  if (M < 0 || M > FW_MAX_EXTENT || tiles128(M, N) > FW_MAX_EXTENT || lda < K || ldc < N ||
      image_bytes < b3_bytes(N, K, planes))
    return QVIT_EINVAL;
  if ((lda % 4) || (ldc % 4) || qvit_misaligned(15, A, Wimg, C) || qvit_misaligned(3, bias)) return QVIT_EALIGN;
  if (M == 0) return QVIT_OK;
  const int8_t* img = reinterpret_cast<const int8_t*>(Wimg);
  if (terms == 6) return launch_epi<6>(epilogue, A, M, K, lda, img, N, bias, C, ldc, stream);
  return launch_epi<3>(epilogue, A, M, K, lda, img, N, bias, C, ldc, stream);
}
