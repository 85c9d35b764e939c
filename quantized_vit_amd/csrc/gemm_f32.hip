// fp32 x fp32 GEMM at fp32-GEMM accuracy on bf16 MFMA: the contractions of QuantizeLinear (quant_layers.py:495-499,
// F.linear on the fake-quantized operands, and what autograd runs behind it) where neither operand is an integer
// code image: weight levels beyond every packed format (the reference's driver starts at num_bits = 32,
// train.py:247-250), fake-quantized fp32 activations beyond int8, and the weight-only mode's fp32 input.
//   NT  C[m][n] = sum_k A[m][k] B[n][k] (+ bias[n])   forward (A = x_q, B = w_q) and dgrad (A = G, B = w_q^T)
//   TN  C[i][j] = sum_m A[m][i] B[m][j]               wgrad (A = G, B = x_q)
// Arithmetic (bf16x3.h): a = a1 + a2 + a3 and b = b1 + b2 + b3 exactly, each term a bf16 (8 significant bits), so
// every product a_p b_q is exact in fp32. Six of the nine go through v_mfma_f32_16x16x32_bf16 into ONE fp32
// accumulator, per 32-deep stage in the fixed order a3b1, a1b3, a2b2, a2b1, a1b2, a1b1 (smallest first); the three
// dropped ones (a2b3, a3b2, a3b3) are below (2^-21 + 2^-30) |a||b| by the truncation widths. The same call gives
// the same bits: no atomics, a fixed stage order, partials folded in ascending split order.
// Special values: x - trunc(x) of Inf is NaN, so a NaN or Inf element makes every output that contracts it NaN
// (NaN times any finite term, zero included, is NaN) and touches no other output: MFMA rows and columns are
// independent, and the zeros that pad a tile stand in rows / columns that are never stored.
//
// Geometry, both forms: one workgroup (4 waves, 2 x 2) per 128 x 128 output tile; a wave owns 64 x 64: 4 x 4 MFMA
// tiles, 64 accumulator registers. The contraction advances in stages of 32: a thread loads its 2 x 4 float4 of
// the next stage into registers while the current one computes (96 MFMAs per wave against 24 fragment reads: the
// fragments of one operand, 12, are held for the stage, the other's are read tile by tile), splits them into the
// three bf16 planes per operand and writes them to the ONE 48 KiB stage buffer (6 planes of 128 x 32 bf16) once
// its readers are done: two barriers per stage, covered by the other workgroups of the CU.
//   NT planes are [128 rows][32 k], 64-byte rows, 16-byte chunk c of row r at c ^ ((r >> 2) & 3): a fragment is one
//   ds_read_b128 (row fr, chunk fq), and the 16 lanes of one fq cover the 64 banks once. Rows past M / N are
//   clamped to the last valid row (never stored); the K tail is zero-filled element by element.
//   TN planes are gemm_wgrad.hip's [32 m][128 columns] images with its chunk swizzle, read with ds_read_b64_tr_b16.
//   Rows m >= M are zero in both images; columns past the extent are not loaded (whole float4 groups: the last
//   group of a row may reach up to 3 floats into the row's padding, whose products land in columns never read).
//   The M range is split as in gemm_wgrad.hip over s workgroups per tile, each writing its raw partial tile to
//   the workspace [s][ipad][jpad]; split_fold_kernel sums them in ascending order. Every element the fold reads
//   is written by the first launch: the workspace's contents do not matter.
// Tiles are dealt to the eight XCDs in contiguous ranges (n tiles fastest: the tiles that share an A panel share an
// L2). Index arithmetic: rows and columns in int32 (extents <= 2^24, K and M <= 2^30), element offsets in int64.
#include "gemm_f32_common.h"
#include "reduce_common.h"

namespace {

typedef short s4v __attribute__((ext_vector_type(4)));
typedef short s8v __attribute__((ext_vector_type(8)));

constexpr int FG_STAGE = 6 * FG_PLANE;   // a1 a2 a3 b1 b2 b3
constexpr int FG_MAX_SPLITS = 16;
constexpr int FG_TARGET_WGS = 512;

// ---- NT (nt_off: gemm_f32_common.h) ----------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void gemm_f32_nt_kernel(const float* __restrict__ A, int M, int K, int64_t lda,
                                                             const float* __restrict__ B, int N, int64_t ldb,
                                                             const float* __restrict__ bias, float* __restrict__ C,
                                                             int64_t ldc, int nb_n, int total) {
  __shared__ __attribute__((aligned(16))) int8_t smem[FG_STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int u = xcd_unit(total);
  if (u >= total) return;
  const int m0 = (u / nb_n) * FG_BT, n0 = (u % nb_n) * FG_BT;

  // this thread's loads per stage and operand: rows lr + 32 j (clamped), k = 4 lq .. 4 lq + 3 of the stage
  const int lr = tid >> 3, lq = tid & 7;
  const float* arow[4];
  const float* brow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    arow[j] = A + (int64_t)min(m0 + lr + 32 * j, M - 1) * lda + 4 * lq;
    brow[j] = B + (int64_t)min(n0 + lr + 32 * j, N - 1) * ldb + 4 * lq;
  }
  f4 av[4], bv[4];
  auto load = [&](int st) __attribute__((always_inline)) {
    const int kk = st * FG_BK + 4 * lq;   // kk < K and lda, ldb >= K rounded up to 4: the float4 stays in its row
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      av[j] = kk < K ? *reinterpret_cast<const f4*>(arow[j] + st * FG_BK) : f4{0.f, 0.f, 0.f, 0.f};
      bv[j] = kk < K ? *reinterpret_cast<const f4*>(brow[j] + st * FG_BK) : f4{0.f, 0.f, 0.f, 0.f};
    }
    if (st * FG_BK + FG_BK > K) {   // the ragged last stage (uniform): what lies past K may be anything
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 1; e < 4; ++e)
          if (kk + e >= K) av[j][e] = 0.f, bv[j][e] = 0.f;
    }
  };
  int8_t* const wr = smem + nt_off(lr, lq >> 1) + 8 * (lq & 1);   // row lr + 32 j: + 2048 j (the swizzle repeats)
  auto stash = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint2 p1, p2, p3;
      split4(av[j], p1, p2, p3);
      *reinterpret_cast<uint2*>(wr + 2048 * j) = p1;
      *reinterpret_cast<uint2*>(wr + 2048 * j + FG_PLANE) = p2;
      *reinterpret_cast<uint2*>(wr + 2048 * j + 2 * FG_PLANE) = p3;
      split4(bv[j], p1, p2, p3);
      *reinterpret_cast<uint2*>(wr + 2048 * j + 3 * FG_PLANE) = p1;
      *reinterpret_cast<uint2*>(wr + 2048 * j + 4 * FG_PLANE) = p2;
      *reinterpret_cast<uint2*>(wr + 2048 * j + 5 * FG_PLANE) = p3;
    }
  };
  // fragments: row 16 t + fr of the wave's 64, k = 8 fq .. 8 fq + 7 (tile t: + 1024)
  const int8_t* const afrag = smem + nt_off(64 * wm + fr, fq);
  const int8_t* const bfrag = smem + 3 * FG_PLANE + nt_off(64 * wn + fr, fq);

  f4 acc[4][4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};

  const int nst = (K + FG_BK - 1) / FG_BK;
  load(0);
  for (int st = 0; st < nst; ++st) {
    stash();
    __syncthreads();
    if (st + 1 < nst) load(st + 1);   // lands while this stage computes
    bf8 bf[4][3];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int p = 0; p < 3; ++p) bf[nt][p] = *reinterpret_cast<const bf8*>(bfrag + p * FG_PLANE + 1024 * nt);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      bf8 af[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) af[p] = *reinterpret_cast<const bf8*>(afrag + p * FG_PLANE + 1024 * mt);
      // MFMA rows = B's rows n, columns = A's rows m: lane (fr, fq) holds C[m = 16 mt + fr][n = 16 nt + 4 fq + e]
      mma6(acc[mt], bf, af);
    }
    __syncthreads();   // the buffer's readers are done: the next stage may overwrite it
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
        *reinterpret_cast<f4*>(dst) = v;
      } else {
        for (int e = 0; e < N - n; ++e) dst[e] = v[e] + (bias ? bias[n + e] : 0.f);
      }
    }
  }
}

// ---- TN ------------------------------------------------------------------------------------------------------
// byte offset of 16-B chunk ch (8 bf16) of row r in a [32][128] image (gemm_wgrad.hip's)
QVIT_DEV int tn_off(int r, int ch) { return 256 * r + 16 * (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))); }

QVIT_DEV s4v tr_read(const int8_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s4v*)(uintptr_t)(const __attribute__((address_space(3))) void*)p);
}
QVIT_DEV bf8 join(s4v a, s4v b) {
  const s8v s = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf8, s);
}

// part[sp][i][j] (i < ipad, j < jpad) = sum over the split's rows m of A[m][i] B[m][j]
__global__ __launch_bounds__(256, 2) void gemm_f32_tn_kernel(const float* __restrict__ A, int M, int I, int64_t lda,
                                                             const float* __restrict__ B, int J, int64_t ldb,
                                                             int splits, int ipad, int jpad,
                                                             float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) int8_t smem[FG_STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int nb_i = ipad / FG_BT, nb_j = jpad / FG_BT;
  const int total = splits * nb_i * nb_j;
  const int u = xcd_unit(total);
  if (u >= total) return;  // (the whole workgroup: every lane of the others stays active for the transposed reads)
  const int tj = u % nb_j, ti = (u / nb_j) % nb_i, sp = u / (nb_j * nb_i);
  const int i0 = ti * FG_BT, j0 = tj * FG_BT;
  const int nst = (M + FG_BK - 1) / FG_BK;
  const int s0 = (int)((int64_t)sp * nst / splits), s1 = (int)((int64_t)(sp + 1) * nst / splits);

  // this thread's loads per stage and operand: rows gr and gr + 16, columns 8 gc .. 8 gc + 7 of the tile
  const int gr = tid >> 4, gc = tid & 15;
  const int ai = i0 + 8 * gc, bj = j0 + 8 * gc;
  const bool aok0 = ai < I, aok1 = ai + 4 < I, bok0 = bj < J, bok1 = bj + 4 < J;
  f4 av[2][2], bv[2][2];
  auto load = [&](int st) __attribute__((always_inline)) {
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int m = st * FG_BK + gr + 16 * h;
      const float* pa = A + (int64_t)m * lda + ai;
      const float* pb = B + (int64_t)m * ldb + bj;
      av[h][0] = (m < M && aok0) ? *reinterpret_cast<const f4*>(pa) : zero;
      av[h][1] = (m < M && aok1) ? *reinterpret_cast<const f4*>(pa + 4) : zero;
      bv[h][0] = (m < M && bok0) ? *reinterpret_cast<const f4*>(pb) : zero;
      bv[h][1] = (m < M && bok1) ? *reinterpret_cast<const f4*>(pb + 4) : zero;
    }
  };
  auto stash = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int8_t* d = smem + tn_off(gr + 16 * h, gc);
      uint2 l1, l2, l3, h1, h2, h3;
      split4(av[h][0], l1, l2, l3);
      split4(av[h][1], h1, h2, h3);
      *reinterpret_cast<uint4*>(d) = make_uint4(l1.x, l1.y, h1.x, h1.y);
      *reinterpret_cast<uint4*>(d + FG_PLANE) = make_uint4(l2.x, l2.y, h2.x, h2.y);
      *reinterpret_cast<uint4*>(d + 2 * FG_PLANE) = make_uint4(l3.x, l3.y, h3.x, h3.y);
      split4(bv[h][0], l1, l2, l3);
      split4(bv[h][1], h1, h2, h3);
      *reinterpret_cast<uint4*>(d + 3 * FG_PLANE) = make_uint4(l1.x, l1.y, h1.x, h1.y);
      *reinterpret_cast<uint4*>(d + 4 * FG_PLANE) = make_uint4(l2.x, l2.y, h2.x, h2.y);
      *reinterpret_cast<uint4*>(d + 5 * FG_PLANE) = make_uint4(l3.x, l3.y, h3.x, h3.y);
    }
  };

  // transposed-read addresses: lane 4 q + p of a 16-lane group supplies row r0 + q, columns 4 p .. 4 p + 3 of the
  // block and receives column fr of rows r0 .. r0 + 3; r0 = 8 fq + 4 h gives the operand's m = 8 fq + e
  int aoff[2][4], boff[2][4];
  {
    const int q = fr >> 2, p = fr & 3;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int r = 8 * fq + 4 * h + q;
        aoff[h][t] = tn_off(r, 2 * (4 * wi + t) + (p >> 1)) + 8 * (p & 1);
        boff[h][t] = 3 * FG_PLANE + tn_off(r, 2 * (4 * wj + t) + (p >> 1)) + 8 * (p & 1);
      }
  }

  f4 acc[4][4];
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) acc[it][jt] = f4{0.f, 0.f, 0.f, 0.f};

  if (s0 < s1) load(s0);
  for (int st = s0; st < s1; ++st) {
    stash();
    __syncthreads();
    if (st + 1 < s1) load(st + 1);   // lands while this stage computes
    bf8 bf[4][3];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        bf[jt][p] = join(tr_read(smem + p * FG_PLANE + boff[0][jt]), tr_read(smem + p * FG_PLANE + boff[1][jt]));
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      bf8 af[3];
#pragma unroll
      for (int p = 0; p < 3; ++p)
        af[p] = join(tr_read(smem + p * FG_PLANE + aoff[0][it]), tr_read(smem + p * FG_PLANE + aoff[1][it]));
      // MFMA rows = B's columns j, columns = A's columns i: lane (fr, fq) holds C[i = 16 it + fr][j = 16 jt + 4 fq + e]
      mma6(acc[it], bf, af);
    }
    __syncthreads();   // the buffer's readers are done: the next stage may overwrite it
  }

  // the whole tile, padding rows and columns included (zeros or never read): the fold reads i < I, j < J
  float* pb = part + ((int64_t)sp * ipad + i0 + 64 * wi + fr) * jpad + j0 + 64 * wj + 4 * fq;
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) *reinterpret_cast<f4*>(pb + (int64_t)16 * it * jpad + 16 * jt) = acc[it][jt];
}

// rows x cols: the output; depth: the contraction. (Grids and split * tile counts fit int32.)
bool f32_sizes_ok(int64_t depth, int64_t rows, int64_t cols, int64_t min_rows) {
  return depth >= 0 && depth <= (1 << 30) && rows >= min_rows && cols >= 1 && rows <= (1 << 24) &&
         cols <= (1 << 24) && tiles128(rows, cols) <= (1 << 24);
}

int64_t tn_splits(int64_t M, int64_t I, int64_t J) {
  return split_count(tiles128(I, J), (M + FG_BK - 1) / FG_BK, FG_MAX_SPLITS, FG_TARGET_WGS);
}

}  // namespace

extern "C" int qvit_gemm_f32_nt(const float* A, int64_t M, int64_t K, int64_t lda, const float* B, int64_t N,
                                int64_t ldb, const float* bias, float* C, int64_t ldc, hipStream_t stream) {
  if (!A || !B || !C) return QVIT_ENULL;
  if (!f32_sizes_ok(K, M, N, 0) || K < 1 || lda < K || ldb < K || ldc < N) return QVIT_EINVAL;
  if ((lda % 4) || (ldb % 4) || (ldc % 4) || qvit_misaligned(15, A, B, C) || qvit_misaligned(3, bias))
    return QVIT_EALIGN;
  if (M == 0) return QVIT_OK;
  const int64_t nb_n = round128(N) / FG_BT, total = tiles128(M, N);
  const unsigned grid = (unsigned)((total + 7) / 8 * 8);
  hipLaunchKernelGGL(gemm_f32_nt_kernel, dim3(grid), dim3(256), 0, stream, A, (int)M, (int)K, lda, B, (int)N, ldb,
                     bias, C, ldc, (int)nb_n, (int)total);
  return qvit_launch_status();
}

extern "C" int64_t qvit_gemm_f32_tn_workspace_bytes(int64_t M, int64_t I, int64_t J) {
  if (!f32_sizes_ok(M, I, J, 1)) return QVIT_EINVAL;
  return tn_splits(M, I, J) * round128(I) * round128(J) * 4;
}

extern "C" int qvit_gemm_f32_tn(const float* A, int64_t M, int64_t I, int64_t lda, const float* B, int64_t J,
                                int64_t ldb, float* C, int64_t ldc, void* workspace, int64_t workspace_bytes,
                                hipStream_t stream) {
  if (!A || !B || !C || !workspace) return QVIT_ENULL;
  if (!f32_sizes_ok(M, I, J, 1) || lda < I || ldb < J || ldc < J) return QVIT_EINVAL;
  if ((lda % 4) || (ldb % 4) || qvit_misaligned(15, A, B, workspace) || qvit_misaligned(3, C)) return QVIT_EALIGN;
  if (workspace_bytes < qvit_gemm_f32_tn_workspace_bytes(M, I, J)) return QVIT_EINVAL;
  const int64_t ipad = round128(I), jpad = round128(J);
  const int64_t splits = M == 0 ? 0 : tn_splits(M, I, J);
  float* part = reinterpret_cast<float*>(workspace);
  if (splits > 0) {
    const int64_t total = splits * tiles128(I, J);
    const unsigned grid = (unsigned)((total + 7) / 8 * 8);
    hipLaunchKernelGGL(gemm_f32_tn_kernel, dim3(grid), dim3(256), 0, stream, A, (int)M, (int)I, lda, B, (int)J, ldb,
                       (int)splits, (int)ipad, (int)jpad, part);
  }
  const unsigned rg = (unsigned)((I * J + 255) / 256);
  hipLaunchKernelGGL((split_fold_kernel<float, int64_t>), dim3(rg), dim3(256), 0, stream, part, (int)splits, (int)I,
                     (int)J, (int)ipad, (int)jpad, 1.0f, C, ldc);
  return qvit_launch_status();
}
