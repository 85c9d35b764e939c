// Weight gradient of QuantizeLinear on the integer path: the backward of quant_layers.py:499's F.linear with
// respect to the quantized weight,
//   dW[n][k] = sum_m G[m][n] x_q[m][k] = d_act * sum_m G[m][n] A[m][k],   G fp32 (the output's gradient),
// A the int8 activation codes the forward contracted (qvit_quantize_act_i8; x_q = d_act A).
// Arithmetic (bf16x3.h): G = g1 + g2 + g3 with g1 = G truncated to bf16, g2 = (G - g1) truncated,
// g3 = G - g1 - g2 (each difference exact in fp32, g3 has at most 8 significant bits: a bf16 exactly); a code
// has at most 7 significant bits, so every product g_i A is exact in fp32 and the three passes of
// v_mfma_f32_16x16x32_bf16 sum G A with fp32 accumulation: an fp32 GEMM of G^T and A, the order of the m-term
// sum aside. One multiply by d_act follows. A NaN / inf in G[m][n] makes g2 (or g1) NaN, and NaN times any code
// (zero included) is NaN: row n of dW is NaN, no other row is touched (MFMA rows are independent).
//
// Geometry: one workgroup (4 waves, 2 x 2) per 128 (n) x 128 (k) output tile and M-split; wave (wn, wk) owns the
// 64 x 64 sub-tile: 4 x 4 MFMA tiles, 16 accumulators of 4 fp32. The contraction index m is the ROW index of both
// row-major operands, so both go through LDS as row-major bf16 images [32 m][128 columns] (256-B rows, 16-B chunk
// c of row r at c ^ ((r & 3) << 2 | (r >> 2) & 3)) and every MFMA operand (8 consecutive m of one column) is two
// ds_read_b64_tr_b16 of 4 rows x 16 columns; a 32-lane half reads two blocks 8 rows apart in the same columns:
// conflict-free. MFMA A = codes^T (rows k), B = G (columns n): lane (fr, fq) ends with
// acc[kt][nt][j] = P[n = 16 nt + fr][k = 16 kt + 4 fq + j], a 16-B store.
// m advances in stages of 32 through two LDS buffers (3 G planes + the codes as bf16, 32 KiB per stage): per stage a
// thread loads 2 x 8 fp32 of G and 16 codes into registers while the current stage computes (48 MFMAs per wave),
// then splits / converts and writes them to the other buffer; one barrier per stage. Rows m >= M are ZERO in both
// images (a clamped row would be summed twice); columns n >= N / k >= K are not loaded (zero) and never stored.
// Split over M: the output is small and M is huge, so the stages are dealt to `splits` workgroups per tile, each
// writing its raw fp32 partial tile to the workspace [split][npad][kpad] (npad, kpad: N, K rounded up to 128);
// split_fold_kernel (reduce_common.h) sums the partials in ascending split order and multiplies by d_act. No atomics: the same
// call gives the same bits. splits = min(16, stages, ceil(512 / tiles)): about two workgroups per CU.
// Budget per workgroup: 64 KiB LDS, 256 threads, 154 VGPRs (64 of them accumulators), no scratch: two workgroups
// per CU (2 waves per SIMD), set by the LDS (128 KiB of 160) and by __launch_bounds__.
#include "bf16x3.h"
#include "reduce_common.h"

namespace {

typedef short s4v __attribute__((ext_vector_type(4)));
typedef short s8v __attribute__((ext_vector_type(8)));

constexpr int WG_BN = 128;            // G columns (dW rows) per tile
constexpr int WG_BK = 128;            // code columns (dW columns) per tile
constexpr int WG_BM = 32;             // m per stage: one MFMA contraction
constexpr int WG_IMG = WG_BM * 256;   // one bf16 image [32][128]: 8 KiB
constexpr int WG_STAGE = 4 * WG_IMG;  // g1, g2, g3, codes
constexpr int WG_MAX_SPLITS = 16;
constexpr int WG_TARGET_WGS = 512;

// byte offset of 16-B chunk ch (8 bf16) of row r in an image: serves the row-wise writes and the transposed reads
QVIT_DEV int img_off(int r, int ch) { return 256 * r + 16 * (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))); }

QVIT_DEV s4v tr_read(const int8_t* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s4v*)(uintptr_t)(const __attribute__((address_space(3))) void*)p);
}
QVIT_DEV bf8 join(s4v a, s4v b) {
  const s8v s = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf8, s);
}

// part[sp][n][k] (n < npad, k < kpad) = sum over the split's rows m of G[m][n] A[m][k]
__global__ __launch_bounds__(256, 2) void gemm_wgrad_kernel(const float* __restrict__ G, int M, int N, int64_t ldg,
                                                            const int8_t* __restrict__ A, int K, int64_t lda,
                                                            int splits, int npad, int kpad,
                                                            float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) int8_t smem[2 * WG_STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;

  // unit = (split, n tile, k tile), k tiles fastest: XCD x (blocks x, x + 8, ...) walks a contiguous range of
  // units, so the k tiles that share one G panel share an L2
  const int nb_n = npad / WG_BN, nb_k = kpad / WG_BK;
  const int total = splits * nb_n * nb_k;
  const int per = (total + 7) >> 3;
  const int u = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (u >= total) return;  // (the whole workgroup: every lane of the others stays active for the transposed reads)
  const int tk = u % nb_k, tn = (u / nb_k) % nb_n, sp = u / (nb_k * nb_n);
  const int n0 = tn * WG_BN, k0 = tk * WG_BK;
  const int nst = (M + WG_BM - 1) / WG_BM;
  const int s0 = (int)((int64_t)sp * nst / splits), s1 = (int)((int64_t)(sp + 1) * nst / splits);

  // this thread's loads per stage: G rows gr and gr + 16, columns n0 + 8 gc .. + 7; codes row cr, columns
  // k0 + 16 cs .. + 15. Columns past N / K are not loaded (ldg >= N rounded up to 4 and lda >= K rounded up to 16
  // keep every issued load inside its row).
  const int gr = tid >> 4, gc = tid & 15;
  const int cr = tid >> 3, cs = tid & 7;
  const int gn = n0 + 8 * gc, ck = k0 + 16 * cs;
  const bool gok0 = gn < N, gok1 = gn + 4 < N, cok = ck < K;
  f4 gv[2][2];
  uint4 cv;
  auto load = [&](int st) __attribute__((always_inline)) {
    const int m0 = st * WG_BM;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int m = m0 + gr + 16 * h;
      const float* src = G + (int64_t)m * ldg + gn;
      gv[h][0] = (m < M && gok0) ? *reinterpret_cast<const f4*>(src) : f4{0.f, 0.f, 0.f, 0.f};
      gv[h][1] = (m < M && gok1) ? *reinterpret_cast<const f4*>(src + 4) : f4{0.f, 0.f, 0.f, 0.f};
    }
    const int m = m0 + cr;
    cv = (m < M && cok) ? *reinterpret_cast<const uint4*>(A + (int64_t)m * lda + ck) : make_uint4(0, 0, 0, 0);
  };
  auto store = [&](int b) __attribute__((always_inline)) {
    int8_t* base = smem + b * WG_STAGE;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint32_t p1[4], p2[4], p3[4];
#pragma unroll
      for (int e = 0; e < 8; e += 2)
        split_bf16x3(gv[h][e >> 2][e & 3], gv[h][(e + 1) >> 2][(e + 1) & 3], p1[e >> 1], p2[e >> 1], p3[e >> 1]);
      int8_t* d = base + img_off(gr + 16 * h, gc);
      *reinterpret_cast<uint4*>(d) = make_uint4(p1[0], p1[1], p1[2], p1[3]);
      *reinterpret_cast<uint4*>(d + WG_IMG) = make_uint4(p2[0], p2[1], p2[2], p2[3]);
      *reinterpret_cast<uint4*>(d + 2 * WG_IMG) = make_uint4(p3[0], p3[1], p3[2], p3[3]);
    }
    uint32_t c[8];
    bytes_bf16(cv.x, c[0], c[1]);
    bytes_bf16(cv.y, c[2], c[3]);
    bytes_bf16(cv.z, c[4], c[5]);
    bytes_bf16(cv.w, c[6], c[7]);
    *reinterpret_cast<uint4*>(base + 3 * WG_IMG + img_off(cr, 2 * cs)) = make_uint4(c[0], c[1], c[2], c[3]);
    *reinterpret_cast<uint4*>(base + 3 * WG_IMG + img_off(cr, 2 * cs + 1)) = make_uint4(c[4], c[5], c[6], c[7]);
  };

  // transposed-read addresses: lane 4 q + p of a 16-lane group supplies row r0 + q, columns 4 p .. 4 p + 3 of the
  // block and receives column fr of rows r0 .. r0 + 3; r0 = 8 fq + 4 h gives the operand's m = 8 fq + j
  int goff[2][4], coff[2][4];
  {
    const int q = fr >> 2, p = fr & 3;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int r = 8 * fq + 4 * h + q;
        goff[h][t] = img_off(r, 2 * (4 * wn + t) + (p >> 1)) + 8 * (p & 1);
        coff[h][t] = 3 * WG_IMG + img_off(r, 2 * (4 * wk + t) + (p >> 1)) + 8 * (p & 1);
      }
  }

  f4 acc[4][4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[kt][nt] = f4{0.f, 0.f, 0.f, 0.f};

  if (s0 < s1) {
    load(s0);
    store(0);
  }
  __syncthreads();
  for (int st = s0; st < s1; ++st) {
    const int cur = (st - s0) & 1;
    if (st + 1 < s1) load(st + 1);  // lands while this stage computes
    const int8_t* base = smem + cur * WG_STAGE;
    bf8 cf[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) cf[kt] = join(tr_read(base + coff[0][kt]), tr_read(base + coff[1][kt]));
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const bf8 gf = join(tr_read(base + p * WG_IMG + goff[0][nt]), tr_read(base + p * WG_IMG + goff[1][nt]));
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          acc[kt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cf[kt], gf, acc[kt][nt], 0, 0, 0);
      }
    if (st + 1 < s1) store(cur ^ 1);  // the other buffer: its last reader finished a barrier ago
    __syncthreads();
  }

  // the whole tile, padding rows and columns included (zeros or never read): the reduction reads n < N, k < K
  float* pb = part + ((int64_t)sp * npad + n0 + 64 * wn + fr) * kpad + k0 + 64 * wk + 4 * fq;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) *reinterpret_cast<f4*>(pb + (int64_t)16 * nt * kpad + 16 * kt) = acc[kt][nt];
}

int64_t round128(int64_t v) { return (v + 127) / 128 * 128; }

bool wgrad_sizes_ok(int64_t M, int64_t N, int64_t K) {
  return M >= 0 && N >= 1 && K >= 1 && M <= INT32_MAX / 2 && N <= (1 << 24) && K <= (1 << 24) &&
         (round128(N) / WG_BN) * (round128(K) / WG_BK) <= (1 << 24);  // (grids and split * tile counts fit int32)
}

int64_t wgrad_splits(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = (round128(N) / WG_BN) * (round128(K) / WG_BK);
  const int64_t nst = (M + WG_BM - 1) / WG_BM;
  return split_count(tiles, nst, WG_MAX_SPLITS, WG_TARGET_WGS);
}

}  // namespace

extern "C" int64_t qvit_gemm_wgrad_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  if (!wgrad_sizes_ok(M, N, K)) return QVIT_EINVAL;
  return wgrad_splits(M, N, K) * round128(N) * round128(K) * 4;
}

extern "C" int qvit_gemm_wgrad(const float* G, int64_t M, int64_t N, int64_t ldg, const int8_t* A, int64_t K,
                               int64_t lda, const float* d_act, float* dW, int64_t ldw, void* workspace,
                               int64_t workspace_bytes, hipStream_t stream) {
  if (!G || !A || !d_act || !dW || !workspace) return QVIT_ENULL;
  if (!wgrad_sizes_ok(M, N, K) || ldg < N || lda < K || ldw < K) return QVIT_EINVAL;
  if ((ldg % 4) || (lda % 16) || qvit_misaligned(15, G, A, workspace) || qvit_misaligned(3, dW)) return QVIT_EALIGN;
  if (workspace_bytes < qvit_gemm_wgrad_workspace_bytes(M, N, K)) return QVIT_EINVAL;
  const int64_t npad = round128(N), kpad = round128(K);
  const int64_t splits = M == 0 ? 0 : wgrad_splits(M, N, K);
  float* part = reinterpret_cast<float*>(workspace);
  if (splits > 0) {
    const int64_t total = splits * (npad / WG_BN) * (kpad / WG_BK);
    const unsigned grid = (unsigned)((total + 7) / 8 * 8);
    hipLaunchKernelGGL(gemm_wgrad_kernel, dim3(grid), dim3(256), 0, stream, G, (int)M, (int)N, ldg, A, (int)K, lda,
                       (int)splits, (int)npad, (int)kpad, part);
  }
  const unsigned rg = (unsigned)((N * K + 255) / 256);
  hipLaunchKernelGGL((split_fold_kernel<const float* __restrict__, int64_t>), dim3(rg), dim3(256), 0, stream, part,
                     (int)splits, (int)N, (int)K, (int)npad, (int)kpad, d_act, dW, ldw);
  return qvit_launch_status();
}
