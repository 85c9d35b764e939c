// Backward of the attention core of Attention.forward (vit_model.py:133-149):
//   S = scale q k^T, P = softmax(S), O = P v;   given dO:
//   D_i = sum_c dO_ic O_ic,  dV = P^T dO,  dP = dO v^T,  dS = P o (dP - D),  dq = scale dS k,  dk = scale dS^T q
// No N x N tensor reaches global memory: S and P are recomputed per 32-row block in registers, once per owner.
//
// Three launches on one stream, no float atomics, every sum in a fixed order (a call is bitwise reproducible):
//   1. bwd_prep_kernel  (one workgroup per (image, head)): D (scaled) per query, and the head's dS bound T.
//   2. bwd_dq_kernel    (query owner; one workgroup per (image, head, group of <= 128 queries)): a first sweep
//      over the key blocks recomputes the softmax row statistics (running max / sum of the forward's S^T = K . Q^T)
//      and writes one log-sum-exp per query to the workspace; a second sweep forms dS^T per key block and
//      accumulates dq^T += K^T . dS^T.
//   3. bwd_dkv_kernel   (key owner; one workgroup per (image, head, group of <= 128 keys)): loops over query blocks
//      with S = Q . K^T (queries on MFMA rows), reads lse and D from the workspace and accumulates
//      dV^T += dO^T . P and dK^T += Q^T . dS.
// S is therefore computed three times; nothing is accumulated across workgroups.
//
// Arithmetic: as the forward (attention.hip). Every MFMA operand is split into fp16 hi/lo and multiplied as
// hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation. Powers of two keep each operand in the
// fp16 range and are undone exactly:
//   q, k, v : in_scale (|x in_scale| <= 2^14, the forward's contract)
//   dO      : g_scale  (|dO g_scale| <= 2^14; the caller derives it from max |dO|)
//   P       : the key owner multiplies P (<= 1) by 2^14, so a row of ~1/N probabilities keeps a normal fp16 lo
//   dS      : see ds_scale below.
//
// Fragment layouts (lane: fr = lane & 15, g = lane >> 4) are the forward's: the "row" operand of the first two
// products comes from a koff image (ds_read_b128), the owner's own rows sit in registers as the B operand, the
// MFMA result puts 8 values of the lane's own row (block rows 16 (e >> 2) + 4 g + (e & 3)) in each lane, and
// those, split to fp16, are the B operand of the second products, whose A operand is the transposed read
// (ds_read_b64_tr_b16) of a voff image.
#include "attn_common.h"

namespace {

using namespace qvit_attn;

constexpr int NWAVES = 4;
constexpr int TW = 2;                    // owner tiles (16 rows) per wave
constexpr int OG = NWAVES * TW * 16;     // owner rows per workgroup (128)
// head dim 80: the query owner keeps two tiles per wave; the key owner, whose two
// accumulators per tile grow to 40 registers, fits only one in 256 registers (64 keys per workgroup)
constexpr int TWQ80 = 2;
constexpr int TWK80 = 1;
constexpr int P_SHIFT = 14;              // the key owner's P operand is 2^14 P

// Workspace: [T: B H floats, padded to 4][lse: B H Np][D: B H Np], Np = N rounded up to 32 (float4 reads of a
// block's 32 rows stay inside a head's slice).
__host__ __device__ inline int64_t np_of(int64_t N) { return (N + 31) / 32 * 32; }
__host__ __device__ inline int64_t hdr_of(int64_t BH) { return (BH + 3) / 4 * 4; }

// dS scale. With x' the scaled operands, dP'_ij = sum_c dO'_ic v'_jc and D'_i = g_scale in_scale D_i, so
// |dP'_ij - D'_i| <= |dO'_i| |v'_j| + |D'_i| <= T := max_i |dO'_i| max_j |v'_j| + max_i |D'_i| (Cauchy-Schwarz;
// the maxima over the head's rows, from bwd_prep_kernel), and P_ij <= 1 up to fp32 rounding of the exponent.
// r = 2^(14 - floor(log2 T)) gives T r < 2^15, so |dS'| = |P (dP' - D') r| < 2^15 (1 + 1e-3) < 65504: inside the
// fp16 range with a factor two to spare for the rounding of T, of the MFMA sums and of P. T is at most a few
// powers of two above the typical |dP' - D'| / P, which keeps the fp16 lo half of dS' out of the subnormals.
QVIT_DEV float ds_scale(float T) {
  int e = (int)((__float_as_uint(T) >> 23) & 0xff) - 127;   // T >= 0, finite
  e = e < -64 ? -64 : (e > 64 ? 64 : e);                   // T == 0 (dO == 0): any r does
  return __uint_as_float((uint32_t)(127 + 14 - e) << 23);
}

QVIT_DEV float max8(const float (&r)[8]) {
  return fmax_nn(fmax_nn(fmax_nn(r[0], r[1]), fmax_nn(r[2], r[3])), fmax_nn(fmax_nn(r[4], r[5]), fmax_nn(r[6], r[7])));
}

// ---- 1. D and the dS bound -----------------------------------------------------------------------------
// A row is read as 4 parts of D / 4 columns (16 at head dim 64, 20 at 80: five 16-B loads, 80-B aligned), each
// part summed left to right by one lane, the 4 parts folded by the same butterfly: the order is fixed at both widths.
template <int D = HD>
__global__ __launch_bounds__(256) void bwd_prep_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                       const float* __restrict__ gout, int N, int H, int64_t ldq,
                                                       int64_t ldo, int64_t ldgo, float in_scale, float g_scale,
                                                       float* __restrict__ ws) {
  __shared__ float red[3][256];
  const int tid = threadIdx.x;
  const int bh = blockIdx.x;
  const int h = bh % H, b = bh / H;
  constexpr int PW = D / 4;  // columns per part
  const int C = H * D;
  const int64_t Np = np_of(N);
  float* Dw = ws + hdr_of((int64_t)gridDim.x) + ((int64_t)gridDim.x + bh) * Np;
  const int part = tid & 3;
  float gm = 0.f, vm = 0.f, dm = 0.f;
  for (int r0 = 0; r0 < (int)Np; r0 += 64) {
    const int row = r0 + (tid >> 2);
    float dsum = 0.f, g2 = 0.f, v2 = 0.f;
    if (row < N) {
      const int64_t R = (int64_t)b * N + row;
      const f4* gp = reinterpret_cast<const f4*>(gout + R * ldgo + h * D + PW * part);
      const f4* op = reinterpret_cast<const f4*>(out + R * ldo + h * D + PW * part);
      const f4* vp = reinterpret_cast<const f4*>(qkv + R * ldq + 2 * C + h * D + PW * part);
#pragma unroll
      for (int k = 0; k < PW / 4; ++k) {
        const f4 gv = gp[k] * g_scale, ov = op[k] * in_scale, vv = vp[k] * in_scale;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dsum = fmaf(gv[j], ov[j], dsum);
          g2 = fmaf(gv[j], gv[j], g2);
          v2 = fmaf(vv[j], vv[j], v2);
        }
      }
    }
    // the 4 parts of a row are 4 adjacent lanes: fixed-order butterfly
    dsum += __shfl_xor(dsum, 1); dsum += __shfl_xor(dsum, 2);
    g2 += __shfl_xor(g2, 1);     g2 += __shfl_xor(g2, 2);
    v2 += __shfl_xor(v2, 1);     v2 += __shfl_xor(v2, 2);
    if (part == 0 && row < (int)Np) Dw[row] = row < N ? dsum : 0.f;
    gm = fmaxf(gm, g2);
    vm = fmaxf(vm, v2);
    dm = fmaxf(dm, fabsf(dsum));
  }
  red[0][tid] = gm; red[1][tid] = vm; red[2][tid] = dm;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) red[k][tid] = fmaxf(red[k][tid], red[k][tid + s]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    float T = fmaf(sqrtf(red[0][0]), sqrtf(red[1][0]), red[2][0]);
    if (!(T <= 3.0e38f)) T = 3.0e38f;   // inf / NaN in the inputs: they reach the gradients, T stays a number
    ws[bh] = T;
  }
}

// ---- shared staging: 32 rows x 64 floats of a [rows][ld] section -> fp16 hi/lo images -----------------------
// thread -> row tid >> 3, 8-float chunk tid & 7 (as the forward's key-block staging)
struct Chunk { f4 a, b; };

QVIT_DEV Chunk load_chunk(const float* col, int64_t ld, int row, int N, int schunk) {
  Chunk c;
  if (row < N) {  // rows past N are never loaded: zeros
    const f4* s = reinterpret_cast<const f4*>(col + (int64_t)row * ld + 8 * schunk);
    c.a = s[0]; c.b = s[1];
  } else {
    c.a = c.b = f4{0.f, 0.f, 0.f, 0.f};
  }
  return c;
}

QVIT_DEV void split_chunk(const Chunk& c, float sc, h8& hi, h8& lo) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) { x[j] = c.a[j] * sc; x[4 + j] = c.b[j] * sc; }
  split8(x, hi, lo);
}

QVIT_DEV void put(int8_t* img, int off, h8 hi, h8 lo) {
  *reinterpret_cast<h8*>(img + off) = hi;
  *reinterpret_cast<h8*>(img + IMG + off) = lo;
}

// Head dim 80 (attn_common.h: 64 + 16 columns): threads 0 .. 127 also stage a block's columns 64 .. 79 (row
// tid >> 2, 4 columns each) into the section's tail image pair; 8 tid is that thread's byte offset in it.
QVIT_DEV f4 load_tail(const float* col, int64_t ld, int row, int N) {
  const int tid = threadIdx.x;
  if (row >= N) return f4{0.f, 0.f, 0.f, 0.f};
  return *reinterpret_cast<const f4*>(col + (int64_t)row * ld + 64 + 4 * (tid & 3));
}

QVIT_DEV void put_tail(int8_t* tail, f4 x, float sc) {
  h4 hi, lo;
  split4(x * sc, hi, lo);
  *reinterpret_cast<h4*>(tail + 8 * threadIdx.x) = hi;
  *reinterpret_cast<h4*>(tail + TAIL + 8 * threadIdx.x) = lo;
}

// the owner's own rows as B operands: lane holds X[row][32 c + 8 g .. + 7] * sc, and at head dim 80
// X[row][64 + 4 g .. + 3] * sc in tile i of yt
template <int D, int T>
QVIT_DEV void load_own(const float* col, int64_t ld, int row, float sc, h8 (&hi)[2], h8 (&lo)[2], TailFrag<T, D>& yt,
                       int i) {
  const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const f4* src = reinterpret_cast<const f4*>(col + (int64_t)row * ld + 32 * c + 8 * g);
    Chunk ch{src[0], src[1]};
    split_chunk(ch, sc, hi[c], lo[c]);
  }
  if constexpr (D == HD80)
    split4(*reinterpret_cast<const f4*>(col + (int64_t)row * ld + 64 + 4 * g) * sc, yt.h[i], yt.l[i]);
}

// X^T . Y^T for one block: A fragments of the 32 block rows from the koff image pair at img (hi, lo),
// B the owner's rows: res[kt][j] = sum_d X[16 kt + 4 g + j][d] Y[row of the lane][d]
// (head dim 80: d = 64 .. 79 last, one K = 16 step on the tail image pair at tail and tile i of yt)
template <int D, int T>
QVIT_DEV void rows_dot(const int8_t* img, const int8_t* tail, const int (&koffs)[2][2], const h8 (&yh)[2],
                       const h8 (&yl)[2], const TailFrag<T, D>& yt, int i, f4 (&res)[2]) {
#pragma unroll
  for (int kt = 0; kt < 2; ++kt) {
    res[kt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 2; ++c)
      res[kt] = mfma3(lds_h8(img, koffs[kt][c]), lds_h8(img + IMG, koffs[kt][c]), yh[c], yl[c], res[kt]);
    if constexpr (D == HD80) {
      const int lane = threadIdx.x & 63;
      const int off = ktoff(16 * kt + (lane & 15), lane >> 4);
      // summed from zero in an accumulator of its own and added on the VALU: the K = 16 instruction never takes
      // the K = 32 instruction's fresh result as its SrcC. Chained, the sums here were wrong and varied from run to
      // run (observed; cause not isolated, missing hazard wait states suspected: attn_common.h mfma3t)
      res[kt] = res[kt] + mfma3t(lds_h4(tail, off), lds_h4(tail + TAIL, off), yt.h[i], yt.l[i],
                                 f4{0.f, 0.f, 0.f, 0.f});
    }
  }
}

// acc^T[16 dt + 4 g + j][row of the lane] += sum over the 32 block rows of X[row'][dim] w[row'], X from the
// voff image pair at img, w (8 values of the lane's row, block rows 16 (e >> 2) + 4 g + (e & 3)) split to fp16
// (head dim 80: the fifth slice, dims 64 .. 79, from the tail image pair at tail)
template <int D>
QVIT_DEV void accum_t(const int8_t* img, const int8_t* tail, const int (&voffs)[4], const float (&w)[8],
                      f4 (&acc)[D / 16]) {
  h8 wh, wl;
  split8(w, wh, wl);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const h8 xh = join(tr_read(img, voffs[dt]), tr_read(img, voffs[dt] + 16 * 128));
    const h8 xl = join(tr_read(img + IMG, voffs[dt]), tr_read(img + IMG, voffs[dt] + 16 * 128));
    acc[dt] = mfma3(xh, xl, wh, wl, acc[dt]);
  }
  if constexpr (D == HD80) {
    const int lane = threadIdx.x & 63;
    const int off = vtoff(lane & 15, lane >> 4);
    const h8 xh = join(tr_read(tail, off), tr_read(tail, off + 16 * 32));
    const h8 xl = join(tr_read(tail + TAIL, off), tr_read(tail + TAIL, off + 16 * 32));
    acc[4] = mfma3(xh, xl, wh, wl, acc[4]);
  }
}

// ---- 2. query owner: row statistics, then dq ------------------------------------------------------------
// LDS stage (24 KiB, double-buffered): K koff hi/lo, V koff hi/lo, K voff hi/lo.
// Head dim 80: + the tail image pairs of K and V (4 KiB; K's serves the koff and the voff reads): 28 KiB.
template <int D>
constexpr int QSTAGE_OF = 6 * IMG + (D == HD80 ? 4 * TAIL : 0);

// NT: owner tiles per wave (the workgroup owns NWAVES * NT * 16 queries)
template <int D = HD, int NT = TW>
__global__ __launch_bounds__(256, 2) void bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ gout,
                                                        int N, int H, int64_t ldq, int64_t ldgo, float scale,
                                                        float in_scale, float g_scale, float* __restrict__ gqkv,
                                                        int64_t ldg, float* __restrict__ ws, int BH) {
  constexpr int QSTAGE = QSTAGE_OF<D>;
  constexpr int OGN = NWAVES * NT * 16;
  __shared__ __attribute__((aligned(16))) int8_t smem[2 * QSTAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15;
  const int g = lane >> 4;

  const int ngroups = (N + OGN - 1) / OGN;
  const int grp = blockIdx.x % ngroups;
  const int bh = blockIdx.x / ngroups;
  const int h = bh % H, b = bh / H;
  const int C = H * D;
  const int64_t Np = np_of(N);
  const float* base = qkv + (int64_t)b * N * ldq;
  const float* qcol = base + h * D;
  const float* kcol = base + C + h * D;
  const float* vcol = base + 2 * C + h * D;
  const float* gcol = gout + (int64_t)b * N * ldgo + h * D;
  float* lse_w = ws + hdr_of(BH) + (int64_t)bh * Np;
  const float* D_w = ws + hdr_of(BH) + ((int64_t)BH + bh) * Np;
  const float rr = ds_scale(ws[bh]);

  const int q0 = grp * OGN;
  h8 qh[NT][2], ql[NT][2], dh[NT][2], dl[NT][2];
  [[maybe_unused]] TailFrag<NT, D> qt, dt_;   // columns 64 .. 79 of q and dO (head dim 80)
  bool tv[NT];
  float Dq[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wave + NWAVES * i;
    tv[i] = q0 + 16 * tile < N;  // wave-uniform
    int q = q0 + 16 * tile + fr;
    q = q < N ? q : N - 1;       // padded queries read a valid row; never stored
    load_own<D>(qcol, ldq, q, in_scale, qh[i], ql[i], qt, i);
    load_own<D>(gcol, ldgo, q, g_scale, dh[i], dl[i], dt_, i);
    Dq[i] = D_w[q];
  }

  const int srow = tid >> 3, schunk = tid & 7;
  Chunk pk, pv;
  [[maybe_unused]] f4 tk, tvv;                    // head dim 80: the tails' staging (load_tail)
  [[maybe_unused]] const bool stail = tid < 128;  // wave-uniform (waves 0 and 1)
  auto load_block = [&](int kb, bool full) {
    pk = load_chunk(kcol, ldq, kb * KB + srow, N, schunk);
    if (full) pv = load_chunk(vcol, ldq, kb * KB + srow, N, schunk);
    if constexpr (D == HD80) {
      if (stail) {
        tk = load_tail(kcol, ldq, kb * KB + (tid >> 2), N);
        if (full) tvv = load_tail(vcol, ldq, kb * KB + (tid >> 2), N);
      }
    }
  };
  auto store_block = [&](int buf, bool full) {
    int8_t* st = smem + buf * QSTAGE;
    h8 hi, lo;
    split_chunk(pk, in_scale, hi, lo);
    put(st, koff(srow, schunk), hi, lo);
    if (full) {
      put(st + 4 * IMG, voff(srow, 16 * schunk), hi, lo);
      split_chunk(pv, in_scale, hi, lo);
      put(st + 2 * IMG, koff(srow, schunk), hi, lo);
    }
    if constexpr (D == HD80) {
      if (stail) {
        put_tail(st + 6 * IMG, tk, in_scale);
        if (full) put_tail(st + 6 * IMG + 2 * TAIL, tvv, in_scale);
      }
    }
  };

  int koffs[2][2], voffs[4];
  fragment_offsets(koffs, voffs);
  const float sl2 = scale * LOG2E / (in_scale * in_scale);
  const int nkb = (N + KB - 1) / KB;

  // sweep 1: running max / sum of the scaled scores (log2 units), per lane over its 8 keys of each block
  float m[NT], l[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) { m[i] = -INFINITY; l[i] = 0.f; }
  load_block(0, false);
  store_block(0, false);
  __syncthreads();
  for (int kb = 0; kb < nkb; ++kb) {
    if (kb + 1 < nkb) load_block(kb + 1, false);
    const int8_t* st = smem + (kb & 1) * QSTAGE;
    const int kbase = kb * KB + 4 * g;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      if (!tv[i]) continue;  // wave-uniform
      f4 s[2];
      rows_dot<D>(st, st + 6 * IMG, koffs, qh[i], ql[i], qt, i, s);
      float r[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = (kbase + 16 * (e >> 2) + (e & 3) < N) ? s[e >> 2][e & 3] : -INFINITY;
      const float bm = xmax(max8(r)) * sl2;   // every block has a key < N: finite
      const float mn = fmax_nn(m[i], bm);
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) ps += __builtin_amdgcn_exp2f(fmaf(r[e], sl2, -mn));
      l[i] = fmaf(l[i], __builtin_amdgcn_exp2f(m[i] - mn), ps);
      m[i] = mn;
    }
    if (kb + 1 < nkb) {
      __syncthreads();  // every wave is done with buffer (kb + 1) & 1
      store_block((kb + 1) & 1, false);
    }
    __syncthreads();
  }
  float lse[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    lse[i] = m[i] + __builtin_amdgcn_logf(xsum(l[i]));  // log2
    const int q = q0 + 16 * (wave + NWAVES * i) + fr;
    if (tv[i] && g == 0 && q < N) lse_w[q] = lse[i];
  }

  // sweep 2: dq^T += K^T . dS'^T
  f4 acc[NT][D / 16];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) acc[i][dt] = f4{0.f, 0.f, 0.f, 0.f};
  load_block(0, true);
  store_block(0, true);
  __syncthreads();
  for (int kb = 0; kb < nkb; ++kb) {
    if (kb + 1 < nkb) load_block(kb + 1, true);
    const int8_t* st = smem + (kb & 1) * QSTAGE;
    const int kbase = kb * KB + 4 * g;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      if (!tv[i]) continue;  // wave-uniform
      f4 s[2], dp[2];
      rows_dot<D>(st, st + 6 * IMG, koffs, qh[i], ql[i], qt, i, s);
      rows_dot<D>(st + 2 * IMG, st + 6 * IMG + 2 * TAIL, koffs, dh[i], dl[i], dt_, i, dp);
      float w[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool ok = kbase + 16 * (e >> 2) + (e & 3) < N;
        const float p = __builtin_amdgcn_exp2f(fmaf(s[e >> 2][e & 3], sl2, -lse[i]));
        w[e] = ok ? p * ((dp[e >> 2][e & 3] - Dq[i]) * rr) : 0.f;   // |w| < 2^15 (ds_scale)
      }
      accum_t<D>(st + 4 * IMG, st + 6 * IMG, voffs, w, acc[i]);
    }
    if (kb + 1 < nkb) {
      __syncthreads();
      store_block((kb + 1) & 1, true);
    }
    __syncthreads();
  }
  // acc = g_scale in_scale^2 r sum_j dS_ij k_j
  const float cq = scale / (g_scale * in_scale * in_scale * rr);
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int q = q0 + 16 * (wave + NWAVES * i) + fr;
    if (!tv[i] || q >= N) continue;
    float* dst = gqkv + ((int64_t)b * N + q) * ldg + h * D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) *reinterpret_cast<f4*>(dst + 16 * dt) = acc[i][dt] * cq;
  }
}

// ---- 3. key owner: dk, dv ----------------------------------------------------------------------------------
// LDS stage (32 KiB, double-buffered): Q koff hi/lo, dO koff hi/lo, Q voff hi/lo, dO voff hi/lo.
// Head dim 80: + the tail image pairs of Q and dO (4 KiB; each serves its koff and its voff reads): 36 KiB, 72 KiB
// per workgroup (a gfx950 workgroup may take up to 160 KiB), two workgroups per CU.
template <int D>
constexpr int KSTAGE_OF = 8 * IMG + (D == HD80 ? 4 * TAIL : 0);

template <int D = HD, int NT = TW>
__global__ __launch_bounds__(256, 2) void bwd_dkv_kernel(const float* __restrict__ qkv,
                                                         const float* __restrict__ gout, int N, int H, int64_t ldq,
                                                         int64_t ldgo, float scale, float in_scale, float g_scale,
                                                         float* __restrict__ gqkv, int64_t ldg,
                                                         const float* __restrict__ ws, int BH) {
  constexpr int KSTAGE = KSTAGE_OF<D>;
  constexpr int OGN = NWAVES * NT * 16;
  __shared__ __attribute__((aligned(16))) int8_t smem[2 * KSTAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15;
  const int g = lane >> 4;

  const int ngroups = (N + OGN - 1) / OGN;
  const int grp = blockIdx.x % ngroups;
  const int bh = blockIdx.x / ngroups;
  const int h = bh % H, b = bh / H;
  const int C = H * D;
  const int64_t Np = np_of(N);
  const float* base = qkv + (int64_t)b * N * ldq;
  const float* qcol = base + h * D;
  const float* kcol = base + C + h * D;
  const float* vcol = base + 2 * C + h * D;
  const float* gcol = gout + (int64_t)b * N * ldgo + h * D;
  const float* lse_w = ws + hdr_of(BH) + (int64_t)bh * Np;
  const float* D_w = ws + hdr_of(BH) + ((int64_t)BH + bh) * Np;
  const float rr = ds_scale(ws[bh]);
  const float rp = rr * (1.f / (float)(1 << P_SHIFT));   // dS' = (2^14 P) ((dP' - D') r 2^-14)

  const int k0 = grp * OGN;
  h8 kh[NT][2], kl[NT][2], vh[NT][2], vl[NT][2];
  [[maybe_unused]] TailFrag<NT, D> kt_, vt_;   // columns 64 .. 79 of k and v (head dim 80)
  bool tv[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int tile = wave + NWAVES * i;
    tv[i] = k0 + 16 * tile < N;  // wave-uniform
    int key = k0 + 16 * tile + fr;
    key = key < N ? key : N - 1;  // padded keys read a valid row; never stored
    load_own<D>(kcol, ldq, key, in_scale, kh[i], kl[i], kt_, i);
    load_own<D>(vcol, ldq, key, in_scale, vh[i], vl[i], vt_, i);
  }

  const int srow = tid >> 3, schunk = tid & 7;
  Chunk pq, pg;
  [[maybe_unused]] f4 tq, tg;                     // head dim 80: the tails' staging (load_tail)
  [[maybe_unused]] const bool stail = tid < 128;  // wave-uniform (waves 0 and 1)
  auto load_block = [&](int qb) {
    pq = load_chunk(qcol, ldq, qb * KB + srow, N, schunk);
    pg = load_chunk(gcol, ldgo, qb * KB + srow, N, schunk);
    if constexpr (D == HD80) {
      if (stail) {
        tq = load_tail(qcol, ldq, qb * KB + (tid >> 2), N);
        tg = load_tail(gcol, ldgo, qb * KB + (tid >> 2), N);
      }
    }
  };
  auto store_block = [&](int buf) {
    int8_t* st = smem + buf * KSTAGE;
    h8 hi, lo;
    split_chunk(pq, in_scale, hi, lo);
    put(st, koff(srow, schunk), hi, lo);
    put(st + 4 * IMG, voff(srow, 16 * schunk), hi, lo);
    split_chunk(pg, g_scale, hi, lo);
    put(st + 2 * IMG, koff(srow, schunk), hi, lo);
    put(st + 6 * IMG, voff(srow, 16 * schunk), hi, lo);
    if constexpr (D == HD80) {
      if (stail) {
        put_tail(st + 8 * IMG, tq, in_scale);
        put_tail(st + 8 * IMG + 2 * TAIL, tg, g_scale);
      }
    }
  };

  int koffs[2][2], voffs[4];
  fragment_offsets(koffs, voffs);
  const float sl2 = scale * LOG2E / (in_scale * in_scale);
  const int nqb = (N + KB - 1) / KB;

  f4 dk[NT][D / 16], dv[NT][D / 16];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) dk[i][dt] = dv[i][dt] = f4{0.f, 0.f, 0.f, 0.f};

  load_block(0);
  store_block(0);
  __syncthreads();
  for (int qb = 0; qb < nqb; ++qb) {
    if (qb + 1 < nqb) load_block(qb + 1);
    const int8_t* st = smem + (qb & 1) * KSTAGE;
    const int qbase = qb * KB + 4 * g;
    // the block's row statistics: queries qbase + 16 (e >> 2) + (e & 3) (inside the padded slice; entries of
    // queries >= N are selected away below)
    float nl[8], Dq[8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const f4 a = *reinterpret_cast<const f4*>(lse_w + qbase + 16 * t);
      const f4 d = *reinterpret_cast<const f4*>(D_w + qbase + 16 * t);
#pragma unroll
      for (int j = 0; j < 4; ++j) { nl[4 * t + j] = (float)P_SHIFT - a[j]; Dq[4 * t + j] = d[j]; }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      if (!tv[i]) continue;  // wave-uniform
      f4 s[2], dp[2];
      rows_dot<D>(st, st + 8 * IMG, koffs, kh[i], kl[i], kt_, i, s);
      rows_dot<D>(st + 2 * IMG, st + 8 * IMG + 2 * TAIL, koffs, vh[i], vl[i], vt_, i, dp);
      float p[8], w[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool ok = qbase + 16 * (e >> 2) + (e & 3) < N;
        const float pe = __builtin_amdgcn_exp2f(fmaf(s[e >> 2][e & 3], sl2, nl[e]));   // 2^14 P <= 2^14 (1 + 1e-3)
        p[e] = ok ? pe : 0.f;
        w[e] = ok ? pe * ((dp[e >> 2][e & 3] - Dq[e]) * rp) : 0.f;                     // |w| < 2^15 (ds_scale)
      }
      accum_t<D>(st + 6 * IMG, st + 8 * IMG + 2 * TAIL, voffs, p, dv[i]);
      accum_t<D>(st + 4 * IMG, st + 8 * IMG, voffs, w, dk[i]);
    }
    if (qb + 1 < nqb) {
      __syncthreads();
      store_block((qb + 1) & 1);
    }
    __syncthreads();
  }
  // dk acc = g_scale in_scale^2 r sum_i dS_ij q_i;  dv acc = 2^14 g_scale sum_i P_ij dO_i
  const float ck = scale / (g_scale * in_scale * in_scale * rr);
  const float cv = 1.f / (g_scale * (float)(1 << P_SHIFT));
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int key = k0 + 16 * (wave + NWAVES * i) + fr;
    if (!tv[i] || key >= N) continue;
    float* dst = gqkv + ((int64_t)b * N + key) * ldg + h * D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      *reinterpret_cast<f4*>(dst + C + 16 * dt) = dk[i][dt] * ck;
      *reinterpret_cast<f4*>(dst + 2 * C + 16 * dt) = dv[i][dt] * cv;
    }
  }
}

}  // namespace

extern "C" int64_t qvit_attention_backward_workspace_bytes(int64_t B, int64_t N, int64_t H) {
  if (B < 0 || N <= 0 || H <= 0 || N > (1 << 20) || B * H > INT32_MAX) return QVIT_EINVAL;
  return 4 * (hdr_of(B * H) + 2 * B * H * np_of(N));
}

extern "C" int qvit_attention_backward(const float* qkv, const float* out, const float* grad_out, int64_t B,
                                       int64_t N, int64_t H, int64_t head_dim, int64_t ldq, int64_t ldo,
                                       int64_t ldgo, float scale, float in_scale, float g_scale, float* grad_qkv,
                                       int64_t ldg, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  if (!qkv || !out || !grad_out || !grad_qkv) return QVIT_ENULL;
  if (head_dim != HD && head_dim != HD80) return QVIT_EINVAL;
  if (B < 0 || N <= 0 || H <= 0 || ldq < 3 * H * head_dim || ldg < 3 * H * head_dim || ldo < H * head_dim ||
      ldgo < H * head_dim)
    return QVIT_EINVAL;
  if (B * N > INT32_MAX || N > (1 << 20) || !(in_scale > 0.f) || !(g_scale > 0.f)) return QVIT_EINVAL;
  if ((ldq % 4) || (ldo % 4) || (ldgo % 4) || (ldg % 4)) return QVIT_EALIGN;
  if (qvit_misaligned(15, qkv, out, grad_out, grad_qkv)) return QVIT_EALIGN;
  if (B == 0) return QVIT_OK;
  const int64_t need = qvit_attention_backward_workspace_bytes(B, N, H);
  if (need < 0) return QVIT_EINVAL;
  if (!workspace) return QVIT_ENULL;
  if (workspace_bytes < need) return QVIT_EINVAL;
  if (qvit_misaligned(15, workspace)) return QVIT_EALIGN;
  const int64_t BH = B * H;
  const int64_t nblk = BH * ((N + OG - 1) / OG);
  if (nblk > INT32_MAX) return QVIT_EINVAL;
  float* ws = reinterpret_cast<float*>(workspace);
  if (head_dim == HD80) {
    hipLaunchKernelGGL(bwd_prep_kernel<HD80>, dim3((unsigned)BH), dim3(256), 0, stream, qkv, out, grad_out, (int)N,
                       (int)H, ldq, ldo, ldgo, in_scale, g_scale, ws);
    constexpr int OGQ = NWAVES * TWQ80 * 16, OGK = NWAVES * TWK80 * 16;
    const int64_t nblk_q = BH * ((N + OGQ - 1) / OGQ), nblk_k = BH * ((N + OGK - 1) / OGK);
    if (nblk_k > INT32_MAX) return QVIT_EINVAL;
    hipLaunchKernelGGL((bwd_dq_kernel<HD80, TWQ80>), dim3((unsigned)nblk_q), dim3(256), 0, stream, qkv, grad_out,
                       (int)N, (int)H, ldq, ldgo, scale, in_scale, g_scale, grad_qkv, ldg, ws, (int)BH);
    hipLaunchKernelGGL((bwd_dkv_kernel<HD80, TWK80>), dim3((unsigned)nblk_k), dim3(256), 0, stream, qkv, grad_out,
                       (int)N, (int)H, ldq, ldgo, scale, in_scale, g_scale, grad_qkv, ldg, ws, (int)BH);
    return qvit_launch_status();
  }
  hipLaunchKernelGGL(bwd_prep_kernel<HD>, dim3((unsigned)BH), dim3(256), 0, stream, qkv, out, grad_out, (int)N,
                     (int)H, ldq, ldo, ldgo, in_scale, g_scale, ws);
  hipLaunchKernelGGL((bwd_dq_kernel<HD, TW>), dim3((unsigned)nblk), dim3(256), 0, stream, qkv, grad_out, (int)N,
                     (int)H, ldq, ldgo, scale, in_scale, g_scale, grad_qkv, ldg, ws, (int)BH);
  hipLaunchKernelGGL((bwd_dkv_kernel<HD, TW>), dim3((unsigned)nblk), dim3(256), 0, stream, qkv, grad_out, (int)N,
                     (int)H, ldq, ldgo, scale, in_scale, g_scale, grad_qkv, ldg, ws, (int)BH);
  return qvit_launch_status();
}
