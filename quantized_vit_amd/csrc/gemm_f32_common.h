// What gemm_f32.hip (both operands split per stage) and gemm_f32w.hip (the weight operand pre-split into an image)
// share: the stage geometry, the swizzled [128][32] bf16 plane, the XCD tile deal and the MFMA rounds.
#pragma once
#include "bf16x3.h"

namespace {

constexpr int FG_BT = 128;               // tile side (both output axes)
constexpr int FG_BK = 32;                // contraction per stage: one MFMA
constexpr int FG_PLANE = FG_BT * FG_BK * 2;   // one bf16 plane: 8 KiB

// One round: the four MFMA tiles of an accumulator row take the product of planes pa (columns) and pb (rows).
#define FG_ROUND(pa, pb)                                                                      \
  _Pragma("unroll") for (int t = 0; t < 4; ++t) acc[t] =                                      \
      __builtin_amdgcn_mfma_f32_16x16x32_bf16(r[t][pb], c[pa], acc[t], 0, 0, 0);

// The six products of the four MFMA tiles of one accumulator row, smallest first: a3b1, a1b3, a2b2, a2b1, a1b2, a1b1
// (each accumulator sees them in that order; the four tiles of a round are independent). r: the planes b1 b2 b3 of
// the operand that supplies the MFMAs' rows, per tile; c: the planes a1 a2 a3 of the one that supplies their columns.
QVIT_DEV void mma6(f4 (&acc)[4], const bf8 (&r)[4][3], const bf8 (&c)[3]) {
  FG_ROUND(2, 0) FG_ROUND(0, 2) FG_ROUND(1, 1) FG_ROUND(1, 0) FG_ROUND(0, 1) FG_ROUND(0, 0)
}
// The three largest of them, same order: a2b1, a1b2, a1b1 (two planes per operand)
QVIT_DEV void mma3(f4 (&acc)[4], const bf8 (&r)[4][2], const bf8 (&c)[2]) {
  FG_ROUND(1, 0) FG_ROUND(0, 1) FG_ROUND(0, 0)
}
#undef FG_ROUND

// this workgroup's unit under the XCD deal: XCD x (blocks x, x + 8, ...) walks a contiguous range of units
QVIT_DEV int xcd_unit(int total) {
  const int per = (total + 7) >> 3;
  return (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
}

QVIT_DEV void split4(f4 v, uint2& p1, uint2& p2, uint2& p3) {
  split_bf16x3(v[0], v[1], p1.x, p2.x, p3.x);
  split_bf16x3(v[2], v[3], p1.y, p2.y, p3.y);
}

// byte offset of 16-B chunk ch (8 bf16) of row r in a [128][32] plane: 64-byte rows, chunk c at c ^ ((r >> 2) & 3)
QVIT_DEV int nt_off(int r, int ch) { return 64 * r + 16 * (ch ^ ((r >> 2) & 3)); }

inline int64_t round128(int64_t v) { return (v + 127) / 128 * 128; }
inline int64_t tiles128(int64_t r, int64_t c) { return (round128(r) / FG_BT) * (round128(c) / FG_BT); }

}  // namespace
