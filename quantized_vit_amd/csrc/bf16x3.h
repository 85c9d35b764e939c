// fp32 as three bf16 terms: the exactness argument behind qvit_gemm_wonly, qvit_conv_wonly*, qvit_gemm_wgrad and
// qvit_conv_wgrad. x = x1 + x2 + x3 with x1 = x truncated to bf16, x2 = (x - x1) truncated, x3 = x - x1 - x2; an
// int8 code (or a power of two times one) is a bf16 exactly, so every product x_i code is exact in fp32 and three
// passes of v_mfma_f32_16x16x32_bf16 sum x code with fp32 accumulation.
#pragma once
#include "qvit_common.h"

namespace {

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));

QVIT_DEV bf8 as_bf8(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return __builtin_bit_cast(bf8, make_uint4(a, b, c, d));
}

QVIT_DEV float trunc_bf16(float x) { return __uint_as_float(__float_as_uint(x) & 0xFFFF0000u); }
QVIT_DEV uint32_t hi16(float a, float b) {  // bf16 bits of a (low half) and b (high half); both exact bf16 values
  return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xFFFF0000u);
}
// four signed bytes -> four bf16 of mul * byte, exact (mul a power of two)
QVIT_DEV void bytes_bf16(uint32_t d, uint32_t& lo, uint32_t& hi, float mul = 1.f) {
  const uint32_t u = d ^ 0x80808080u;  // unsigned byte = signed + 128
  const float f0 = ((float)(u & 0xff) - 128.f) * mul, f1 = ((float)((u >> 8) & 0xff) - 128.f) * mul;
  const float f2 = ((float)((u >> 16) & 0xff) - 128.f) * mul, f3 = ((float)(u >> 24) - 128.f) * mul;
  lo = hi16(f0, f1);
  hi = hi16(f2, f3);
}

// the pair (a, c) as one packed word per term: p_i = {a_i (low half), c_i (high half)}
QVIT_DEV void split_bf16x3(float a, float c, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
  const float a1 = trunc_bf16(a), c1 = trunc_bf16(c);
  const float ar = a - a1, cr = c - c1;      // exact
  const float a2 = trunc_bf16(ar), c2 = trunc_bf16(cr);
  const float a3 = ar - a2, c3 = cr - c2;    // exact, <= 8 significant bits
  p1 = hi16(a1, c1);
  p2 = hi16(a2, c2);
  p3 = hi16(a3, c3);
}

}  // namespace
