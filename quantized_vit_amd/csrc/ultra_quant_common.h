// Device code of UltraNet's weight quantizer (reference `4-bit quantization/quant_ultra.py:50-55`) shared by its
// forward (ultra_conv.hip: qvit_ultra_weight_codes) and its backward (ultra_backward.hip:
// qvit_ultra_weight_quant_backward): t = tanh(w) and m = max|t|. Both passes call these routines, so the backward
// sees the very t and m, and with them the set of elements attaining the maximum, that the forward saw.
#pragma once
#include "qvit_common.h"

namespace {

QVIT_DEV float ultra_tanh(float w) { return tanhf(w); }
QVIT_DEV float ultra_absmax(float m, float t) { return fmaxf(m, fabsf(t)); }  // (a NaN t is skipped)

// *maxbits (zeroed by the caller) = the bits of max|tanh(w)|; m >= 0, so the bit order is the value order and the
// integer atomic gives the same result in any arrival order
__global__ void ultra_wmax_kernel(const float* __restrict__ w, int64_t n, unsigned* __restrict__ maxbits) {
  float m = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    m = ultra_absmax(m, ultra_tanh(w[i]));
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) atomicMax(maxbits, __float_as_uint(m));
}

}  // namespace
