// The epilogue of the GEMMs whose lanes end up with 16 consecutive output columns of one row in registers
// (gemm_a4.hip, gemm_f6.hip): gemm_skinny.hip's epilogue arithmetic, which is qvit_gemm's, with nothing staged.
#pragma once

#include "qvit_common.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

struct Epi16Args {
  const float* d_act;
  const float* d_wt;
  const float* bias;
  int out_qtype;
  const float* out_d;
  const float* out_qm;
  const float* out_t;
  int out_levels;
  const int8_t* table;   // optional code table of the int8 epilogues (qvit_epi_table_build)
};

// the int8 epilogues' quantizer state: the table's header, or the direct quantizer's scalars
struct Epi16Quant {
  bool use_table;
  float c0, inv_w, top;
  QParams qp;
};

// the table's header if it is usable; false: the caller loads the quantizer's scalars (load_qparams) instead
QVIT_DEV Epi16Quant epi16_quant(const int8_t* table) {
  Epi16Quant q{false, 0.f, 0.f, 0.f, {}};
  if (table != nullptr) {
    const EpiTableHdr h = *reinterpret_cast<const EpiTableHdr*>(table);
    q.use_table = h.valid != 0 && h.nb >= 1 && h.nb <= QVIT_EPI_TABLE_MAX_NB;
    q.c0 = h.c0;
    q.inv_w = h.inv_w;
    q.top = epi_top(h.nb);
  }
  return q;
}

// Row m, columns nb + 4 r + j of one 16-row group: gemm_skinny.hip's epilogue arithmetic (qvit_gemm's results).
// SHIFT: the accumulators hold 2^SHIFT acc; alpha carries 2^-SHIFT.
template <int EPI, int SHIFT>
QVIT_DEV void epi16_row(const v4i (&acc)[4], int m, int nb, int N, void* __restrict__ C, int64_t ldc, float alpha,
                        const Epi16Args& ep, const Epi16Quant& q) {
  if constexpr (EPI == QVIT_EPI_I32) {
    int32_t* dst = reinterpret_cast<int32_t*>(C) + (int64_t)m * ldc + nb;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const v4i a = v4i{acc[r][0] >> SHIFT, acc[r][1] >> SHIFT, acc[r][2] >> SHIFT, acc[r][3] >> SHIFT};   // exact
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
    // int8 codes: the table's entry {thr, lo | hi << 8} of v's bucket, or the quantizer itself; the same code for
    // every v (the table is built from this very function)
    uint32_t wd[4] = {0u, 0u, 0u, 0u};
    if (q.use_table) {
      const int8_t* ent = ep.table + sizeof(EpiTableHdr);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint2 e = *reinterpret_cast<const uint2*>(ent + 8 * epi_bucket(v[i], q.c0, q.inv_w, q.top));
        const uint32_t code = (v[i] >= __uint_as_float(e.x)) ? ((e.y >> 8) & 0xffu) : (e.y & 0xffu);
        wd[i >> 2] |= code << (8 * (i & 3));
      }
    } else {
#pragma unroll 1
      for (int i = 0; i < 16; ++i) {
        const float x = (EPI == QVIT_EPI_I8_GELU) ? gelu_ref(v[i]) : v[i];
        const uint32_t code = (uint32_t)(uint8_t)to_i8_sat(quant_code(x, q.qp));
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

}  // namespace
