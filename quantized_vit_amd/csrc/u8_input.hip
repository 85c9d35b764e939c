// uint8 image input of libqvit_hip.so (gfx950): the host-side ToTensor + Normalize and the activation quantizer
// of the first convolution folded into per-channel tables of 256 entries, looked up from LDS.
//
//   qvit_im2col_u8_i8     : codes[(b, oh, ow)][c kh kw + ih kw + iw] = T[c][img(b, c, y, x)], 0 for a tap outside the
//                           image and in columns [K, kpad): the rows qvit_im2col_quant_i8 writes from the fp32 image
//                           V[c][img], when T = quantize(V) (the caller builds T with qvit_quantize_act_i8).
//   qvit_u8_normalize_f32 : out[b][c][y][x] = V[c][img(b, c, y, x)], fp32 NCHW.
//
// img(b, c, y, x) is byte ((b C + c) H + y) W + x of an NCHW image and ((b H + y) W + x) C + c of an NHWC one.
//
// Every workgroup copies the table into LDS once (C * 256 bytes of codes, C * 1024 bytes of values; C <= 16) and then
// walks its work items in a grid-stride loop. The lookups are byte (codes) or dword (values) LDS reads at
// data-dependent addresses: one per image byte, the only work besides the loads and stores.
//
// Arms of the im2col kernel, identical bytes where more than one applies (the host picks):
//   kNchw16 : kw % 16 == 0, dw == 1, ph == pw == 0, W % 16 == 0, sw % 16 == 0, a 16-byte aligned image: a 16-column
//             chunk is 16 consecutive bytes of one image row: one 16-byte load, 16 lookups, one 16-byte store.
//   kNhwc3  : the same conditions on an NHWC image with C == 3: one work item is the 16 pixels (ih, iw0 .. iw0 + 15)
//             of a patch, 48 consecutive bytes: three 16-byte loads, 48 lookups, three 16-byte stores, one into each
//             channel's chunk. The chunks of the padding columns [K, kpad) are further work items that store zeros.
//   kScalar : everything else, either layout: a bounds-checked gather per element.
// On the two 16-byte arms no bounds check is needed: with ph == pw == 0 the output size gives
// y = oh sh + ih dh <= (OH - 1) sh + (kh - 1) dh < H, and x0 = ow sw + iw0 is a multiple of 16 below W, W % 16 == 0,
// so x0 + 16 <= W.
// I is the index type of the element arithmetic, as in im2col_quant_kernel (quant_kernels.hip).
#include "qvit_common.h"
#include "reduce_common.h"

namespace {

constexpr int kMaxC = 16;           // channels whose tables fit the LDS arrays below
enum U8Arm { kScalar = 0, kNchw16 = 1, kNhwc3 = 2 };

// `bytes` (a multiple of 4) from global to LDS by the whole workgroup; dwords when the source allows
QVIT_DEV void stage_table(const void* __restrict__ src, void* lds, int bytes) {
  if ((((uintptr_t)src) & 3) == 0) {
    const uint32_t* s = static_cast<const uint32_t*>(src);
    uint32_t* d = static_cast<uint32_t*>(lds);
    for (int i = threadIdx.x; i < bytes / 4; i += blockDim.x) d[i] = s[i];
  } else {
    const uint8_t* s = static_cast<const uint8_t*>(src);
    uint8_t* d = static_cast<uint8_t*>(lds);
    for (int i = threadIdx.x; i < bytes; i += blockDim.x) d[i] = s[i];
  }
  __syncthreads();
}

QVIT_DEV uint32_t byte_of(const uint32_t* w, int n) { return (w[n >> 2] >> (8 * (n & 3))) & 0xffu; }

template <typename I, int ARM>
__global__ __launch_bounds__(kThreads) void im2col_u8_kernel(
    const uint8_t* __restrict__ img, int64_t B_, int64_t C_, int64_t H_, int64_t W_, int nhwc, int kh, int kw, int sh,
    int sw, int ph, int pw, int dh, int dw, int64_t OH_, int64_t OW_, const int8_t* __restrict__ code_table,
    int8_t* __restrict__ codes, int64_t ldc_, int64_t kpad_) {
  __shared__ __attribute__((aligned(16))) int8_t tab[kMaxC * 256];
  const I B = (I)B_, C = (I)C_, H = (I)H_, W = (I)W_, OH = (I)OH_, OW = (I)OW_, ldc = (I)ldc_, kpad = (I)kpad_;
  stage_table(code_table, tab, (int)C * 256);
  const I K = C * kh * kw;
  const I rows = B * OH * OW;
  // work items per row: 16-column chunks; on kNhwc3 a pixel chunk stands for its three channels' chunks
  const I pix_chunks = kh * (kw / 16);
  const I per_row = (ARM == kNhwc3) ? pix_chunks + (kpad - K) / 16 : kpad / 16;
  const I total = rows * per_row;
  for (I id = blockIdx.x * (I)blockDim.x + threadIdx.x; id < total; id += (I)gridDim.x * blockDim.x) {
    const I r = id / per_row;
    const I j = id - r * per_row;
    const I b = r / (OH * OW);
    const I rem = r - b * OH * OW;
    const I oh = rem / OW, ow = rem - (rem / OW) * OW;
    int8_t* dst_row = codes + r * ldc;
    if (ARM == kNhwc3) {
      if (j >= pix_chunks) {
        *reinterpret_cast<uint4*>(dst_row + K + (j - pix_chunks) * 16) = make_uint4(0, 0, 0, 0);
        continue;
      }
      const I ih = j / (kw / 16), iw0 = (j - ih * (kw / 16)) * 16;
      const I y = oh * sh + ih * dh;
      const I xx = ow * sw + iw0;
      const uint4* src = reinterpret_cast<const uint4*>(img + ((b * H + y) * W + xx) * 3);
      uint32_t p[12];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const uint4 v = src[q];
        p[4 * q + 0] = v.x; p[4 * q + 1] = v.y; p[4 * q + 2] = v.z; p[4 * q + 3] = v.w;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t acc = 0;
#pragma unroll
          for (int bb = 0; bb < 4; ++bb)
            acc |= ((uint32_t)(uint8_t)tab[c * 256 + byte_of(p, 3 * (4 * i + bb) + c)]) << (8 * bb);
          w[i] = acc;
        }
        *reinterpret_cast<uint4*>(dst_row + c * kh * kw + ih * kw + iw0) = make_uint4(w[0], w[1], w[2], w[3]);
      }
      continue;
    }
    const I c0 = j * 16;
    uint32_t w[4];
    if (ARM == kNchw16) {
      if (c0 >= K) {   // K % 16 == 0 here: a chunk is inside the patch or all padding
        w[0] = w[1] = w[2] = w[3] = 0;
      } else {
        const I ci = c0 / (kh * kw);
        const I r2 = c0 - ci * kh * kw;
        const I ih = r2 / kw, iw = r2 - ih * kw;
        const I y = oh * sh + ih * dh;
        const I xx = ow * sw + iw;
        const uint4 v = *reinterpret_cast<const uint4*>(img + ((b * C + ci) * H + y) * W + xx);
        const uint32_t p[4] = {v.x, v.y, v.z, v.w};
        const int8_t* t = tab + ci * 256;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          uint32_t acc = 0;
#pragma unroll
          for (int bb = 0; bb < 4; ++bb) acc |= ((uint32_t)(uint8_t)t[byte_of(p, 4 * i + bb)]) << (8 * bb);
          w[i] = acc;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t acc = 0;
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) {
          const I kk = c0 + 4 * i + bb;
          uint32_t code = 0;
          if (kk < K) {
            const I ci = kk / (kh * kw);
            const I r2 = kk - ci * kh * kw;
            const I ih = r2 / kw, iw = r2 - ih * kw;
            const I y = oh * sh - ph + ih * dh;
            const I xx = ow * sw - pw + iw * dw;
            if (y >= 0 && y < H && xx >= 0 && xx < W) {
              const I at = nhwc ? ((b * H + y) * W + xx) * C + ci : ((b * C + ci) * H + y) * W + xx;
              code = (uint8_t)tab[ci * 256 + img[at]];
            }
          }
          acc |= code << (8 * bb);
        }
        w[i] = acc;
      }
    }
    *reinterpret_cast<uint4*>(dst_row + c0) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// one thread = up to four consecutive x of one output row (b, c, y); a 16-byte store where W and `out` allow
template <typename I>
__global__ __launch_bounds__(kThreads) void u8_normalize_kernel(
    const uint8_t* __restrict__ img, int64_t B_, int64_t C_, int64_t H_, int64_t W_, int nhwc,
    const float* __restrict__ value_table, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float tab[kMaxC * 256];
  const I B = (I)B_, C = (I)C_, H = (I)H_, W = (I)W_;
  stage_table(value_table, tab, (int)C * 1024);
  const bool vec = (W % kVec == 0) && ((((uintptr_t)out) & 15) == 0);
  const I groups = (W + kVec - 1) / kVec;
  const I total = B * C * H * groups;
  for (I id = blockIdx.x * (I)blockDim.x + threadIdx.x; id < total; id += (I)gridDim.x * blockDim.x) {
    const I row = id / groups;              // (b, c, y)
    const I x0 = (id - row * groups) * kVec;
    const I bc = row / H;
    const I y = row - bc * H;
    const I b = bc / C;
    const I c = bc - b * C;
    const uint8_t* src = nhwc ? img + ((b * H + y) * W + x0) * C + c : img + row * W + x0;
    const I step = nhwc ? C : (I)1;
    const float* t = tab + c * 256;
    float* dst = out + row * W + x0;
    if (vec) {
      float4 o;
      o.x = t[src[0]]; o.y = t[src[step]]; o.z = t[src[2 * step]]; o.w = t[src[3 * step]];
      *reinterpret_cast<float4*>(dst) = o;
    } else {
#pragma unroll
      for (int i = 0; i < kVec; ++i)
        if (x0 + i < W) dst[i] = t[src[i * step]];
    }
  }
}

// the element arithmetic fits int, with headroom for the grid stride (the rule of qvit_im2col_quant_i8)
bool fits_int(int64_t a, int64_t b, int64_t c) {
  const int64_t lim = (int64_t)INT32_MAX - 2 * (int64_t)256 * 16 * kThreads;
  return a < lim && b < lim && c < lim;
}

template <typename I>
void launch_im2col(int arm, int grid, hipStream_t stream, const uint8_t* img, int64_t B, int64_t C, int64_t H,
                   int64_t W, int layout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int64_t OH,
                   int64_t OW, const int8_t* table, int8_t* codes, int64_t ldc, int64_t kpad) {
#define QVIT_U8_LAUNCH(ARM)                                                                                         \
  hipLaunchKernelGGL((im2col_u8_kernel<I, ARM>), dim3(grid), dim3(kThreads), 0, stream, img, B, C, H, W, layout, kh, \
                     kw, sh, sw, ph, pw, dh, dw, OH, OW, table, codes, ldc, kpad)
  if (arm == kNchw16) QVIT_U8_LAUNCH(kNchw16);
  else if (arm == kNhwc3) QVIT_U8_LAUNCH(kNhwc3);
  else QVIT_U8_LAUNCH(kScalar);
#undef QVIT_U8_LAUNCH
}

}  // namespace

extern "C" {

int qvit_im2col_u8_i8(const uint8_t* img, int64_t B, int64_t C, int64_t H, int64_t W, int layout, int kh, int kw,
                      int sh, int sw, int ph, int pw, int dh, int dw, const int8_t* code_table, int8_t* codes,
                      int64_t ldc, int64_t kpad, hipStream_t stream) {
  if (!img || !code_table || !codes) return QVIT_ENULL;
  if (layout != QVIT_U8_NCHW && layout != QVIT_U8_NHWC) return QVIT_EINVAL;
  ConvShape cs;
  if (qvit_conv_shape(B, C, H, W, kh, kw, sh, sw, ph, pw, dh, dw, cs)) return QVIT_EINVAL;
  if (C > kMaxC) return QVIT_EINVAL;
  if (kpad < cs.K || kpad % 16 || ldc < kpad) return QVIT_EINVAL;
  if ((ldc % 16) || qvit_misaligned(15, codes)) return QVIT_EALIGN;
  if (B == 0) return QVIT_OK;
  const bool wide16 = kw % 16 == 0 && dw == 1 && ph == 0 && pw == 0 && W % 16 == 0 && sw % 16 == 0 &&
                      !qvit_misaligned(15, img);
  const int arm = !wide16 ? kScalar : (layout == QVIT_U8_NCHW ? kNchw16 : (C == 3 ? kNhwc3 : kScalar));
  const int64_t chunks = cs.M * (kpad / 16);
  // kNhwc3: a pixel chunk covers its three channels' chunks, the padding chunks stay one work item each
  const int64_t work = arm == kNhwc3 ? cs.M * (kh * (int64_t)(kw / 16) + (kpad - cs.K) / 16) : chunks;
  const int grid = grid_for(work, kThreads);
  if (fits_int(chunks, B * C * H * W, cs.M * ldc))
    launch_im2col<int>(arm, grid, stream, img, B, C, H, W, layout, kh, kw, sh, sw, ph, pw, dh, dw, cs.OH, cs.OW,
                       code_table, codes, ldc, kpad);
  else
    launch_im2col<int64_t>(arm, grid, stream, img, B, C, H, W, layout, kh, kw, sh, sw, ph, pw, dh, dw, cs.OH, cs.OW,
                           code_table, codes, ldc, kpad);
  return qvit_launch_status();
}

int qvit_u8_normalize_f32(const uint8_t* img, int64_t B, int64_t C, int64_t H, int64_t W, int layout,
                          const float* value_table, float* out, hipStream_t stream) {
  if (!img || !value_table || !out) return QVIT_ENULL;
  if (layout != QVIT_U8_NCHW && layout != QVIT_U8_NHWC) return QVIT_EINVAL;
  const int64_t ext = (int64_t)1 << 20;   // bounds the products below
  if (B < 0 || C < 1 || H < 1 || W < 1 || B > ext || H > ext || W > ext || C > kMaxC) return QVIT_EINVAL;
  if (qvit_misaligned(3, value_table, out)) return QVIT_EALIGN;
  if (B == 0) return QVIT_OK;
  const int64_t n = B * C * H * W;
  const int64_t work = B * C * H * ((W + kVec - 1) / kVec);
  const int grid = grid_for(work, kThreads);
  if (fits_int(n, n, n))
    hipLaunchKernelGGL(u8_normalize_kernel<int>, dim3(grid), dim3(kThreads), 0, stream, img, B, C, H, W, layout,
                       value_table, out);
  else
    hipLaunchKernelGGL(u8_normalize_kernel<int64_t>, dim3(grid), dim3(kThreads), 0, stream, img, B, C, H, W, layout,
                       value_table, out);
  return qvit_launch_status();
}

}  // extern "C"
