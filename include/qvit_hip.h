/*
 * qvit_hip.h — C-ABI of libqvit_hip.so, the MI355X (gfx950) implementation of the
 * 4-bit QuantizeLinear / QuantizeConv2d forward path of LongAoTianxia/Quantized_ViT.
 *
 * Every entry point replaces one step of the reference's fake-quant forward
 * (paths relative to the reference checkout; OTO = QViT_with_GETA/only_train_once):
 *
 *   qvit_quantize_act_i8      OTO/quantization/quant_layers.py:356-381 (QuantizeMixin.quantize_act)
 *                             -> SymQuantizerLinear.forward :137-161 / SymQuantizerNonLinear.forward :41-69,
 *                             emitted as integer codes k (value = d * k) instead of fake-quant floats;
 *                             also 4-bit quantization/quant_ultra.py:59-73 (activation_quantize_fn).
 *   qvit_fake_quant_f32       the same quantizers emitting the reference's fp32 fake-quant values
 *                             (used when a layer's level count does not fit int8, e.g. num_bits > 8).
 *   qvit_quant_backward       quant_layers.py:71-125 (SymQuantizerNonLinear.backward), :163-205
 *                             (SymQuantizerLinear.backward) and :248-290 (DGEQuantizer.backward): grad_x and the
 *                             three quantizer-scalar gradients in one streaming pass with a deterministic
 *                             two-stage reduction (the reference: ~30 elementwise launches and three host syncs).
 *   qvit_quant_error          the squared error of those quantizers' forward (quant_layers.py:41-69, :137-161) against
 *                             their un-rounded input, for up to 64 candidate (d_quant, q_m) pairs in one pass: the
 *                             scoring step of a clip search that stands in for GETA's learned parameters.
 *   qvit_qat_step / qvit_qat_quant_step
 *                             OTO/optimizer/geta.py:571-804, :873-943 and base_optimizer.py:40-86: the warm-up, bit-range
 *                             projection and fix stages of the GETA optimizer as one multi-tensor launch for the dense
 *                             tensors and one for the quantizer scalars, with no .item() on the way.
 *   qvit_prune_scores / qvit_prune_scores_fold / qvit_prune_scores_finish / qvit_prune_joint_scalars /
 *   qvit_prune_joint_reduce /
 *   qvit_prune_joint_finish / qvit_prune_joint_apply
 *                             OTO/optimizer/geta.py:167-248, :281-521, :944-1026 and base_hybrid_sparse_optimizer.py:
 *                             194-291: the saliency scores and the joint pruning and quantization stage for declared
 *                             row groups, a fixed number of launches per step and no .item().
 *   qvit_pack_weight          quant_layers.py:332-354 (QuantizeMixin.quantize_weight) + the GEMM operand
 *                             layout: codes packed int4 (8 per u32) or int8, rows padded/permuted.
 *   qvit_im2col_quant_i8      quant_layers.py:575-587 (QuantizeConv2d.forward): the conv input patches
 *                             quantized to codes, K-order (c, kh, kw) = the reference weight flattening.
 *   qvit_im2col_u8_i8 / qvit_u8_normalize_f32
 *                             predict.py:18-19 and train.py:150-151 (transforms.ToTensor + transforms.Normalize on the
 *                             host) folded into the step above: the image stays uint8 up to the device, and the
 *                             normaliser (with quantize_act, for the codes) is a table of 256 entries per channel.
 *   qvit_layernorm_quant_i8   vit_model.py:193,206-207 (Block.norm1/norm2, eps 1e-6) fused with the next
 *                             QuantizeLinear's quantize_act (quant_layers.py:497-498).
 *   qvit_gemm                 quant_layers.py:499 (nn.functional.linear on fake-quant operands) as an
 *                             int8 x int4/int8 -> int32 MFMA contraction with a fused epilogue:
 *                             d_act * d_wt * acc + bias, optionally + residual (vit_model.py:206-207),
 *                             or GELU (vit_model.py:173) + the next layer's activation quantizer.
 *   qvit_gemm_wonly           quant_layers.py:495-499 in the default WEIGHT_ONLY mode (quant_model.py:23): fp32
 *                             activations x int4/int8 weight codes on bf16 MFMA (x split into three exact
 *                             bf16 terms), d_wt * acc + bias — F.linear(x, quantize_weight(W), b).
 *   qvit_gemm_wgrad           the backward of quant_layers.py:499's F.linear w.r.t. the quantized weight on the
 *                             integer path: fp32 grad_out^T x int8 activation codes on bf16 MFMA (the same exact
 *                             three-term split); the input's gradient is qvit_gemm_wonly on transposed codes.
 *   qvit_col2im_quant_backward  the backward of quant_layers.py:575-587 (QuantizeConv2d.forward) w.r.t. its input behind
 *                             the im2col lowering: col2im of the patch-row gradient fused with quantize_act's backward.
 *   qvit_conv_wonly           quant_layers.py:575-587 (QuantizeConv2d.forward, WEIGHT_ONLY) and quant_ultra.py:85-89
 *                             (Conv2d_Q.forward): the same contraction as an implicit GEMM over the NCHW input
 *                             (patches gathered in the kernel), NCHW fp32 out — F.conv2d(x, quantize_weight(W), b).
 *   qvit_ultra_*              4-bit quantization/quant_ultra.py:8-91 + mymodel.py:62-144 (UltraNet: weight
 *                             codes, BN folding, fused conv+BN+quantizer+maxpool blocks, the 26 x 26 tail of
 *                             the network in one launch, YOLO decode).
 *   qvit_ultra_weight_quant_backward / qvit_ultra_act_quant_backward / qvit_conv_wgrad
 *                             4-bit quantization/quant_ultra.py:8-27 (uniform_quantize's straight-through
 *                             backward) behind :50-55 (weight_quantize_fn), :71 (activation_quantize_fn) and
 *                             :85-89 (Conv2d_Q's F.conv2d, the weight gradient against the activation codes).
 *   qvit_bn_stats / qvit_bn_act_pool_forward / qvit_bn_act_pool_backward_reduce / qvit_bn_act_pool_backward_dx
 *                             4-bit quantization/mymodel.py:71-124 in training mode: the nn.BatchNorm2d (batch
 *                             statistics) -> activation_quantize_fn (quant_ultra.py:59-73) -> nn.MaxPool2d(2, 2)
 *                             run between two Conv2d_Q, forward and backward, as streaming passes over NCHW fp32.
 *   qvit_attention            vit_model.py:133-149 (Attention.forward between qkv and proj):
 *                             softmax(q k^T * scale) v per (image, head), fp32 out or fused with the
 *                             proj layer's quantize_act (quant_layers.py:497) -> int8 codes.
 *   qvit_attention_backward   the gradient autograd takes through vit_model.py:133-149 (dq, dk, dv from dO),
 *                             softmax recomputed on chip, nothing N x N in memory.
 *
 * Conventions
 *   - Plain pointers and sizes only. All pointers are device pointers (hipMalloc'd / torch CUDA
 *     tensors) unless stated otherwise. Every entry point is stream-ordered on `stream`, never
 *     synchronises the host, never allocates, and is safe to capture into a hipGraph.
 *   - Quantizer parameters are per-tensor device scalars (float[1]): d_quant, q_m, t_quant, exactly the
 *     reference's nn.Parameter([1]) tensors (quant_layers.py:315-325). t_quant may be NULL for the
 *     linear quantizer. Reading them on the device keeps the host free of .item() syncs.
 *   - Return value: 0 on success; QVIT_E* (< 0) on a rejected argument; QVIT_EHIP - hipError_t
 *     when a launch fails. qvit_strerror() maps a code to text.
 */
#ifndef QVIT_HIP_H
#define QVIT_HIP_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------- */
#define QVIT_OK          0
#define QVIT_EINVAL     -1   /* bad size / stride / enum */
#define QVIT_EALIGN     -2   /* pointer or leading dimension not aligned as required */
#define QVIT_ENULL      -3   /* required pointer is NULL */
#define QVIT_EHIP    -1000   /* QVIT_EHIP - (int)hipError_t */

/* ---- quantizer kinds (QuantizationType, quant_layers.py:20-24; quant_ultra.py) ---------- */
#define QVIT_QT_LINEAR      0  /* SymQuantizerLinear / DGEQuantizer forward: k = sgn(x) rne(|x|/d) */
#define QVIT_QT_NONLINEAR   1  /* SymQuantizerNonLinear: k = sgn(x) rne(exp(t log|x|)/d)          */
#define QVIT_QT_ULTRA_ACT   2  /* quant_ultra activation_quantize_fn: k = rne(clamp(x,0,1) (2^b-1)),
                                  d_quant = NULL, the level count 2^b-1 is passed as `levels`      */

/* ---- GEMM weight storage ---------------------------------------------------------------- */
#define QVIT_W4 4   /* int4 codes, 8 per uint32 (see qvit_pack_weight for the nibble order) */
#define QVIT_W8 8   /* int8 codes                                                           */
#define QVIT_W4R 40 /* qvit_gemm / qvit_gemm_qkv_split only: QVIT_W4 codes in the register-weight image
                       (qvit_pack_weight_w4r); same results, each wave's weight rows loaded into registers */
#define QVIT_W8R 80 /* qvit_gemm / qvit_gemm_qkv_split only: QVIT_W4 codes in the int8 register image
                       (qvit_pack_weight_w8r); same results, no unpack in the main loop, twice the bytes  */
#define QVIT_W16 16 /* qvit_gemm_wonly only: codes |k| <= 32639 as balanced base-256 digits k = 256 h + l, h and l
                       in [-128, 127], two QVIT_W8 images of npad * kpad bytes (h, then l; qvit_pack_weight)  */
#define QVIT_W24 24 /* the same with three digits k = 65536 a + 256 h + l (|k| < 2^23, e.g. 16-bit layers whose
                       saturation code is 32768): three QVIT_W8 images, a, h, l                               */

/* ---- GEMM epilogues ----------------------------------------------------------------------- */
#define QVIT_EPI_F32        0  /* C[m,n]  = d_act d_wt acc + bias[n]                 (fp32)          */
#define QVIT_EPI_F32_RESID  1  /* C[m,n] += d_act d_wt acc + bias[n]                 (fp32, in place) */
#define QVIT_EPI_I8_GELU    2  /* C[m,n]  = q_next(gelu(d_act d_wt acc + bias[n]))  (int8 codes)    */
#define QVIT_EPI_I8         3  /* C[m,n]  = q_next(d_act d_wt acc + bias[n])        (int8 codes)    */
#define QVIT_EPI_I32        4  /* C[m,n]  = acc                                      (int32, exact)  */
#define QVIT_EPI_QKV_SPLIT  5  /* fp16 hi/lo planes of in_scale (d_act d_wt acc + bias[n]); only via
                                  qvit_gemm_qkv_split (qvit_gemm rejects it)                        */

/* ---- qvit_ultra_conv epilogues (UltraNet, 4-bit quantization/mymodel.py) -------------------- */
#define QVIT_ULTRA_CODES       0  /* codes = rne(clamp(bn(acc/den), 0, 1) (2^a_bit-1))       (uint codes) */
#define QVIT_ULTRA_CODES_POOL  1  /* the same followed by MaxPool2d(2, 2)                    (uint codes) */
#define QVIT_ULTRA_F32         2  /* out = acc/den + bias (shift = bias)                      (fp32)       */

/* ---- qvit_attention output modes -------------------------------------------------------------- */
#define QVIT_ATT_F32        0  /* out = softmax(q k^T * scale) v                     (fp32)          */
#define QVIT_ATT_I8         1  /* out = q_next(softmax(q k^T * scale) v)             (int8 codes)    */

/* ---- uint8 image layouts (qvit_im2col_u8_i8, qvit_u8_normalize_f32) ----------------------------- */
#define QVIT_U8_NCHW 0  /* byte ((b C + c) H + y) W + x: a decoded batch after permute + contiguous        */
#define QVIT_U8_NHWC 1  /* byte ((b H + y) W + x) C + c: a decoder's [B][H][W][C] output, torch.channels_last */

/* Tile geometry the packed operands must be padded to. */
#define QVIT_TILE_N  256   /* weight rows (out features) are padded to a multiple of this  */
#define QVIT_TILE_K  128   /* the reduction dim is padded to a multiple of this (zeros)    */

const char* qvit_strerror(int code);
/* Library version / build tag, e.g. "qvit_hip 0.1 gfx950". Host pointer, static storage. */
const char* qvit_version(void);

/*
 * Activation quantizer -> int8 codes (value = d_quant * code).
 *   x      : fp32 [rows][ldx], first `cols` columns used
 *   codes  : int8 [rows][ldc]; columns [cols, kpad) are written with 0 (kpad <= ldc, kpad % 16 == 0)
 *   qtype  : QVIT_QT_*; levels is only read for QVIT_QT_ULTRA_ACT.
 * Codes saturate at +-127 (the caller rejects layers whose level count exceeds 127).
 * Special values: a NaN gives code 0; +-Inf and +-FLT_MAX give +-min(L, 127), L the saturation code rne(p_sat / d);
 * +-0 and a finite value whose quotient rounds to 0 give 0; a negative q_m saturates every non-zero value. With
 * QVIT_QT_ULTRA_ACT a NaN gives 0 (fmax(NaN, 0)), -Inf 0 and +Inf `levels`. The codes are the same on the guarded fast
 * path and under QVIT_QT_FORCE_CAREFUL, on the 16-byte and the scalar loads, and for a nonlinear quantizer on values
 * below 1e-30 (denormals included), which always take the careful sequence; a step d below 2^-128, whose reciprocal
 * is not finite, sends every element there. An element changes its own code only. The same rules hold for every
 * int8 code output of this header (tests/test_gpu_special_values.py).
 * Replaces quant_layers.py:356-381 (+ :41-69 / :137-161) and quant_ultra.py:66-73.
 */
int qvit_quantize_act_i8(const float* x, int64_t rows, int64_t cols, int64_t ldx,
                         int qtype, const float* d_quant, const float* q_m, const float* t_quant,
                         int levels, int8_t* codes, int64_t ldc, int64_t kpad, hipStream_t stream);

/*
 * Fake-quant fp32 values exactly as the reference returns them (y = sgn(x) * (d * rne(...)),
 * saturation and zero masks in the reference's order). Elementwise over n contiguous floats.
 * Special values: as the reference on every input: a NaN comes out a NaN (sign(NaN) * output), +-Inf and +-FLT_MAX
 * +-d L, +-0 gives 0. QVIT_QT_ULTRA_ACT keeps NaN -> 0 (round(clamp(x, 0, 1) n) / n with fmax(NaN, 0) = 0). The codes
 * behind the values (qvit_quantize_act_i8, qvit_quant_error) keep NaN -> 0.
 * Replaces SymQuantizerLinear/NonLinear.forward (quant_layers.py:41-69,137-161) when a layer's
 * levels do not fit the integer path.
 */
int qvit_fake_quant_f32(const float* x, int64_t n, int qtype, const float* d_quant,
                        const float* q_m, const float* t_quant, int levels, float* y,
                        hipStream_t stream);

/*
 * Backward of the fake quantizers over n contiguous floats (q_s = 0): SymQuantizerLinear.backward
 * (quant_layers.py:163-205), SymQuantizerNonLinear.backward (:71-125) and, with dge_k > 0, DGEQuantizer.backward
 * (:248-290; linear forward only, k = 5 * 4 / num_bits as :236 derives it).
 *   grad_x        : grad_out, zeroed where x >= clip_hi or x <= clip_lo (:77-79, :169-171); with dge_k > 0 then
 *                   scaled by (1/k) |x - d/2|^(1/k - 1) and clamped to +-3 (:259-265). May alias grad_out.
 *   grad_scalars  : float[3] = sum(grad_out * term) for d_quant, q_m, t_quant (:95, :99, :105, :183, :187);
 *                   the t_quant sum is 0 for the linear quantizer. With a = |x|, p = a or exp(t log a), q = p / d:
 *                     d    : sgn(x) (rne(q) - q); sgn(x) (L - range_pow / d) where a >= q_m; 0 where a <= 0
 *                     q_m  : sgn(x) (linear) or sgn(x) t exp((t - 1) log(|q_m| + 1e-6)), only where a > q_m
 *                     t    : sgn(x) p log a; sgn(x) range_pow log(|q_m| + 1e-6) where a >= q_m; 0 where a <= 0
 *                   rne(q) is the code qvit_fake_quant_f32 / qvit_quantize_act_i8 produce for the same element.
 *                   Masks select (a masked element never contributes a NaN); a NaN in grad_out or in a parameter
 *                   reaches the sums, which is what the reference's NanInGradientError checks (:108-123, :190-204).
 *   workspace     : qvit_quant_backward_workspace_bytes(n) bytes, 8-byte aligned: one partial per workgroup,
 *                   folded in a fixed order by a second launch (no float atomics: a call is bitwise reproducible).
 * x, grad_out and grad_x must be 16-byte aligned. qtype is QVIT_QT_LINEAR or QVIT_QT_NONLINEAR (t_quant required).
 * n == 0 writes three zeros. qvit_quant_backward_workspace_bytes returns QVIT_EINVAL for n < 0.
 */
int64_t qvit_quant_backward_workspace_bytes(int64_t n);
int qvit_quant_backward(const float* x, const float* grad_out, int64_t n, int qtype,
                        const float* d_quant, const float* q_m, const float* t_quant,
                        float clip_lo, float clip_hi, float dge_k,
                        float* grad_x, float* grad_scalars /* [3] */,
                        void* workspace, int64_t workspace_bytes, hipStream_t stream);

/*
 * Quantization error of x under ncand candidate quantizers that share the type and t: the scoring pass of an
 * error-minimising clip search (calibrate.py; GETA's projection picks d = q_m^t / (2^(b-1) - 1) from the same
 * family, optimizer/geta.py:788-804). One read of x per block of 16 candidates replaces one qvit_fake_quant_f32
 * pass and one reduction per candidate.
 *   x        : fp32 [rows][ldx], cols <= ldx; columns >= cols are never read. May be NULL when rows * cols == 0.
 *   d, q_m   : device float[ncand], 1 <= ncand <= 64. t: device float[1] shared by all candidates (NULL for
 *              QVIT_QT_LINEAR). qtype is QVIT_QT_LINEAR or QVIT_QT_NONLINEAR; QVIT_QT_FORCE_CAREFUL-style flag bits
 *              are accepted and change nothing (every element takes the careful sequence here).
 *   err[c]   : double, sum over the elements of ((double)p - (double)fq)^2 with fq = the fp32 value
 *              qvit_fake_quant_f32 returns for x under (d[c], q_m[c], t), rounding ties included, and the target
 *              p = x (linear) or sgn(x) exp(t log|x|) (nonlinear: the un-rounded fp32 input_pow of
 *              quant_layers.py:63, taken once per element; sgn is torch.sign, 0 at 0).
 *   nclip[c] : int64, the number of elements with |x| >= q_m[c] (the saturation mask, :67, :159).
 *   accumulate : 0 overwrites err and nclip; otherwise the call adds to what they hold, so a caller streams batches.
 *   workspace  : qvit_quant_error_workspace_bytes(rows, cols, ncand) bytes (16 per workgroup and candidate, at most
 *              1024 workgroups), 8-byte aligned, contents irrelevant.
 * rows * cols == 0 writes zeros, or nothing under accumulate. A NaN or infinite x makes every err[c] non-finite (it
 * is not masked) and is counted in nclip only where |x| >= q_m[c] holds (never for a NaN).
 * Reduction: per-thread double accumulation, a fixed-order wave / workgroup tree, one partial per workgroup and
 * candidate, folded in index order by a second launch that also applies `accumulate`. No atomics: two identical
 * calls give identical bits. A thread takes 4 consecutive elements per step as one 16-byte load when x is 16-byte
 * aligned and cols % 4 == 0, ldx % 4 == 0, else one by one with the same element-to-thread map: the same bits.
 * 32-bit indexing when rows * ldx < 2^31 - 2^21, else 64-bit (the rule of qvit_im2col_quant_i8).
 * Order of the checks (part of the ABI): d, q_m, err, nclip or workspace NULL (QVIT_ENULL); the qtype (unknown
 * enum, stray flag bits, QVIT_QT_ULTRA_ACT: QVIT_EINVAL); nonlinear with t NULL (QVIT_ENULL); the sizes (ncand
 * outside 1 .. 64, rows < 0, cols < 0, ldx < cols, rows * ldx > 2^48: QVIT_EINVAL); a short workspace
 * (QVIT_EINVAL); x NULL with rows * cols > 0 (QVIT_ENULL); alignment (x, d, q_m, t 4 bytes; err, nclip, workspace
 * 8: QVIT_EALIGN). qvit_quant_error_workspace_bytes returns QVIT_EINVAL on the same size errors (with ldx = cols).
 */
int64_t qvit_quant_error_workspace_bytes(int64_t rows, int64_t cols, int ncand);
int qvit_quant_error(const float* x, int64_t rows, int64_t cols, int64_t ldx, int qtype, const float* d,
                     const float* q_m, const float* t, int ncand, int accumulate, double* err, int64_t* nclip,
                     void* workspace, int64_t workspace_bytes, hipStream_t stream);

/*
 * The quantization-aware stages of the GETA optimizer (optimizer/geta.py:571-804, :873-943 with the pruning stages
 * absent; grad_variant of optimizer/base_optimizer.py:40-86) as at most two launches per step, neither of which
 * reads anything back to the host. fp32, one IEEE operation per reference operation in the reference's order, fmaf
 * where torch's CPU add_(b, alpha=s) is a fused multiply-add, correctly rounded division and sqrt, safe_guard 1e-8
 * added after the sqrt.
 *
 * Hyper-parameters, by value, the same for both entry points:
 *   variant        : QVIT_QAT_SGD (momentum, dampening, coupled weight decay), QVIT_QAT_ADAM, QVIT_QAT_ADAMW (decay
 *                    applied to p at the step's rate before the gradient step).
 *   first_step     : non-zero on the optimizer's first step: every moment becomes grad (grad^2), un-scaled
 *                    (base_optimizer.py:20-21, :31-32); a descriptor's own flag says the same for one tensor.
 *   lr, lr_quant   : the rates of learning-rate class 0 and 1.
 *   first_momentum, second_momentum : the moment decay factors; <= 0 keeps no such moment (the gradient stands in).
 *   alpha1, alpha2 : 1 - dampening of the two moment updates as the host rounds them from double (adam: 1 - the
 *                    momenta; sgd: alpha1 = 1 - dampening, alpha2 unused).
 *   weight_decay   : 0 for none.  bias_correction1/2: 1 - momentum^step (adam, adamw).
 *   clip_lo, clip_hi : grad is clamped into [clip_lo, clip_hi] as it is loaded (geta.py:160-165; -inf, +inf: off).
 *
 * qvit_qat_step — every dense tensor from one launch.
 *   tensors : device table of ntensors descriptors of 48 bytes: { float* p; const float* grad; float* m; float* v;
 *             int64_t numel; int32_t lr_class; int32_t flags; }. grad NULL skips the tensor and leaves its moments
 *             untouched (base_optimizer.py:51); m / v NULL where the variant keeps no such moment; flags bit 0: this
 *             tensor's first step. The tensors stay in their own storage.
 *   chunks  : device list of nchunks pairs { int32_t tensor; int32_t index; }: elements [4096 index, 4096 (index +
 *             1)) of that tensor, clipped to numel. Workgroups (at most 1024) stride over the list. Pairs that name
 *             no tensor or start past numel are skipped. A tensor whose p, grad, m and v are all 16-byte aligned is
 *             read and written 16 bytes at a time with a scalar tail; any other one element at a time: same bits.
 * Order of the checks (part of the ABI): tensors or chunks NULL (QVIT_ENULL); either off 8 bytes (QVIT_EALIGN);
 * ntensors < 0, nchunks < 0 or nchunks > 2^40 (QVIT_EINVAL); unknown variant (QVIT_EINVAL). ntensors == 0 or
 * nchunks == 0 is a no-op success.
 *
 * qvit_qat_quant_step — every quantizer scalar and the stage's projection, one thread per (layer, side).
 *   quants  : device table of nquants descriptors of 64 bytes: { float* s[3]; const float* g[3]; float* mom;
 *             int32_t side; int32_t flags; }: d_quant, q_m, t_quant (t NULL: t = 1, the linear type), their gradients
 *             (NULL: that scalar is skipped), six floats of moments (first of d, q_m, t, then second), side 0 weight /
 *             1 activation, flags bits 0..2: first step of d, q_m, t.
 *   Update  : all three at lr_quant. In QVIT_QAT_RANGE an activation-side triple is first stepped at lr and then
 *             again at lr_quant from the same grad_variant, as geta.py:598-630 followed by :667-697 does.
 *   stage   : QVIT_QAT_WARMUP no projection; QVIT_QAT_RANGE d is clamped into [d(max_bit), d(min_bit)] of its side
 *             with d(b) = exp(t log(max(|q_m|, 1e-10))) / (2^(b-1) - 1) evaluated in double from the updated q_m
 *             and t and rounded to fp32 (geta.py:787-804); QVIT_QAT_FIX d = d(bits[i]). With first_fix non-zero
 *             bits[i] = rint(log2(exp(t log|q_m|) / |d| + 1) + 1) (half to even; geta.py:774-785) is taken first,
 *             from the scalars as the step finds them (the reference reads them before its update, :932-940).
 *   bits    : device int32[nquants], written under first_fix, read in QVIT_QAT_FIX.
 * Order of the checks: quants or bits NULL (QVIT_ENULL); quants off 8 bytes or bits off 4 (QVIT_EALIGN);
 * nquants < 0 (QVIT_EINVAL); unknown variant (QVIT_EINVAL); unknown stage (QVIT_EINVAL); a bit range outside
 * 2 <= min <= max <= 32 on either side (QVIT_EINVAL). nquants == 0 is a no-op success.
 */
#define QVIT_QAT_SGD    0
#define QVIT_QAT_ADAM   1
#define QVIT_QAT_ADAMW  2
#define QVIT_QAT_WARMUP 0
#define QVIT_QAT_RANGE  1
#define QVIT_QAT_FIX    2
int qvit_qat_step(const void* tensors, int ntensors, const void* chunks, int64_t nchunks, int variant,
                  int first_step, float lr, float lr_quant, float first_momentum, float second_momentum,
                  float alpha1, float alpha2, float weight_decay, float bias_correction1, float bias_correction2,
                  float clip_lo, float clip_hi, hipStream_t stream);
int qvit_qat_quant_step(const void* quants, int nquants, int32_t* bits, int stage, int first_fix, int variant,
                        int first_step, float lr, float lr_quant, float first_momentum, float second_momentum,
                        float alpha1, float alpha2, float weight_decay, float bias_correction1,
                        float bias_correction2, float clip_lo, float clip_hi, int min_bit_wt, int max_bit_wt,
                        int min_bit_act, int max_bit_act, hipStream_t stream);

/*
 * The pruning stages of the GETA optimizer for declared row groups (optimizer/geta.py:167-248, :281-521, :944-1026;
 * base_hybrid_sparse_optimizer.py:194-291; the importance_score package). A group is a set of member tensors sliced along
 * dim 0: row r of the group is row r of every member. The launches per step do not depend on the number of groups,
 * and nothing is read back. The hyper-parameters are those of qvit_qat_step, and the gradient variant is recomputed
 * in registers from grad, m and v by the function qvit_qat_step runs.
 *
 * Device tables (the host fills them as int64 rows):
 *   groups  : ngroups descriptors of 64 bytes: { float* d; const float* q_m; const float* t; int32_t member_begin,
 *             member_count; int32_t rows; int32_t joint; int32_t red_begin, red_count; int64_t elems; int32_t
 *             sections, unit_rows; }: the weight quantizer scalars of the group's layer (t NULL: the linear type), its
 *             members [member_begin, member_begin + member_count) of `members`, its row count, joint = 1 while it has
 *             active redundant rows, the range of its redundant rows in the reduce's item list, elems = the elements
 *             of one unit over all members, and the geometry of a unit: sections and unit_rows both 0 (or 1): a unit
 *             is one row; else a member has sections x units x unit_rows rows and unit h is the rows (s units + h)
 *             unit_rows + j for s in [0, sections), j in [0, unit_rows) (head h of a qkv projection: sections = 3,
 *             unit_rows = the head dim).
 *   members : nmembers descriptors of 48 bytes: { float* p; const float* grad; float* m; float* v; int64_t width;
 *             int32_t quantized; int32_t flags; }: qvit_qat_step's tensor descriptor with the row width in place of
 *             numel; quantized = 1 for the layer's weight; flags bit 0: this tensor's first step. A member whose
 *             four pointers are 16-byte aligned and whose width is a multiple of 4 moves 16 bytes at a time, any
 *             other one element at a time: same bits.
 *   items   : nitems entries of 16 bytes: { int32_t group, row, state, link; }, state 0 important, 1 active
 *             redundant, 2 pruned: the state of the row's unit. A wave owns one item, a physical row in every geometry.
 *             link = the row's unit, 0 where a unit is one row. Items that name no group or no row of it are skipped.
 *   units   : (qvit_prune_scores_fold and the finish behind it) the same 16 bytes per unit: row = the unit's index
 *             in its group, link = the index in `items` of row 0 of that group, whose rows follow it in ascending
 *             order.
 *
 * qvit_prune_scores: sums[3 i .. 3 i + 2] = sum p^2, sum g^2, sum p g of item i's row over the members, g the
 *   gradient variant, in double (a member without grad adds to sum p^2 only).
 * qvit_prune_scores_fold: unit_sums[3 u ..] = the three sums of unit u added up over its rows' entries of `sums`,
 *   section-major, row ascending, by one thread: the same bits in every run. A unit whose group, index or rows do not
 *   agree with the tables (the row items' group, row and link are compared) gets zeros. Only needed where some group
 *   has units of several rows; the finish then takes `units` and `unit_sums` for items and sums, and scores has one
 *   entry per unit.
 * qvit_prune_scores_finish: scores[i] = sum_c w_c score_c(i) / (sqrt(1e-8 + sum_j score_c(j)^2) + 1e-8) over the
 *   criteria magnitude = sqrt(sum p^2), avg_magnitude = magnitude / (elems + 1e-6), cosine = sum p g / (|p| + 1e-8) /
 *   (|g| + 1e-8) + 1, taylor1 = |sum p g|, taylor2 = 0.5 taylor1^2, in that order; a weight of 0 leaves a criterion
 *   out. One workgroup.
 * qvit_prune_joint_scalars: quants as qvit_qat_quant_step's. A weight-side triple: q_m and t step at lr_quant
 *   without decay, d only moves its moments (geta.py:952-960); an activation-side triple takes the range stage's
 *   activation pass (:667-721): one step at lr_quant, then d clamped into [d(max_bit_act), d(min_bit_act)].
 * qvit_prune_joint_reduce: items lists the rows of the active redundant units, a group's rows contiguous at [red_begin, red_begin +
 *   red_count); partials[6 i ..] = <clip, g>, |clip|^2, |g|^2, <res, g>, |res|^2, sum clip of that row, clip and res
 *   by _clip_helper and _residual_helper (:821-850) for the quantized member, clip = p and res = 0 for the others.
 * qvit_prune_joint_finish: one workgroup per group folds its partials in index order and evaluates compute_gamma_d
 *   (:373-499) in double with every branch; writes d to the group's d_quant, gamma[g] and info[g] (bits 0..2: 0
 *   mean(clip) < 1e-8, 1 non-finite cosine, 2 the schedule, 3 negative cosine, 4 / 5 clamped from above / below;
 *   bit 3 d = d_quant_upper by the safeguard, bit 4 the x 0.8 loop ran, bit 5 the final min took d_quant_upper, bit 6
 *   the loop was cut after 861 turns (fp32's whole exponent range): d = d_quant_upper, gamma = 0, where the reference
 *   would not end; -1 for a group that is not joint). lr is the host's double; period and t_in_period give the
 *   schedule 1 - (period - t - 1) / (period - t).
 * qvit_prune_joint_apply: items lists every row of every group. Joint groups: on the rows of redundant units p -= gamma *
 *   quantize(p) (weight; _quantize_helper :806-819 with the new d) or gamma * p (others), then p -= lr g without
 *   adamw's decay (:982-1008); other groups: the dense step. Moments as qvit_qat_step leaves them; pruned rows are
 *   written as zeros (base_hybrid_sparse_optimizer.py:194-211).
 * Order of the checks (part of the ABI), for scores, joint_reduce and joint_apply: a table or the output NULL
 * (QVIT_ENULL); any of them off 8 bytes (QVIT_EALIGN); a count < 0 or nitems > 2^31 - 1 (QVIT_EINVAL); unknown variant
 * (QVIT_EINVAL); a zero count is a no-op success. scores_fold: a table, sums or unit_sums NULL; any of the five off 8
 * bytes; a count < 0, nitems or nunits > 2^31 - 1; ngroups or nunits zero is a no-op success. scores_finish: NULL; groups, items or sums off 8 bytes or scores
 * off 4; counts. joint_scalars: NULL; off 8 bytes; nquants < 0; variant; the bit range. joint_finish: NULL; groups or
 * partials off 8 bytes or gamma or info off 4; counts; period < 1 or t_in_period outside [0, period); the bit range.
 */
int qvit_prune_scores(const void* groups, int ngroups, const void* members, int nmembers, const void* items,
                      int64_t nitems, double* sums, int variant, int first_step, float lr, float lr_quant,
                      float first_momentum, float second_momentum, float alpha1, float alpha2, float weight_decay,
                      float bias_correction1, float bias_correction2, float clip_lo, float clip_hi,
                      hipStream_t stream);
int qvit_prune_scores_fold(const void* groups, int ngroups, const void* items, int64_t nitems, const double* sums,
                           const void* units, int64_t nunits, double* unit_sums, hipStream_t stream);
int qvit_prune_scores_finish(const void* groups, int ngroups, const void* items, int64_t nitems, const double* sums,
                             double w_magnitude, double w_avg_magnitude, double w_cosine, double w_taylor1,
                             double w_taylor2, float* scores, hipStream_t stream);
int qvit_prune_joint_scalars(const void* quants, int nquants, int variant, int first_step, float lr, float lr_quant,
                             float first_momentum, float second_momentum, float alpha1, float alpha2,
                             float weight_decay, float bias_correction1, float bias_correction2, float clip_lo,
                             float clip_hi, int min_bit_act, int max_bit_act, hipStream_t stream);
int qvit_prune_joint_reduce(const void* groups, int ngroups, const void* members, int nmembers, const void* items,
                            int64_t nitems, double* partials, int variant, int first_step, float lr, float lr_quant,
                            float first_momentum, float second_momentum, float alpha1, float alpha2,
                            float weight_decay, float bias_correction1, float bias_correction2, float clip_lo,
                            float clip_hi, hipStream_t stream);
int qvit_prune_joint_finish(const void* groups, int ngroups, const double* partials, int64_t npartials, double lr,
                            int period, int t_in_period, int min_bit_wt, int max_bit_wt, float* gamma, int32_t* info,
                            hipStream_t stream);
int qvit_prune_joint_apply(const void* groups, int ngroups, const void* members, int nmembers, const void* items,
                           int64_t nitems, const float* gamma, int variant, int first_step, float lr, float lr_quant,
                           float first_momentum, float second_momentum, float alpha1, float alpha2,
                           float weight_decay, float bias_correction1, float bias_correction2, float clip_lo,
                           float clip_hi, hipStream_t stream);

/*
 * y = GELU(x) elementwise over n contiguous floats: nn.GELU() (QViT_with_GETA/vit_model.py:173,242), bit-identical
 * to torch's ATen CPU kernel (erf as Abramowitz-Stegun 7.1.26 with SLEEF's expf, IEEE division) — the same
 * function the QVIT_EPI_I8_GELU epilogue evaluates. For the Mlp path outside the fused block, and for tests.
 */
int qvit_gelu_f32(const float* x, int64_t n, float* y, hipStream_t stream);

/*
 * Train-time fusion of a QuantizeLinear's pre-op with its activation quantizer (train_fuse.hip): the backward of
 * qvit_layernorm_quant_i8, and GELU + quantizer forward and backward. No fp32 tensor of the pre-op's output exists.
 *
 * qvit_layernorm_quant_backward: backward of codes = quantize(LayerNorm(x)) given grad_y, the gradient with respect
 * to the quantizer's output (what the input-gradient GEMM returns).
 *   x        : fp32 [rows][ldx], the LayerNorm input; gamma, beta: fp32 [cols] (both required); eps as the forward.
 *   qtype .. clip_hi : the activation quantizer, as qvit_quant_backward (QVIT_QT_LINEAR / QVIT_QT_NONLINEAR).
 *   grad_y   : fp32 [rows][ldg];  grad_x : fp32 [rows][ldo], may be grad_y itself (then ldo == ldg).
 *   grad_gamma, grad_beta : fp32 [cols], sum over rows of gy * xhat and of gy (gy: the quantizer backward's grad_x at
 *              y = LayerNorm(x), xhat the normalized row); either may be NULL, and that reduction is skipped.
 *   grad_scalars : [3] for d_quant, q_m, t_quant: definitions, masks and NaN behaviour of qvit_quant_backward at y.
 *   y is recomputed with the operations of the forward in the same order, so every mask and rne(q) refers to the
 *   value the forward quantized. A NaN in grad_y reaches the scalar sums and only its own row of grad_x.
 *   workspace : qvit_layernorm_quant_backward_workspace_bytes(rows, cols) bytes, 16-byte aligned: one partial per
 *              workgroup, folded in a fixed order by a second launch (no float atomics: bitwise
 *              reproducible). The query returns QVIT_EINVAL for a negative size.
 * Fast path only: cols % 4 == 0, cols <= 2048, ldx, ldg, ldo % 4 == 0, x / gamma / beta / grad_y / grad_x 16-byte
 * aligned; anything else is QVIT_EALIGN and nothing is written (callers run the separate ops). rows == 0 writes zeros
 * to the sums. Columns [cols, ld*) are never touched. Moves 3 rows cols 4 bytes plus the partials.
 *
 * qvit_gelu_quant_i8: codes = quantize(GELU(h)), byte for byte qvit_quantize_act_i8(qvit_gelu_f32(h)); arguments as
 * qvit_quantize_act_i8.
 *
 * Special values: the codes of qvit_quantize_act_i8 at GELU(h) as torch computes it: GELU(NaN) and GELU(-Inf) = -Inf * 0
 * are NaN (code 0), GELU(+Inf) = +Inf (the saturation code); fast and QVIT_QT_FORCE_CAREFUL agree.
 *
 * qvit_gelu_quant_backward: qvit_quant_backward at a = GELU(h) followed by GELU's own derivative:
 * grad_h = (Phi(h) + h phi(h)) gy with Phi from the forward's erf; grad_scalars, workspace, alignment, aliasing
 * (grad_h may be grad_y) and n == 0 as qvit_quant_backward. Moves 3 n 4 bytes.
 */
int64_t qvit_layernorm_quant_backward_workspace_bytes(int64_t rows, int64_t cols);
int qvit_layernorm_quant_backward(const float* x, int64_t rows, int64_t cols, int64_t ldx,
                                  const float* gamma, const float* beta, float eps,
                                  int qtype, const float* d_quant, const float* q_m, const float* t_quant,
                                  float clip_lo, float clip_hi,
                                  const float* grad_y, int64_t ldg, float* grad_x, int64_t ldo,
                                  float* grad_gamma, float* grad_beta, float* grad_scalars /* [3] */,
                                  void* workspace, int64_t workspace_bytes, hipStream_t stream);
int qvit_gelu_quant_i8(const float* h, int64_t rows, int64_t cols, int64_t ldh, int qtype,
                       const float* d_quant, const float* q_m, const float* t_quant, int levels,
                       int8_t* codes, int64_t ldc, int64_t kpad, hipStream_t stream);
int64_t qvit_gelu_quant_backward_workspace_bytes(int64_t n);
int qvit_gelu_quant_backward(const float* h, const float* grad_y, int64_t n, int qtype,
                             const float* d_quant, const float* q_m, const float* t_quant,
                             float clip_lo, float clip_hi, float* grad_h, float* grad_scalars /* [3] */,
                             void* workspace, int64_t workspace_bytes, hipStream_t stream);

/*
 * Weight quantizer + GEMM operand packing (QuantizeMixin.quantize_weight, quant_layers.py:332-354).
 *   w      : fp32 [n][ldw], first k columns used (nn.Linear weight [out,in]; a conv weight
 *            [Cout,Cin,kh,kw] is passed as [Cout][Cin*kh*kw]).
 *   wfmt   : QVIT_W4 -> packed uint32 [npad][kpad/8]; QVIT_W8 -> int8 [npad][kpad].
 *            npad % QVIT_TILE_N == 0, kpad % QVIT_TILE_K == 0, npad >= n, kpad >= k; padding = 0.
 *   Row order: within every 64-row group the two 2-bit fields of the row index are swapped
 *   (packed row (r<<4)|(q<<2)|j holds weight row (q<<4)|(r<<2)|j) so that each GEMM lane ends up
 *   owning 16 consecutive output features.  W4 nibble order inside each uint32 covering
 *   k0..k0+7: byte b holds k0+b in bits [0,4) and k0+4+b in bits [4,8), two's complement.
 *   overflow (int32[1], device, may be NULL): atomically set to 1 if any code does not fit wfmt.
 */
int qvit_pack_weight(const float* w, int64_t n, int64_t k, int64_t ldw, int qtype,
                     const float* d_quant, const float* q_m, const float* t_quant, int wfmt,
                     void* packed, int64_t npad, int64_t kpad, int32_t* overflow,
                     hipStream_t stream);

/*
 * The register-weight image (QVIT_W4R) of a QVIT_W4 image from qvit_pack_weight: the same npad * kpad / 2 bytes,
 * re-ordered so that in every (256-row tile, 64-deep k stage) chunk of 8 KiB the GEMM lane l of wave w finds its
 * four 8-byte fragments (rows 64 w + 16 r + (l & 15) of the tile, r = 0..3, k bytes 8 (l >> 4) .. + 7 of the
 * stage) contiguously at byte 2048 w + 32 l. npad % QVIT_TILE_N == 0, kpad % QVIT_TILE_K == 0, kpad <= 65536;
 * out must not alias packed. qvit_gemm with wfmt QVIT_W4R on it gives the QVIT_W4 results byte for byte (same
 * accumulation order); it loads each wave's weights straight into registers instead of through LDS.
 * Replaces nothing in the reference: a second storage form of quantize_weight's codes (quant_layers.py:332-354).
 */
int qvit_pack_weight_w4r(const void* packed, int64_t npad, int64_t kpad, void* out, hipStream_t stream);

/*
 * The int8 register image (QVIT_W8R) of a QVIT_W4 image from qvit_pack_weight: npad * kpad bytes (twice the W4
 * image). In every (256-row tile, 64-deep k stage) chunk of 16 KiB the GEMM lane l of wave w finds its four 16-byte
 * MFMA operands (rows 64 w + 16 r + (l & 15) of the tile, r = 0..3, k 16 (l >> 4) .. + 15 of the stage, each code
 * as the byte 16 k) contiguously at byte 4096 w + 64 l. Same argument rules as qvit_pack_weight_w4r. qvit_gemm with
 * wfmt QVIT_W8R on it gives the QVIT_W4 results byte for byte (same operands, same accumulation order) with no int4
 * unpack in the main loop.
 * Replaces nothing in the reference: a third storage form of quantize_weight's codes (quant_layers.py:332-354).
 */
int qvit_pack_weight_w8r(const void* packed, int64_t npad, int64_t kpad, void* out, hipStream_t stream);

/*
 * Pads a bias vector to npad floats (zeros past n; bias may be NULL -> all zeros).
 */
int qvit_pad_bias(const float* bias, int64_t n, float* out, int64_t npad, hipStream_t stream);

/*
 * Conv input -> quantized im2col codes for QuantizeConv2d (quant_layers.py:575-587), groups == 1.
 *   x      : fp32 NCHW [B][C][H][W] contiguous
 *   codes  : int8 [B*OH*OW][ldc], row (b, oh, ow), column (c, ih, iw) = c*kh*kw + ih*kw + iw;
 *            columns [C*kh*kw, kpad) zero. Zero-padding of the image quantizes to code 0, as in
 *            the reference (quantize_act runs before F.conv2d pads).
 *   Special values: a NaN pixel gives code 0 and a +-Inf pixel the saturation code in exactly the entries that tap
 *   it (rows (b, oh, ow) and columns (c, ih, iw) with oh sh - ph + ih dh = y, ow sw - pw + iw dw = x); no other entry
 *   changes. qvit_im2col_u8_i8 takes bytes and a caller-made code table: a NaN or Inf in the normaliser's
 *   value_table is the caller's qvit_quantize_act_i8 call, nothing is defined here beyond that.
 *   OH = (H + 2 ph - dh (kh - 1) - 1) / sh + 1, OW alike; a padded image smaller than the dilated kernel on
 *   either axis is QVIT_EINVAL at every stride.
 */
int qvit_im2col_quant_i8(const float* x, int64_t B, int64_t C, int64_t H, int64_t W,
                         int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                         int qtype, const float* d_quant, const float* q_m, const float* t_quant,
                         int levels, int8_t* codes, int64_t ldc, int64_t kpad, hipStream_t stream);

/*
 * The same rows from a uint8 image: codes[(b, oh, ow)][c*kh*kw + ih*kw + iw] = code_table[c][img(b, c, y, x)].
 * With value_table[c][v] = (v / 255 - mean_c) / std_c (transforms.ToTensor + transforms.Normalize, predict.py:18-19)
 * and code_table = qvit_quantize_act_i8(value_table), the output equals qvit_im2col_quant_i8 on the fp32 image
 * value_table[c][img] byte for byte: an image byte has 256 values, so the table holds every code the quantizer can give.
 *   img        : uint8, [B][C][H][W] (layout QVIT_U8_NCHW) or [B][H][W][C] (QVIT_U8_NHWC), contiguous, any alignment
 *                (a 16-byte aligned image on the patchify geometry kw % 16 == 0, dw == 1, ph == pw == 0, W % 16 == 0,
 *                sw % 16 == 0 is read 16 bytes at a time: NCHW, and NHWC with C == 3)
 *   code_table : int8 [C][256], C <= 16 (held in LDS), any alignment
 *   codes      : as qvit_im2col_quant_i8: columns [C*kh*kw, kpad) zero, columns [kpad, ldc) never touched; a tap
 *                outside the image gives code 0 (padding comes after normalisation, as in the reference).
 * Checks, in this order: a NULL img, code_table or codes (QVIT_ENULL); layout (QVIT_EINVAL); the geometry, by the
 * rules of qvit_im2col_quant_i8 (QVIT_EINVAL); C > 16 (QVIT_EINVAL); kpad < C*kh*kw, kpad % 16, ldc < kpad
 * (QVIT_EINVAL); ldc % 16 or codes off 16 bytes (QVIT_EALIGN); B == 0 returns QVIT_OK without a launch.
 */
int qvit_im2col_u8_i8(const uint8_t* img, int64_t B, int64_t C, int64_t H, int64_t W, int layout,
                      int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                      const int8_t* code_table, int8_t* codes, int64_t ldc, int64_t kpad, hipStream_t stream);

/*
 * out[b][c][y][x] = value_table[c][img(b, c, y, x)]: the normalised fp32 NCHW image of a uint8 one, for the routes
 * that read fp32 (transforms.ToTensor + transforms.Normalize, predict.py:18-19, as a lookup).
 *   img         : as above, either layout, any alignment
 *   value_table : fp32 [C][256], C <= 16 (held in LDS)
 *   out         : fp32 [B][C][H][W] contiguous
 * Checks, in this order: a NULL pointer (QVIT_ENULL); layout, B < 0, C, H or W < 1, B, H or W > 2^20, C > 16
 * (QVIT_EINVAL); value_table or out off 4 bytes (QVIT_EALIGN); B == 0 returns QVIT_OK without a launch.
 */
int qvit_u8_normalize_f32(const uint8_t* img, int64_t B, int64_t C, int64_t H, int64_t W, int layout,
                          const float* value_table, float* out, hipStream_t stream);

/*
 * LayerNorm (biased variance, eps) followed by the next layer's activation quantizer.
 *   x : fp32 [rows][ldx] (D = cols), gamma/beta fp32 [cols] (may be NULL -> 1 / 0)
 *   codes : int8 [rows][ldc], columns [cols, kpad) zero; 4-byte aligned, ldc % 4 == 0. Columns [kpad, ldc) and x
 *            columns [cols, ldx) are never touched. Any ldx and any alignment of x / gamma / beta is accepted (rows
 *            with cols % 4, ldx % 4 or a base off 16 bytes take a scalar kernel, as do cols > 2048).
 *   code_table : nullable, 16-B aligned; a qvit_epi_table_build table (QVIT_EPI_I8 semantics) of the
 *            same quantizer, used only if valid and <= 2046 buckets (results never depend on it).
 * Special values: a NaN or +-Inf anywhere in a row makes the row's mean, and with it every y of the row, NaN: all
 * `cols` codes of that row are 0 (its padding stays 0), on every kernel arm, with and without the code table, and in
 * the T32 order. Every other row is bit-identical to what it is without the special value (a workgroup holds four
 * rows; nothing is shared between them).
 */
int qvit_layernorm_quant_i8(const float* x, int64_t rows, int64_t cols, int64_t ldx,
                            const float* gamma, const float* beta, float eps,
                            int qtype, const float* d_quant, const float* q_m,
                            const float* t_quant, int levels,
                            int8_t* codes, int64_t ldc, int64_t kpad,
                            const void* code_table, hipStream_t stream);

/*
 * Quantized contraction C = epilogue(A_codes @ W_codes^T).
 *   A      : int8 codes [M][lda], K valid columns; K % QVIT_TILE_K == 0 (and K <= 65536 for QVIT_W4), lda % 16 == 0,
 *            A 16-byte aligned, columns past the true in-features must be 0 (the quantizers
 *            above write them so).
 *   Wp     : packed weights from qvit_pack_weight (wfmt, npad rows, kpad == K), or with wfmt QVIT_W4R the
 *            qvit_pack_weight_w4r image of a QVIT_W4 one (same results).
 *   N      : true out features (<= npad); outputs for n >= N are not written.
 *   d_act, d_wt : device float[1] scales; bias : device float[npad] (padded) or NULL.
 *   C      : fp32 / int8 / int32 [M][ldc] per epilogue; ldc % 4 == 0 (fp32/int32), % 16 (int8).
 *   For QVIT_EPI_I8*: the next layer's quantizer (out_qtype, out_d, out_qm, out_t, out_levels) and an
 *   optional code table (qvit_epi_table_build, NULL -> per-element evaluation).
 * Special values: the activations are codes, so a NaN or Inf enters through bias[n] or (QVIT_EPI_F32_RESID) C[m][n].
 * A bias entry changes its own column only: QVIT_EPI_F32 / _RESID write NaN, +Inf, -Inf there; QVIT_EPI_I8 writes 0,
 * L, -L and QVIT_EPI_I8_GELU 0, L, 0 (GELU(-Inf) is NaN), the same for QVIT_W4, W8, W4R and W8R and with or without the
 * code table. A NaN in C[m][n] stays that one element.
 */
int qvit_gemm(const int8_t* A, int64_t M, int64_t K, int64_t lda,
              const void* Wp, int wfmt, int64_t N, int64_t npad,
              const float* d_act, const float* d_wt, const float* bias,
              int epilogue, void* C, int64_t ldc,
              int out_qtype, const float* out_d, const float* out_qm, const float* out_t,
              int out_levels, const void* epi_table, hipStream_t stream);

/*
 * QVIT_ACT_T32: activation codes in the operand order of the int8 32x32x32 matrix instruction, the input of
 * qvit_gemm_a32. An [M][kpad] code matrix (kpad % 64 == 0) is stored as 1-KiB blocks of 32 rows x 32 columns,
 * block (r / 32, c / 32) at byte (r / 32 * kpad / 32 + c / 32) * 1024; inside it, 16-byte group
 * (r % 32) + 32 * ((c / 16) % 2) holds columns c - c % 16 .. + 15 of row r. Buffers hold ceil(M / 64) * 64 rows
 * (rows past M are never stored).
 *
 * qvit_layernorm_quant_i8_t32: qvit_layernorm_quant_i8 (vit_model.py:206-207 norm2 + the fc1 layer's quantize_act,
 *   quant_layers.py:356-381) with the codes written in QVIT_ACT_T32 order: cols % 4 == 0, cols <= 1024,
 *   kpad % 64 == 0, x / gamma / beta / codes 16-byte aligned. Same codes as qvit_layernorm_quant_i8, byte for byte.
 * qvit_gemm_a32: qvit_gemm with the activations in QVIT_ACT_T32 order, for the int8-code epilogues of Mlp.fc1
 *   (quant_layers.py:495-499 under vit_model.py:172: GELU + fc2's quantizer): a weight-stationary schedule (each
 *   CU holds one 96-row panel of the int4 weights in LDS for the whole launch) on int8 32x32x32 MFMA. Same codes
 *   as qvit_gemm on the row-major codes, byte for byte. Shapes: qvit_gemm_a32_fits (wfmt QVIT_W4, epilogue
 *   QVIT_EPI_I8 / QVIT_EPI_I8_GELU, N == npad == 3072, K == 768 or 1024) returns 1, else the call is QVIT_EINVAL.
 *   C: int8 [M][ldc], ldc % 16 == 0, 16-byte aligned.
 * Special values: qvit_layernorm_quant_i8_t32 as qvit_layernorm_quant_i8 (a poisoned row: all codes 0), qvit_gemm_a32 as
 * qvit_gemm (a bias entry changes its column only; same codes direct and tabled).
 */
int qvit_layernorm_quant_i8_t32(const float* x, int64_t rows, int64_t cols, int64_t ldx, const float* gamma,
                                const float* beta, float eps, int qtype, const float* d_quant, const float* q_m,
                                const float* t_quant, int levels, int8_t* codes, int64_t kpad,
                                const void* code_table, hipStream_t stream);
int qvit_gemm_a32_fits(int64_t K, int wfmt, int64_t N, int64_t npad, int epilogue);
int qvit_gemm_a32(const int8_t* A, int64_t M, int64_t K, const void* Wp, int wfmt, int64_t N, int64_t npad,
                  const float* d_act, const float* d_wt, const float* bias, int epilogue, void* C, int64_t ldc,
                  int out_qtype, const float* out_d, const float* out_qm, const float* out_t, int out_levels,
                  const void* epi_table, hipStream_t stream);

/*
 * Weight-only QuantizeLinear.forward (quant_layers.py:495-499, quant_mode WEIGHT_ONLY: quantize_act is the
 * identity, :356-358): Y[m, n] = d_wt * sum_k X[m, k] k_w[n, k] + bias[n] with fp32 X.
 *   X      : fp32 [M][ldx], K valid columns; K % QVIT_TILE_K == 0 (pad X with zero columns to the packed
 *            kpad), ldx % 4 == 0, X 16-byte aligned.
 *   Wp     : packed weights from qvit_pack_weight (wfmt QVIT_W4 / QVIT_W8, npad rows, kpad == K), or QVIT_W16 /
 *            QVIT_W24: the QVIT_W8 images of the balanced base-256 digits back to back (levels beyond int8).
 *   d_wt   : device float[1]; bias : device float[npad] (padded) or NULL.
 *   Y      : fp32 [M][ldy], ldy % 4 == 0, 16-byte aligned; outputs for n >= N are not written.
 *   workspace : optional device buffer (16-byte aligned, workspace_bytes long) for small M: with fewer tiles
 *            than half the CUs the K range is split over several workgroups whose fp32 partials
 *            (splits * M * npad floats) are then summed in a fixed order; NULL -> no split.
 * fp32-GEMM accuracy: X is split into three bf16 terms whose sum is X exactly, every product with a code is
 * exact in fp32, accumulation is fp32 (the order of the K-term sum differs from the reference's GEMM).
 * Special values: a NaN or Inf in X[m][k] changes row m of Y only, with or without the split-K workspace (the
 * partials are per row); a NaN makes Y[m][n] NaN for every n, as the exact product does (NaN * 0 is NaN). What an Inf
 * leaves in its row is not defined (the bf16 split of Inf has NaN terms).
 */
int qvit_gemm_wonly(const float* X, int64_t M, int64_t K, int64_t ldx, const void* Wp, int wfmt,
                    int64_t N, int64_t npad, const float* d_wt, const float* bias, float* Y, int64_t ldy,
                    float* workspace, int64_t workspace_bytes, hipStream_t stream);

/*
 * The backward GEMMs of QuantizeLinear (what autograd runs behind quant_layers.py:499's F.linear, with G the
 * gradient of the layer's output):
 *   dgrad  grad_xq[m, k] = sum_n G[m, n] (d_wt k_w[n, k])  is qvit_gemm_wonly itself: X = G (zero columns up to
 *          the image's reduction padding), Wp = the qvit_pack_weight image of the TRANSPOSED codes (rows = the
 *          layer's in-features, reduction = its out-features), bias = NULL. No new entry point.
 *   wgrad  dW[n, k] = d_act * sum_m G[m, n] A[m, k]  (qvit_gemm_wgrad), A the int8 activation codes the forward
 *          contracted (qvit_quantize_act_i8: x_q = d_act A), dW in the layout of nn.Linear.weight.grad.
 *   G      : fp32 [M][ldg], N valid columns; ldg % 4 == 0, 16-byte aligned.
 *   A      : int8 [M][lda], K valid columns, |code| <= 127; lda % 16 == 0, 16-byte aligned. Columns [K, lda) are
 *            padding: whatever they hold never reaches dW.
 *   d_act  : device float[1].
 *   dW     : fp32 [N][ldw], ldw >= K (any 4-byte aligned pointer and any ldw); columns [K, ldw) are not written.
 *   workspace : qvit_gemm_wgrad_workspace_bytes(M, N, K) bytes, 16-byte aligned, contents irrelevant. The M range
 *            is split over s = max(1, min(16, ceil(M / 32), ceil(512 / tiles))) workgroups per output tile (tiles =
 *            ceil(N / 128) ceil(K / 128)); their fp32 partials (s tiles of 128 x 128 each) are summed in ascending
 *            split order by a second launch: no atomics, the same call gives the same bits. The query returns
 *            s * 128 ceil(N / 128) * 128 ceil(K / 128) * 4: non-decreasing in M, at most 16 times the padded
 *            output and at most (tiles + 511) * 64 KiB (Mlp.fc1 of ViT-B: 4 N K 4 bytes).
 * Any M >= 0, N >= 1, K >= 1 (M <= 2^30, N, K <= 2^24, tiles <= 2^24; else QVIT_EINVAL, also from the query);
 * misaligned G / A / workspace or ldg / lda: QVIT_EALIGN (callers pad a copy). Rows m >= M contribute zero. M == 0
 * writes zeros.
 * fp32-GEMM accuracy, as qvit_gemm_wonly: G is split into three bf16 terms whose sum is G exactly, every product
 * with a code (7 significant bits) is exact in fp32, accumulation is fp32 on v_mfma_f32_16x16x32_bf16, one multiply
 * by d_act ends it. A NaN / inf in G[m][n] leaves row n of dW NaN and no other row.
 */
int64_t qvit_gemm_wgrad_workspace_bytes(int64_t M, int64_t N, int64_t K);
int qvit_gemm_wgrad(const float* G, int64_t M, int64_t N, int64_t ldg, const int8_t* A, int64_t K, int64_t lda,
                    const float* d_act, float* dW, int64_t ldw, void* workspace, int64_t workspace_bytes,
                    hipStream_t stream);

/*
 * The backward GEMMs of QuantizeConv2d on the integer path are those of QuantizeLinear over the patch rows the
 * forward contracted (qvit_im2col_quant_i8 + qvit_gemm): M = B OH OW rows of K = C kh kw columns.
 *   wgrad  qvit_gemm_wgrad on G2 (the [M][N] row view of the output gradient) and the im2col codes, which
 *          qvit_im2col_quant_i8 recomputes; dW [N][K] is nn.Conv2d.weight.grad's layout. No new entry point.
 *   dgrad  P = G2 (d_wt k_w) on qvit_gemm_wonly as for QuantizeLinear, then qvit_col2im_quant_backward: the adjoint
 *          of im2col (col2im) and the backward of quantize_act in one pass over the image,
 *            grad_xq[b][c][y][x] = sum over ky ascending, inside it kx ascending, with
 *                                  (y + ph - ky dh) % sh == 0, oy = (y + ph - ky dh) / sh in [0, OH) (x axis alike)
 *                                  of P[(b OH + oy) OW + ox][(c kh + ky) kw + kx],
 *          then (grad_x, grad_scalars) exactly as qvit_quant_backward gives them for (x, grad_out = grad_xq), dge_k 0.
 *   P      : fp32 [M][ldp], K valid columns in the order of qvit_im2col_quant_i8; columns [K, ldp) are never read.
 *   x      : fp32 NCHW [B][C][H][W] contiguous, the layer's input; NULL selects the fold-only mode: grad_x receives
 *            grad_xq itself, and qtype, the quantizer scalars, the clip values, grad_scalars and the workspace are
 *            not looked at (all may be 0 / NULL). For layers without an activation quantizer.
 *   grad_x : fp32 NCHW [B][C][H][W] contiguous. Must not alias P (an element is written while other threads still
 *            read rows of P) nor x.
 *   grad_scalars : float[3] as qvit_quant_backward. workspace: qvit_col2im_quant_backward_workspace_bytes(...)
 *            bytes, 8-byte aligned, contents irrelevant (one partial per workgroup, at most 1024, folded in a fixed
 *            order by a second launch).
 * A gather: every image element adds its own taps in the order above in fp32, starting from 0. No atomics, two
 * calls give the same bits; an element that no output position reads is exactly 0; a tap on the zero padding has no
 * image element and contributes nothing. A NaN in P reaches the elements that tap it (where the clip lets grad_out
 * through) and the sums.
 * Arms (the same bits wherever both apply): groups of four consecutive x read one 16-byte chunk of a row of P per
 * ky tap when pw == 0, dw == 1, kw % 4 == 0, sw % 4 == 0, sw >= kw, W % 4 == 0, ldp % 4 == 0 and P, x, grad_x are
 * 16-byte aligned (the patch embedding: k == s, p == 0); otherwise one element per thread, any geometry, any 4-byte
 * aligned pointers. Offsets are 32-bit while M ldp < 2^31 and B C H W < 2^31, else 64-bit.
 * Sizes: groups == 1, zero padding; B, C <= 2^20; H, W, sh, sw, ph, pw <= 2^16; kh, kw, dh, dw <= 1024; K <= 2^24;
 * K <= ldp <= 2^24; B C H W, M and M ldp < 2^40; else QVIT_EINVAL (the geometry and the image totals also from the
 * query). B == 0 writes three zeros (nothing in the fold-only mode).
 * Order of the checks: NULL (P, grad_x; with x also grad_scalars, d_quant, q_m, workspace); with x the qtype
 * (QVIT_EINVAL), then t_quant for the nonlinear quantizer (QVIT_ENULL); the upper bounds, the geometry
 * (qvit_im2col_quant_i8's rules) and the totals, then ldp (QVIT_EINVAL); with x the workspace size (QVIT_EINVAL);
 * 4-byte alignment of P, x, grad_x and 8-byte alignment of the workspace (QVIT_EALIGN).
 */
int64_t qvit_col2im_quant_backward_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int kh, int kw,
                                                   int sh, int sw, int ph, int pw, int dh, int dw);
int qvit_col2im_quant_backward(const float* P, int64_t ldp, const float* x, int64_t B, int64_t C, int64_t H,
                               int64_t W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int qtype,
                               const float* d_quant, const float* q_m, const float* t_quant, float clip_lo,
                               float clip_hi, float* grad_x, float* grad_scalars /* [3] */, void* workspace,
                               int64_t workspace_bytes, hipStream_t stream);

/*
 * Weight-only convolution (QuantizeConv2d.forward, quant_layers.py:575-587, quant_mode WEIGHT_ONLY; UltraNet's
 * Conv2d_Q.forward, quant_ultra.py:85-89, whose quantize_fn values are k / (2^(w_bit-1) - 1)):
 *   Y[b][n][oy][ox] = d_wt * sum_{c,ky,kx} X[b][c][oy sh - ph + ky dh][ox sw - pw + kx dw] k_w[n][(c kh + ky) kw + kx]
 *                     + bias[n]   (zero padding; groups = 1)
 *   X      : fp32 NCHW [B][C][H][W], contiguous (any alignment).
 *   Wp     : qvit_pack_weight image of the codes [N][C kh kw] in the weight's flattening order (npad rows, kpad
 *            == K >= C kh kw columns, K % QVIT_TILE_K == 0); wfmt as qvit_gemm_wonly.
 *   d_wt, bias : as qvit_gemm_wonly.
 *   Y      : fp32 NCHW [B][N][OH][OW] contiguous, OH = (H + 2 ph - dh (kh - 1) - 1) / sh + 1 (OW alike).
 *   workspace : as qvit_gemm_wonly (split K for few output pixels).
 * The patch rows are never materialised: the kernel gathers them from X stage by stage. Same arithmetic as
 * qvit_gemm_wonly on the patch matrix.
 */
int qvit_conv_wonly(const float* X, int64_t B, int64_t C, int64_t H, int64_t W, int kh, int kw, int sh, int sw,
                    int ph, int pw, int dh, int dw, const void* Wp, int wfmt, int64_t N, int64_t npad, int64_t K,
                    const float* d_wt, const float* bias, float* Y, float* workspace, int64_t workspace_bytes,
                    hipStream_t stream);
/* N <= 64 output channels with QVIT_W4 / QVIT_W8 codes whose first ceil(C kh kw / 64) stages of 16 ceil(N / 16)
 * rows take at most 24 KiB (and C kh kw <= 1024, H, W < 32767) run the narrow schedule: weights and a tap-offset
 * table LDS-resident, every wave on its own 16-pixel tiles, no workspace used; bit-identical to the wide one.
 * qvit_conv_wonly_narrow(0 / 1) turns it off / on for the process (-1: query); returns the previous setting. */
int qvit_conv_wonly_narrow(int enable);

/*
 * Conv2d_Q -> BatchNorm2d (eval, running statistics) -> activation_quantize_fn in one launch (UltraNet's blocks,
 * reference mymodel.py:71-124 run module by module; quant_ultra.py:59-73, :76-91):
 *   Y = round(clamp(fma(y, bn_alpha[n], bn_shift[n]), 0, 1) * a_levels) / a_levels,  y = qvit_conv_wonly's value
 *   (one fused multiply-add with the fold qvit_ultra_bn_fold computes; IEEE division by a_levels = 2^a_bit - 1).
 *   Arguments as qvit_conv_wonly; bn_alpha, bn_shift: device float[N]; 1 <= a_levels <= 127.
 * Only for layers on the narrow schedule (QVIT_EINVAL otherwise: run the modules one by one).
 */
int qvit_conv_wonly_bn_act(const float* X, int64_t B, int64_t C, int64_t H, int64_t W, int kh, int kw, int sh,
                           int sw, int ph, int pw, int dh, int dw, const void* Wp, int wfmt, int64_t N, int64_t npad,
                           int64_t K, const float* d_wt, const float* bias, const float* bn_alpha,
                           const float* bn_shift, int a_levels, float* Y, hipStream_t stream);

/*
 * The residual contraction of a transformer block with the next LayerNorm behind it, in one launch:
 * replaces QuantizeLinear.forward of Attention.proj / Mlp.fc2 (quant_layers.py:495-499) + the residual add of
 * Block.forward (reference vit_model.py:202-208) + the following norm2 / next block's norm1 (vit_model.py:193,
 * 206-207) + the next layer's quantize_act (quant_layers.py:356-381), i.e. qvit_gemm(QVIT_EPI_F32_RESID) then
 * qvit_layernorm_quant_i8 on the same rows, with the same results.
 *   A .. ldc : as qvit_gemm with QVIT_EPI_F32_RESID (C += d_act d_wt acc + bias); N % 4 == 0, N <= 1024,
 *              M * ldc * 4 < 2^31.
 *   gamma, beta, eps, out_* , ln_table : the LayerNorm and the next quantizer, as qvit_layernorm_quant_i8
 *              (ln_table: its QVIT_EPI_I8 code table, nullable; used if valid and <= 2174 buckets).
 *   codes    : int8 [M][ldcodes], the LayerNorm codes of the updated rows, columns [N, kpad_codes) zero.
 *   counters : int32 [ceil(M / 128)] (one per 128-row block), scratch: the call zeroes it on `stream` before
 *              the launch, so no state carries over between launches; it must not be shared with a launch
 *              running concurrently on another stream.
 * The last of a row block's npad / 256 workgroups runs the LayerNorm of its rows; the residual rows are written
 * through (sc1) and read back with sc1 loads behind an agent-scope counter.
 * Special values: a NaN in C[m][n] (or a bias column) stays where qvit_gemm(QVIT_EPI_F32_RESID) leaves it, and row m's
 * codes are the poisoned-row codes of qvit_layernorm_quant_i8 (all 0), with and without ln_table. Every other row of C
 * and of the codes is bit-identical: the hand-off between workgroups is per 128-row block and carries no values.
 */
int qvit_gemm_resid_ln(const int8_t* A, int64_t M, int64_t K, int64_t lda, const void* Wp, int wfmt,
                       int64_t N, int64_t npad, const float* d_act, const float* d_wt, const float* bias,
                       float* C, int64_t ldc, const float* gamma, const float* beta, float eps,
                       int out_qtype, const float* out_d, const float* out_qm, const float* out_t,
                       int out_levels, const void* ln_table, int8_t* codes, int64_t ldcodes,
                       int64_t kpad_codes, int32_t* counters, hipStream_t stream);

/*
 * Code table for the int8 epilogues (optional `epi_table` of qvit_gemm; 16-byte aligned,
 * QVIT_EPI_TABLE_BYTES(nb) bytes). The output code of QVIT_EPI_I8 / QVIT_EPI_I8_GELU is a piecewise
 * constant function of the pre-activation v = d_act d_wt acc + bias; the table holds it exactly over
 * nb uniform buckets of width w starting at v_lo (w must be below the smallest distance between two
 * of its change points, and the function constant beyond both ends). The device builds it by bisection
 * with the epilogue's own arithmetic and validates it; qvit_gemm uses it only if valid (else the
 * Bucket j holds the v with rne((v - v_lo) / w) == j, clamped to [0, nb - 1]; a NaN reads bucket 0. Bucket 0 must hold a
 * single code (start the range a bucket below the first change point): its spare byte then carries the direct path's
 * code of a NaN (0). A table whose bucket 0 has a change point is invalid.
 * direct per-element evaluation runs), so results never depend on the choice of (v_lo, w, nb).
 */
#define QVIT_EPI_TABLE_MAX_NB 3800
#define QVIT_EPI_TABLE_BYTES(nb) ((16 + 8 * (nb) + 1023) / 1024 * 1024)  /* staged in 1-KiB pieces */
int qvit_epi_table_build(int epilogue, int out_qtype, const float* out_d, const float* out_qm,
                         const float* out_t, int out_levels, float v_lo, float w, int64_t nb,
                         void* table, hipStream_t stream);

/*
 * Attention core between the qkv and proj QuantizeLinear layers of Attention.forward
 * (reference vit_model.py:133-149): out = softmax((q @ k^T) * scale) @ v per (image, head),
 * written as [B*N][ldo] with column h*head_dim + d (the reference's transpose(1, 2).reshape).
 *   qkv      : fp32 [B*N][ldq], row = [q | k | v], each H*head_dim wide (qkv.reshape(B,N,3,H,hd)).
 *   head_dim : 64, or 80 with QVIT_ATT_F32 (80 with QVIT_ATT_I8, or any other size: QVIT_EINVAL);
 *              ldq >= 3 H head_dim, ldo >= H head_dim. scale: qk_scale (head_dim ** -0.5 by default).
 *   in_scale : power of two applied to q, k, v before their fp16 hi/lo split (keeps |x * in_scale|
 *              < 65504; undone exactly), 1.0 for ordinary activations.
 *   out_mode : QVIT_ATT_F32 -> fp32 out (ldo % 4 == 0, 16-B aligned);
 *              QVIT_ATT_I8  -> int8 codes of the next layer's activation quantizer
 *              (out_qtype, out_d, out_qm, out_t, out_levels as in qvit_gemm), ldo % 4 == 0.
 * fp32 matmuls are formed from fp16 hi/lo products with fp32 accumulation (~2^-22 relative error).
 * Special values (qvit_attention and qvit_attention_split): a NaN or Inf in q, k or v of one (image, head) changes the
 * outputs of that (image, head) only; every other block is bit-identical. A NaN in q[i] makes out[i][:] of the block
 * NaN, a NaN in v[j][d] makes out[:][d] of the block NaN, exactly where the exact product is NaN. What +-Inf leaves
 * inside its block is not defined (inf - inf in the softmax). QVIT_ATT_I8: a NaN output has code 0, direct and
 * through the code table alike.
 */
/*
 * UltraNet (reference `4-bit quantization/`: quant_ultra.py:8-91, mymodel.py:23-144).
 * Weight codes k_w = rne(tanh(w)/max|tanh(w)| * (2^(w_bit-1)-1)) (weight_quantize_fn, quant_ultra.py:30-56),
 * activation codes k_a = rne(clamp(x,0,1) * (2^a_bit-1)) (activation_quantize_fn :59-73), so a
 * Conv2d_Q on codes is the int32 contraction acc with value acc / den, den = (2^(w_bit-1)-1)(2^a_bit-1).
 *
 * qvit_ultra_weight_codes: w fp32 [cout][cin][ks][ks] -> codes int8 [cout_pad][kpad] in K order
 *   (ky, kx, c), zero padded; values (nullable) = the reference's fake-quant weight k_w/(2^(w_bit-1)-1)
 *   in w's own layout; workspace = device unsigned[1] (max |tanh| scratch).
 * qvit_ultra_bn_fold: BatchNorm2d eval constants alpha = gamma/sqrt(var+eps), shift = beta - mean*alpha.
 * qvit_ultra_conv0: layer 0 (mymodel.py:73-77): float image NCHW [B][3][H][W] -> conv 3x3 pad 1 with the
 *   fake-quant weights (wvals [16][3][3][3], the `values` output of qvit_ultra_weight_codes)
 *   -> BN (alpha, shift) -> activation quantizer -> MaxPool2d(2,2);
 *   out = codes NHWC [B][H/2][W/2][16], 16-byte aligned.
 * qvit_ultra_conv: layers 1..8: in = codes NHWC [B][H][W][cin] (16-B aligned), ks in {1, 3} (pad ks/2),
 *   wcodes [round_up(cout,16)][kpad] from qvit_ultra_weight_codes; mode QVIT_ULTRA_* ; out NHWC with
 *   row (pixel) pitch ldo: codes (ldo % 4 == 0) or fp32 (the 1x1 head, shift = its bias).
 *   Supported (cin, ks, cout): (16,3,17..32), (32,3,49..64), (64,3,49..64), (64,1,33..48).
 * qvit_yolo_decode: YOLOLayer eval decode (mymodel.py:47-60) of the head output NHWC [B][ny][nx][ldh]
 *   (channel a*no + o) with anchors (device float [na][2]) and stride -> io and p, both
 *   [B][na][ny][nx][no] (io.view(bs, -1, no) is the reference's first output).
 */
int qvit_ultra_weight_codes(const float* w, int64_t cout, int64_t cin, int64_t ks, int w_bit,
                            int8_t* codes, int64_t kpad, int64_t cout_pad, float* values,
                            unsigned* workspace, hipStream_t stream);
int qvit_ultra_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var,
                       float eps, int64_t n, float* alpha, float* shift, hipStream_t stream);
int qvit_ultra_conv0(const float* img, int64_t B, int64_t H, int64_t W, const float* wvals,
                     const float* alpha, const float* shift, int a_bit, int8_t* out, hipStream_t stream);
int qvit_ultra_conv(const int8_t* in, int64_t B, int64_t H, int64_t W, int64_t cin, int64_t ks,
                    const int8_t* wcodes, int64_t kpad, int64_t cout, int w_bit, int a_bit,
                    const float* alpha, const float* shift, int mode, void* out, int64_t ldo,
                    hipStream_t stream);
/*
 * qvit_ultra_tail: UltraNetQua.layers.16-28 (mymodel.py:104-124: four Conv2d_Q 64 -> 64 3x3 + BatchNorm2d +
 *   activation_quantize_fn blocks, then the 1x1 Conv2d_Q head with bias) in one launch, one workgroup per image
 *   with the maps resident in LDS. Same results as qvit_ultra_conv(QVIT_ULTRA_CODES) four times and
 *   qvit_ultra_conv(QVIT_ULTRA_F32) once, bit for bit.
 *   in      : codes NHWC [B][H][W][64], H, W <= 26 (UltraNet @416: 26 x 26), 16-byte aligned.
 *   wcodes, alpha, shift : HOST arrays of 4 device pointers (layers 4..7): weight codes [64][kpad] in K order
 *             (ky, kx, c) (qvit_ultra_weight_codes, kpad >= 576, % 16), BN alpha / shift [64] (qvit_ultra_bn_fold).
 *   hcodes  : head codes [48][hkpad] (hkpad >= 64); hbias device float[hout], hout <= 48.
 *   out     : fp32 NHWC [B][H][W][ldo], channels < hout written (io == NULL), or
 *   anchors, na, no, stride, io, p : with io != NULL the YOLOLayer decode of qvit_yolo_decode is applied in the
 *             kernel instead (hout == na * no; io, p [B][na][H][W][no]; out unused and may be NULL).
 */
int qvit_ultra_tail(const int8_t* in, int64_t B, int64_t H, int64_t W, const int8_t* const* wcodes, int64_t kpad,
                    const float* const* alpha, const float* const* shift, const int8_t* hcodes, int64_t hkpad,
                    const float* hbias, int64_t hout, int w_bit, int a_bit, float* out, int64_t ldo,
                    const float* anchors, int64_t na, int64_t no, float stride, float* io, float* p,
                    hipStream_t stream);

/*
 * UltraNet training: the straight-through backward of quant_ultra.py's quantizers (uniform_quantize.backward,
 * quant_ultra.py:23-25, hands the gradient through the rounding unchanged) and Conv2d_Q's weight gradient.
 *
 * qvit_ultra_weight_quant_backward: backward of weight_quantize_fn.forward, 2 <= w_bit <= 8 (quant_ultra.py:50-55:
 *   weight = tanh(x); weight = weight / max|weight|; weight_q = uniform_q(weight)). With t = tanh(w), m = max|t|:
 *     g_t = g / m - sgn(t) [|t| == m] (sum_i g_i t_i) / (m^2 c),   grad_w = g_t (1 - t^2),
 *   c the number of elements attaining the maximum (torch's full-reduction max spreads its gradient evenly over
 *   ties). t and m come from the device routines qvit_ultra_weight_codes uses, so the tie set is the forward's.
 *   w, grad_out, grad_w : device float[n] (4-byte aligned; grad_w may be grad_out).
 *   workspace : qvit_ultra_weight_quant_backward_workspace_bytes(n) bytes (16 + 16 per workgroup, at most 1024
 *               workgroups), 8-byte aligned, contents irrelevant. The query returns QVIT_EINVAL for n < 0.
 *   The sum and the count take per-thread double accumulation, a fixed-order wave / block tree, one partial per
 *   workgroup and a one-block fold in index order: no float atomics, two calls give the same bits. Masks select: a
 *   NaN in grad_out[i] reaches grad_w[i] and, through the sum, every tied element. n == 0 does nothing.
 * qvit_ultra_act_quant_backward: backward of activation_quantize_fn.forward (quant_ultra.py:71,
 *   uniform_q(clamp(x, 0, 1))): grad_x = grad_out where 0 <= x <= 1 (both boundaries pass), else 0 (a NaN x: 0).
 *   x, grad_out, grad_x : device float[n], 16-byte aligned (QVIT_EALIGN otherwise); grad_x may be grad_out.
 * qvit_conv_wgrad: the weight gradient of Conv2d_Q.forward's F.conv2d (quant_ultra.py:85-89) with respect to the
 *   quantized weight, for an input that holds activation_quantize_fn values (quant_ultra.py:66-73):
 *     dW[n][c][ky][kx] = (1 / levels) sum_{b,oy,ox} G[b][n][oy][ox] k_x[b][c][oy sh - ph + ky dh][ox sw - pw + kx dw]
 *   G      : fp32 NCHW [B][N][OH][OW] contiguous, OH = (H + 2 ph - dh (kh - 1) - 1) / sh + 1 (OW alike).
 *   X      : fp32 NCHW [B][C][H][W] contiguous; the caller declares X = k_x / levels with integer 0 <= k_x <= levels
 *            (the quantizer's output, max-pooled or not). The kernel recovers k_x = rint(X levels).
 *   levels : 1 .. 127 (2^a_bit - 1).
 *   dW     : fp32 [N][C][kh][kw] contiguous, the layout of nn.Conv2d.weight.grad; nothing outside it is written.
 *   workspace : qvit_conv_wgrad_workspace_bytes(...) bytes, 16-byte aligned, contents irrelevant: the reduction
 *            range B OH OW is split over s = max(1, min(256, ceil(B OH OW / 32), ceil(2048 / tiles))) waves per
 *            64 x 64 output tile (tiles = ceil(N / 64) ceil(C kh kw / 64)); their fp32 partials (s 64 ceil(N / 64)
 *            64 ceil(C kh kw / 64) 4 bytes) are summed in ascending split order by a second launch. No atomics.
 *   Zero padding, groups == 1, any stride / padding / dilation; out-of-image taps contribute zero. B == 0 writes
 *   zeros. Sizes: C, H, W, N, strides, paddings, C kh kw <= 2^20, kh, kw, dh, dw <= 1024, OH OW <= 2^30,
 *   B OH OW < 2^31 - 64 and a non-empty output, else QVIT_EINVAL (also from the query); pointers 4-byte aligned
 *   (workspace 16), else QVIT_EALIGN.
 *   fp32-GEMM accuracy, as qvit_gemm_wgrad: G is split into three bf16 terms whose sum is G exactly, every product
 *   with a code is exact in fp32, accumulation is fp32 on v_mfma_f32_16x16x32_bf16, one multiply by 1 / levels ends
 *   it. A NaN / inf in G[b][n][.][.] leaves dW[n] NaN and no other output channel.
 * The input gradient needs no entry point: for stride 1 and p <= d (k - 1) it is qvit_conv_wonly with X = G, the
 * qvit_pack_weight image of the codes transposed (C rows) and flipped in (ky, kx), and padding d (k - 1) - p.
 */
int64_t qvit_ultra_weight_quant_backward_workspace_bytes(int64_t n);
int qvit_ultra_weight_quant_backward(const float* w, const float* grad_out, int64_t n, int w_bit, float* grad_w,
                                     void* workspace, int64_t workspace_bytes, hipStream_t stream);
int qvit_ultra_act_quant_backward(const float* x, const float* grad_out, int64_t n, float* grad_x,
                                  hipStream_t stream);
int64_t qvit_conv_wgrad_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int64_t N, int kh, int kw,
                                        int sh, int sw, int ph, int pw, int dh, int dw);
int qvit_conv_wgrad(const float* G, const float* X, int64_t B, int64_t C, int64_t H, int64_t W, int64_t N, int kh,
                    int kw, int sh, int sw, int ph, int pw, int dh, int dw, int levels, float* dW, void* workspace,
                    int64_t workspace_bytes, hipStream_t stream);
/*
 * UltraNet training: BatchNorm2d on batch statistics -> activation_quantize_fn (a_bit <= 7) -> optional
 * MaxPool2d(2, 2) (mymodel.py:71-124) over x fp32 NCHW [B][C][H][W] contiguous, M = B H W values per channel.
 * Common to the entry points below: B, C, H, W >= 1 and each < 2^31, H W <= 2^31 - 1 - 8192, B C < 2^31,
 * M >= 2, pool 0 or 1 and then H, W >= 2, and B C ceil(H W / 8192) < 2^31 (the grid), else QVIT_EINVAL (also from
 * the workspace queries); fp32 pointers 4-byte aligned, sums and workspaces 8, else QVIT_EALIGN. The 16-byte arm
 * runs when the tensors are 16-byte aligned (flag bytes: 4) and H W % 4 == 0 (pooled: W % 4 == 0), else a scalar
 * arm with the same results. Reductions: double accumulation per thread, a fixed-order wave / workgroup tree, one
 * partial pair per workgroup in the workspace (contents irrelevant), folded per channel in index order. No atomics:
 * two calls give the same bits.
 *
 * qvit_bn_stats: mean[c], var[c] (biased) and invstd[c] = 1 / sqrt(var + eps) (computed in double on data shifted
 *   by x[0][c][0][0], rounded once to fp32), and when the running pointers are not NULL nn.BatchNorm2d's update
 *   r = (1 - factor) r + factor new with new = mean, resp. var M / (M - 1); factor is the module's momentum or
 *   1 / num_batches_tracked. workspace: qvit_bn_stats_workspace_bytes(B, C, H, W) = 16 B C ceil(H W / 8192) bytes.
 * qvit_bn_act_pool_forward: a = gamma[c] invstd[c] (fp32; gamma NULL: 1), y = fmaf(x - mean[c], a, beta[c]) (beta
 *   NULL: 0), k = rint(clamp(y, 0, 1) levels) (a NaN y: 0), pass = 0 <= y <= 1 (both edges pass, a NaN fails: the
 *   mask of qvit_ultra_act_quant_backward). levels 1 .. 127.
 *   pool 0: out [B][C][H][W] = k / levels, flags [B][C][H][W] bytes = pass.
 *   pool 1: 2 x 2 windows, stride 2, floor mode (an odd last row / column is dropped): out [B][C][H/2][W/2] = the
 *     window's maximum k / levels; flags [B][C][H/2][W/2] = pass(winner) | winner << 1 with winner = 2 dy + dx of the
 *     FIRST maximum in row-major order (ATen's max pool: val > maxval), so equal codes select the top-left element.
 * qvit_bn_act_pool_backward_reduce: g_y = grad_out (shaped as out) at the element / the window's winner when its
 *   pass bit is set, else 0 (selected, never multiplied: a NaN grad_out behind a cleared bit is not read into a
 *   sum); sums[c] = S1 = sum g_y, sums[C + c] = S2 = sum g_y xhat, xhat = (x - mean) invstd. sums: double[2 C].
 *   workspace: qvit_bn_act_pool_backward_workspace_bytes(B, C, H, W, pool) bytes.
 * qvit_bn_act_pool_backward_dx: dx [B][C][H][W] = a (g_y - S1 / M - xhat S2 / M) at every element of x (pooled-away
 *   elements and dropped rows / columns have g_y = 0), dgamma[c] = S2 and dbeta[c] = S1 when those are not NULL.
 */
int64_t qvit_bn_stats_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W);
int qvit_bn_stats(const float* x, int64_t B, int64_t C, int64_t H, int64_t W, double eps, double factor,
                  float* running_mean, float* running_var, float* mean, float* var, float* invstd, void* workspace,
                  int64_t workspace_bytes, hipStream_t stream);
int qvit_bn_act_pool_forward(const float* x, int64_t B, int64_t C, int64_t H, int64_t W, const float* mean,
                             const float* invstd, const float* gamma, const float* beta, int levels, int pool,
                             float* out, uint8_t* flags, hipStream_t stream);
int64_t qvit_bn_act_pool_backward_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int pool);
int qvit_bn_act_pool_backward_reduce(const float* x, const float* grad_out, const uint8_t* flags, int64_t B,
                                     int64_t C, int64_t H, int64_t W, const float* mean, const float* invstd,
                                     int pool, double* sums, void* workspace, int64_t workspace_bytes,
                                     hipStream_t stream);
int qvit_bn_act_pool_backward_dx(const float* x, const float* grad_out, const uint8_t* flags, int64_t B, int64_t C,
                                 int64_t H, int64_t W, const float* mean, const float* invstd, const float* gamma,
                                 const double* sums, int pool, float* dx, float* dgamma, float* dbeta,
                                 hipStream_t stream);
/*
 * UltraNet integer deploy (reference `4-bit quantization/`: quantization.py:24-31,68-89,
 * qnn_param_reader.py:58-85, ultranet_param_gen.py:14-22 — the FPGA flow's integer parameters):
 *   code = clamp(round((acc * inc_q[o] + bias_q[o]) / 2^S), 0, 2^out_bit - 1), round half up, 64-bit
 *   intermediate, S = w_bit - 1 + in_bit + l_shift; inc_q / bias_q from bn_act_quantize_int (host side).
 *   Replaces the accelerator's conv + BN + activation stage (its HLS source is absent from the reference;
 *   the rounding shown is the float path's round(), restated in integers: parity unpinned beyond it).
 * qvit_ultra_conv0_int: layer 0 on uint8 pixels NCHW [B][3][H][W] (in_bit 8), weight codes [16][3][3][3]
 *   (reference layout, weight_quantize_int) -> 2x2 max-pooled codes NHWC [B][H/2][W/2][16] (16-B aligned).
 * qvit_ultra_conv_int: layers 1..7 as qvit_ultra_conv (same input / weight layouts and shapes, 3x3 only)
 *   with the integer threshold; pool != 0 adds MaxPool2d(2, 2) on the codes.
 */
int qvit_ultra_conv0_int(const uint8_t* img, int64_t B, int64_t H, int64_t W, const int8_t* wcodes,
                         const int32_t* inc, const int32_t* bias, int shift_bits, int out_bit, int8_t* out,
                         hipStream_t stream);
int qvit_ultra_conv_int(const int8_t* in, int64_t B, int64_t H, int64_t W, int64_t cin, int64_t ks,
                        const int8_t* wcodes, int64_t kpad, int64_t cout, const int32_t* inc, const int32_t* bias,
                        int shift_bits, int out_bit, int pool, int8_t* out, int64_t ldo, hipStream_t stream);
int qvit_yolo_decode(const float* head, int64_t B, int64_t ny, int64_t nx, int64_t na, int64_t no,
                     int64_t ldh, const float* anchors, float stride, float* io, float* p,
                     hipStream_t stream);

int qvit_attention(const float* qkv, int64_t B, int64_t N, int64_t H, int64_t head_dim, int64_t ldq,
                   float scale, float in_scale, int out_mode, void* out, int64_t ldo,
                   int out_qtype, const float* out_d, const float* out_qm, const float* out_t,
                   int out_levels, hipStream_t stream);

/*
 * Backward of qvit_attention with QVIT_ATT_F32 (the gradient torch autograd takes through vit_model.py:133-149):
 * with S = scale q k^T, P = softmax(S), O = P v and D_i = sum_c dO_ic O_ic,
 *   dv = P^T dO,  dS = P o (dO v^T - D),  dq = scale dS k,  dk = scale dS^T q.
 * S and P are recomputed per 32-row block on chip; nothing N x N reaches global memory.
 * With hd = head_dim:
 *   qkv      : fp32 [B N][ldq], the forward's input (q, k, v sections of H * hd columns); ldq >= 3 H hd
 *   out      : fp32 [B N][ldo], the forward's output O (required); ldo >= H hd
 *   grad_out : fp32 [B N][ldgo], dO; ldgo >= H hd
 *   grad_qkv : fp32 [B N][ldg], written in the layout of qkv (columns [0, 3 H hd) only); ldg >= 3 H hd
 *   in_scale : the forward's power of two (|qkv in_scale| <= 16384)
 *   g_scale  : a power of two with |grad_out g_scale| <= 16384, as close to it as the caller can make it (gradients
 *              of 1e-8 would flush in the fp16 operand split); undone exactly, so grad(a dO) = a grad(dO) bit for
 *              bit for a power of two a when g_scale follows max |dO|
 *   workspace: qvit_attention_backward_workspace_bytes(B, N, H) bytes (O(B H N): one log-sum-exp and one D per
 *              query, one bound per head), 16-byte aligned, caller-owned, no state carried between calls.
 * head_dim must be 64 or 80 (the workspace does not depend on it); every pointer 16-byte aligned and
 * every leading dimension a multiple of 4. Three launches
 * (row sums, query owner -> dq, key owner -> dk, dv), no float atomics: a call is bitwise reproducible.
 * qvit_attention_backward_workspace_bytes returns QVIT_EINVAL for N <= 0, H <= 0 or B < 0.
 */
int64_t qvit_attention_backward_workspace_bytes(int64_t B, int64_t N, int64_t H);
int qvit_attention_backward(const float* qkv, const float* out, const float* grad_out, int64_t B, int64_t N,
                            int64_t H, int64_t head_dim, int64_t ldq, int64_t ldo, int64_t ldgo, float scale,
                            float in_scale, float g_scale, float* grad_qkv, int64_t ldg, void* workspace,
                            int64_t workspace_bytes, hipStream_t stream);

/*
 * The qkv projection feeding qvit_attention_split (fused block path; replaces the fp32 qkv of
 * Attention.forward, vit_model.py:130-137, with the operand form the attention kernel consumes).
 * The value x = d_act d_wt acc + bias[n] is computed exactly as QVIT_EPI_F32 does, scaled by the power
 * of two in_scale and split into fp16 hi = f16(x s), lo = f16(x s - hi), stored head-major:
 *   qkv_hi / qkv_lo : fp16 [B][N / 64][seq][64], B = M / seq, plane p = n / 64 (q heads, k heads,
 *                     v heads), element (b, p, t, n % 64) for row m = b seq + t; 16-B aligned.
 * A, Wp, d_act, d_wt, bias as qvit_gemm; N % 64 == 0, M % seq == 0.
 */
int qvit_gemm_qkv_split(const int8_t* A, int64_t M, int64_t K, int64_t lda,
                        const void* Wp, int wfmt, int64_t N, int64_t npad,
                        const float* d_act, const float* d_wt, const float* bias,
                        int64_t seq, float in_scale, void* qkv_hi, void* qkv_lo, hipStream_t stream);

/*
 * qvit_gemm_qkv_split with the head width as an argument: planes fp16 [B][N / head_dim][seq][head_dim], plane
 * p = n / head_dim, element (b, p, t, n % head_dim); the same value arithmetic (x as QVIT_EPI_F32, hi = f16(x s),
 * lo = f16(x s - hi)). head_dim is 64 or 80 and N % head_dim == 0. At 64 the bytes are those of qvit_gemm_qkv_split;
 * at 80 a plane row is 160 B, so rows stay 16-B aligned.
 * Order of the checks (part of the ABI), the same list for both entry points, qvit_gemm_qkv_split with head_dim 64:
 * NULL pointers (QVIT_ENULL); wfmt; head_dim not 64 or 80; the sizes, N % head_dim among them; the seq / in_scale
 * rules; K of the 4-bit formats (all QVIT_EINVAL); then alignment (QVIT_EALIGN): lda and A / Wp, the planes, bias; then
 * M == 0 is QVIT_OK. So a bad head_dim wins over every seq and alignment rule and loses to NULL and wfmt.
 */
int qvit_gemm_qkv_split_hd(const int8_t* A, int64_t M, int64_t K, int64_t lda,
                           const void* Wp, int wfmt, int64_t N, int64_t npad,
                           const float* d_act, const float* d_wt, const float* bias,
                           int64_t seq, int64_t head_dim, float in_scale, void* qkv_hi, void* qkv_lo,
                           hipStream_t stream);

/*
 * qvit_attention on the split operands of qvit_gemm_qkv_split / qvit_gemm_qkv_split_hd (planes
 * [B][3H][N][head_dim], head_dim 64 or 80, in_scale the same power of two): identical arithmetic, bit for bit;
 * K/V blocks stream into LDS by DMA with no conversion. Both out modes at both widths (unlike qvit_attention, whose
 * int8 epilogue is for 64 only); ldo >= H * head_dim. Any other head_dim is QVIT_EINVAL, at the position the
 * head_dim != 64 check always had (after NULL and the table's alignment, before the sizes).
 * epi_table (QVIT_ATT_I8 only, nullable): a qvit_epi_table_build table with QVIT_EPI_I8 semantics for
 * the output quantizer (<= 2046 buckets; used only if valid, results never depend on it).
 */
int qvit_attention_split(const void* qkv_hi, const void* qkv_lo, int64_t B, int64_t N, int64_t H,
                         int64_t head_dim, float scale, float in_scale, int out_mode, void* out,
                         int64_t ldo, int out_qtype, const float* out_d, const float* out_qm,
                         const float* out_t, int out_levels, const void* epi_table, hipStream_t stream);

/*
 * Fused qkv projection + attention core (vit_model.py:130-152) for the fused block: the qkv
 * QuantizeLinear (qvit_gemm_qkv_split semantics: d_act d_wt acc + bias, scaled by in_scale, split to
 * fp16 hi/lo) and qvit_attention_split in one kernel, q/k/v never written to HBM.
 *   A    : activation codes [B*N][lda] (K valid columns, K % 256 == 0, K <= 65536), N <= 208 tokens, H*64 <= 768;
 *   Wp   : the qkv layer's packed int4 weights (qvit_pack_weight, wfmt QVIT_W4, npad rows), bias [npad];
 *   out  : as qvit_attention_split (QVIT_ATT_F32 / QVIT_ATT_I8 + optional code table epi_table).
 * The dims of each q.k sum are added in a different order than in qvit_attention_split (fp32-level
 * differences only).
 */
int qvit_qkv_attention(const int8_t* A, int64_t B, int64_t N, int64_t K, int64_t lda, const void* Wp,
                       int wfmt, int64_t npad, const float* d_act, const float* d_wt, const float* bias,
                       int64_t H, int64_t head_dim, float scale, float in_scale, int out_mode, void* out,
                       int64_t ldo, int out_qtype, const float* out_d, const float* out_qm,
                       const float* out_t, int out_levels, const void* epi_table, hipStream_t stream);

/*
 * qvit_qkv_attention for the first NQ tokens of each image only (the class / distillation token rows the
 * head of a classifier reads after the last block): K and V are projected for all N tokens, q and the
 * attention only for query tile 0, with the block body and key-block order the full kernel uses for it.
 *   NQ   : 1 <= NQ <= min(N, 32), else QVIT_EINVAL and nothing is launched;
 *   out  : compact [B*NQ][ldo]; row b*NQ + i equals, bit for bit, row b*N + i of what qvit_qkv_attention
 *          writes for the same arguments (both out modes, with and without epi_table). Columns >= H*64
 *          and every other row are not written.
 * Every other argument as qvit_qkv_attention.
 */
int qvit_qkv_attention_q(const int8_t* A, int64_t B, int64_t N, int64_t NQ, int64_t K, int64_t lda,
                         const void* Wp, int wfmt, int64_t npad, const float* d_act, const float* d_wt,
                         const float* bias, int64_t H, int64_t head_dim, float scale, float in_scale,
                         int out_mode, void* out, int64_t ldo, int out_qtype, const float* out_d,
                         const float* out_qm, const float* out_t, int out_levels, const void* epi_table,
                         hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* QVIT_HIP_H */
