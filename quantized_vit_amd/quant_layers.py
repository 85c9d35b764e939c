"""QuantizeLinear / QuantizeConv2d for MI355X: the reference's module surface, HIP underneath.

Mirrors OTO/quantization/quant_layers.py (OTO = QViT_with_GETA/only_train_once): same class
names, constructor arguments, parameter names / state_dict keys (weight, bias, d_quant_wt, q_m_wt,
[t_quant_wt], [d_quant_act, q_m_act, t_quant_act]), enums, from_module(), weight_bit /
activation_bit and LAYER_TO_QUANTLAYER, so model_to_quantize_model and existing callers
(vit_model.py:100,133,151,172,175,327) work unchanged.

What differs is how forward() computes (quant_layers.py:495-499, 575-587). The reference
re-quantizes the fp32 master weight on every call and runs an fp32 F.linear on fake-quant
operands. Here, on a ROCm device:
  * weights are quantized once per parameter version into int4 (|level| <= 7) or int8 codes,
    packed for the MFMA kernel (qvit_pack_weight), and cached;
  * activations are quantized to int8 codes by a HIP kernel (qvit_quantize_act_i8);
  * the product is an exact int32 MFMA contraction with the fp32 epilogue
    d_act * d_wt * acc + bias (qvit_gemm) — mathematically the reference's F.linear on
    d_a*k_a and d_w*k_w, differing only in fp32 rounding.
Layers whose levels do not fit int8 (e.g. the 16/32-bit initial states, weight-only mode) run
the reference's fake-quant values (HIP kernel qvit_fake_quant_f32) through the library fp32
GEMM instead. CPU tensors are rejected: the product has no CPU fallback.

Autograd: a layer called with gradients enabled, and an input or a parameter that requires grad, records
one autograd node around the very same forward (bit-identical output). Its backward runs the two GEMM
gradients (QuantizeLinear: on the integer codes, qvit_gemm_wonly on the transposed weight codes and
qvit_gemm_wgrad on the activation codes, see BACKWARD_GEMM; QuantizeConv2d: the same two kernels over the im2col
patch rows plus qvit_col2im_quant_backward, see CONV_BACKWARD_GEMM; otherwise torch's fp32 GEMM / convolution) and the
reference's quantizer backwards (quant_layers.py:71-125, 163-205) as
one fused HIP pass each (qvit_quant_backward): grad_x plus the gradients of d_quant, q_m and t_quant through
a deterministic reduction. SymQuantizerLinear / SymQuantizerNonLinear / DGEQuantizer expose the same pass at
the function level. Under torch.no_grad() nothing of this runs. The quantization stages of the GETA optimizer are qat_optim.py; its
pruning stages are out of scope.
"""
from __future__ import annotations

import logging
import math
import os
import warnings
from dataclasses import dataclass, field
from enum import Enum
from typing import Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

logger = logging.getLogger(__name__)


class NanInGradientError(Exception):
    """quant_layers.py:10-13: raised by a quantizer's backward when its gradient holds a NaN."""

    def __init__(self, message):
        self.message = message
        super().__init__(self.message)


class QuantizationType(Enum):
    """quant_layers.py:20-24."""
    SYMMETRIC_LINEAR = "symmetric+linear"
    SYMMETRIC_NONLINEAR = "symmetric+nonlinear"
    DGE = "dge"


class QuantizationMode(Enum):
    """quant_layers.py:27-29."""
    WEIGHT_ONLY = "weight_only"
    WEIGHT_AND_ACTIVATION = "weight_and_activation"


def _qtype_code(qt: QuantizationType) -> int:
    # DGEQuantizer.forward (quant_layers.py:217-246) is the linear quantizer's forward
    if qt in (QuantizationType.SYMMETRIC_LINEAR, QuantizationType.DGE):
        return _lib.QT_LINEAR
    if qt == QuantizationType.SYMMETRIC_NONLINEAR:
        return _lib.QT_NONLINEAR
    raise NotImplementedError(qt)


_warned_grad = False

# Parity instrumentation (tests): when CODE_TRACE is a dict, every int8 activation-code operand handed to
# a layer's contraction is recorded as CODE_TRACE[layer] = codes[:, :K] (a stream-ordered copy), so a
# checker can compare each quantizer boundary of a full forward with the reference's.
CODE_TRACE: Optional[dict] = None


def trace_codes(layer, codes: torch.Tensor, k: int) -> None:
    if CODE_TRACE is not None:
        CODE_TRACE[layer] = codes[:, :k].detach().clone()


def _warn_no_grad() -> None:
    global _warned_grad
    if not _warned_grad:
        _warned_grad = True
        warnings.warn("quantized_vit_amd: the HIP forward path records no autograd history "
                      "(inference only); run under torch.no_grad() to silence this warning.")


def _autograd_live(module: nn.Module, x: torch.Tensor) -> bool:
    """Whether a call of `module` on `x` has to record autograd history."""
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters()))


def _as_param_ptr(p: Optional[torch.Tensor], device: torch.device) -> Optional[torch.Tensor]:
    if p is None:
        return None
    t = p.detach()
    if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.float32).contiguous()
    return t


def saturation_level(qtype: int, d: float, q_m: float, t: float = 1.0) -> float:
    """Host copy of the device formula: rne(|q_m| / d) (linear, quant_layers.py:154,159) or
    rne(exp(t log(|q_m| + 1e-6)) / d) (nonlinear, :62,67), in fp32."""
    f = np.float32
    with np.errstate(all="ignore"):
        if qtype == _lib.QT_LINEAR:
            p = np.abs(f(q_m))
        else:
            p = np.exp(f(t) * np.log(np.abs(f(q_m)) + f(1e-6)), dtype=np.float32)
        q = f(p) / f(d)
    return float(np.rint(q)) if np.isfinite(q) else float("inf")


# ---- quantizer autograd functions (quant_layers.py:33-290) -----------------------------------------
def _clip_pair(clip_val) -> Tuple[float, float]:
    if isinstance(clip_val, torch.Tensor):
        clip_val = clip_val.detach().cpu().tolist()
    lo, hi = clip_val
    return float(lo), float(hi)


def _check_q_s(q_s) -> None:
    """q_s is 0 everywhere in the reference's callers (quant_layers.py:335,362); a host value is checked, a
    device tensor is taken on trust (reading it would sync)."""
    if q_s is None or (isinstance(q_s, torch.Tensor) and q_s.is_cuda):
        return
    if float(q_s) != 0.0:
        raise NotImplementedError("the HIP quantizers implement q_s = 0 only")


def _nan_message(what: str, names, tensors, host) -> str:
    vals = ", ".join(f"{n}: {float(v.reshape(-1)[0]):.5f}" for n, v in zip(names, tensors) if v is not None)
    return (f"Error: NaN appears in gradient ({what})!\n{vals}, q_s: 0\n"
            f"grad_d: {host[0]:.5f}\ngrad_qm: {host[1]:.5f}\ngrad_t: {host[2]:.5f}")


def _quantizer_forward(ctx, input_, d_quant, q_m, t_quant, clip_val, q_s, qtype: int, dge_k: float):
    _check_q_s(q_s)
    dev = input_.device
    d, qm, t = (_as_param_ptr(p, dev) for p in (d_quant, q_m, t_quant))
    ctx.save_for_backward(input_, d, qm, t)
    ctx.qtype, ctx.dge_k, ctx.clip = qtype, dge_k, _clip_pair(clip_val)
    ctx.like = [None if p is None else (p.shape, p.device, p.dtype) for p in (d_quant, q_m, t_quant)]
    return _lib.fake_quant_f32(input_.detach(), qtype, d, qm, t).to(input_.dtype)


def _quantizer_backward(ctx, grad_output):
    """(grad_x, [grad_d, grad_qm, grad_t] shaped as the parameters, device scalars, saved tensors)."""
    input_, d, qm, t = ctx.saved_tensors
    gx, scal = _lib.quant_backward(input_, grad_output, ctx.qtype, d, qm, t, ctx.clip[0], ctx.clip[1], ctx.dge_k)
    grads = [None if like is None else scal[i:i + 1].reshape(like[0]).to(device=like[1], dtype=like[2])
             for i, like in enumerate(ctx.like)]
    return gx.to(input_.dtype), grads, scal, (d, qm, t)


class SymQuantizerLinear(torch.autograd.Function):
    """quant_layers.py:128-205 on the device: qvit_fake_quant_f32 forward, qvit_quant_backward backward."""

    @staticmethod
    def forward(ctx, input, d_quant, q_m, clip_val, q_s):
        return _quantizer_forward(ctx, input, d_quant, q_m, None, clip_val, q_s, _lib.QT_LINEAR, 0.0)

    @staticmethod
    def backward(ctx, grad_output):
        gx, grads, scal, params = _quantizer_backward(ctx, grad_output)
        host = scal.cpu().tolist()   # the one host sync (the reference syncs on the same check, :190-204)
        if math.isnan(host[0]):
            raise NanInGradientError(_nan_message("grad_d", ("d", "q_m"), params, host))
        return gx, grads[0], grads[1], None, None


class SymQuantizerNonLinear(torch.autograd.Function):
    """quant_layers.py:33-125 on the device."""

    @staticmethod
    def forward(ctx, input, d_quant, q_m, t_quant, clip_val, q_s):
        return _quantizer_forward(ctx, input, d_quant, q_m, t_quant, clip_val, q_s, _lib.QT_NONLINEAR, 0.0)

    @staticmethod
    def backward(ctx, grad_output):
        gx, grads, scal, params = _quantizer_backward(ctx, grad_output)
        host = scal.cpu().tolist()   # :108-123
        if math.isnan(host[2]):
            raise NanInGradientError(_nan_message("grad_t", ("d", "q_m", "t"), params, host))
        return gx, grads[0], grads[1], grads[2], None, None


class DGEQuantizer(torch.autograd.Function):
    """quant_layers.py:208-290 on the device: the linear quantizer's forward; the backward scales grad_x by
    (1/k) |x - d/2|^(1/k - 1), k = 5 * 4 / num_bits (:236), clamped to +-3."""

    @staticmethod
    def forward(ctx, input, d_quant, q_m, clip_val, q_s, num_bits):
        k = 5.0 * (4.0 / float(num_bits))
        if not k > 0.0:
            raise ValueError(f"DGEQuantizer: num_bits = {float(num_bits)} gives k = {k}")
        return _quantizer_forward(ctx, input, d_quant, q_m, None, clip_val, q_s, _lib.QT_LINEAR, k)

    @staticmethod
    def backward(ctx, grad_output):
        gx, grads, scal, params = _quantizer_backward(ctx, grad_output)
        host = torch.cat([scal, torch.isnan(gx).any().reshape(1).float()]).cpu().tolist()   # :281
        if host[3]:
            raise NanInGradientError(_nan_message(f"grad_x, k: {ctx.dge_k:.4f}", ("d", "q_m"), params, host))
        return gx, grads[0], grads[1], None, None, None


def _get_quantizer(qtype: QuantizationType):
    """quant_layers.py:292-300."""
    if qtype == QuantizationType.SYMMETRIC_LINEAR:
        return SymQuantizerLinear
    if qtype == QuantizationType.SYMMETRIC_NONLINEAR:
        return SymQuantizerNonLinear
    if qtype == QuantizationType.DGE:
        return DGEQuantizer
    raise NotImplementedError


# The int path's W4 GEMMs (qvit_gemm, qvit_gemm_qkv_split) take a register image of the packed codes (same
# results, each GEMM wave's weight rows loaded into registers instead of through LDS): "w4r" (qvit_pack_weight_w4r,
# the int4 bytes re-ordered; round 5: fc1 -2.6 % in the model) or "w8r" (qvit_pack_weight_w8r, the codes already
# unpacked to the MFMA's int8 operands: twice the bytes, no unpack in the main loop). QVIT_GEMM_WREG=w4 (or the
# older QVIT_GEMM_W4R=0) keeps the LDS-staged form (same-box A/B).
GEMM_WREG = os.environ.get("QVIT_GEMM_WREG", "w4r" if os.environ.get("QVIT_GEMM_W4R", "1") == "1" else "w4")
if GEMM_WREG not in ("w4", "w4r", "w8r"):
    raise ValueError(f"QVIT_GEMM_WREG={GEMM_WREG!r}: expected w4, w4r or w8r")
GEMM_W4R = GEMM_WREG != "w4"   # a register image is in use

# The backward GEMMs of QuantizeLinear (behind F.linear's backward): "hip" runs both on the project's kernels,
# dgrad (grad_out @ quantize_weight(W)) as qvit_gemm_wonly on the transposed weight codes wherever the plan holds
# packed codes, wgrad (grad_out^T @ quantize_act(x)) as qvit_gemm_wgrad on the int8 activation codes of the
# integer path; "torch" keeps both on torch.mm (fp32 library GEMMs); "dgrad" / "wgrad" select one op.
# QVIT_BWD_GEMM sets it (the measurement behind the default: DESIGN.md section 13).
BACKWARD_GEMM = os.environ.get("QVIT_BWD_GEMM", "hip")
_lib.backward_ops(BACKWARD_GEMM, "QVIT_BWD_GEMM")   # an unknown value stops the import


def _backward_gemm_ops() -> tuple:
    return _lib.backward_ops(BACKWARD_GEMM, "BACKWARD_GEMM")


# The backward GEMMs of QuantizeConv2d (behind F.conv2d's backward), a switch of its own: "hip" runs both on the
# project's kernels wherever the layer is eligible (groups 1, zero padding, packed codes), wgrad as qvit_gemm_wgrad
# on the recomputed im2col codes (integer path), dgrad as qvit_gemm_wonly on the transposed weight codes followed by
# qvit_col2im_quant_backward (the fold and the activation quantizer's backward in one pass); "torch" keeps both on
# torch.nn.grad's convolutions; "dgrad" / "wgrad" select one op. Unset (None: not a value the variable can name), a layer takes the route that was
# faster where it was measured: both ops on the kernels where no two kernel taps reach the
# same input element (stride >= dilated kernel extent on both axes: the patch embeddings, 2.1x to 9.6x the library),
# both on the library where taps overlap (P is then kh kw / (sh sw) times the image; the one 3 x 3 stride-1 layer
# measured ran at a third of the library's speed on either op). QVIT_CONV_BWD_GEMM sets it.
CONV_BACKWARD_GEMM = os.environ.get("QVIT_CONV_BWD_GEMM")
if CONV_BACKWARD_GEMM is not None:
    _lib.backward_ops(CONV_BACKWARD_GEMM, "QVIT_CONV_BWD_GEMM")


def _conv_backward_gemm_ops(overlap: bool) -> tuple:
    if CONV_BACKWARD_GEMM is None:
        return () if overlap else ("dgrad", "wgrad")
    return _lib.backward_ops(CONV_BACKWARD_GEMM, "CONV_BACKWARD_GEMM")


def _wreg_unit_order(device: torch.device) -> torch.Tensor:
    """For each of the 1024 fragments of a (tile_n, k-stage) chunk of a register image, in the image's order, the
    index of the 8-byte fragment of the packed W4 chunk it was taken from (pack_w4r_kernel / pack_w8r_kernel: wave w,
    lane l, r -> row 64 w + 16 r + (l & 15), the row's k-chunk (l >> 4) ^ (2 if l & 8 else 0)): a permutation."""
    u = torch.arange(1024, device=device)
    w, ln, r = (u >> 8) & 3, (u >> 2) & 63, u & 3
    lfr, lfq = ln & 15, ln >> 4
    return (64 * w + 16 * r + lfr) * 4 + (lfq ^ (((lfr >> 3) & 1) << 1))


def unpack_wreg(image: torch.Tensor, wfmt: int, npad: int, kpad: int) -> torch.Tensor:
    """The packed W4 codes (qvit_pack_weight layout) a register image was made from, bit for bit: the inverse of
    qvit_pack_weight_w4r (a permutation of 8-byte fragments) or qvit_pack_weight_w8r (the same permutation, every
    nibble widened to the byte 16 k). Torch index ops on the device: this runs once per plan and route, never per
    forward."""
    if wfmt == _lib.W8R:
        q = image.view(torch.int32).view(-1, 4)   # nib16_lo(p.x), nib16_hi(p.x), nib16_lo(p.y), nib16_hi(p.y)
        lo, hi = 0x0F0F0F0F, -0x0F0F0F10            # 0xF0F0F0F0 as an int32
        frags = torch.stack([((q[:, 0] >> 4) & lo) | (q[:, 1] & hi), ((q[:, 2] >> 4) & lo) | (q[:, 3] & hi)], 1)
    elif wfmt == _lib.W4R:
        frags = image.view(torch.int32).view(-1, 2)
    else:
        raise ValueError(f"unpack_wreg: wfmt {wfmt} is no register image")
    frags = frags.view(-1, 1024, 2)
    out = torch.empty_like(frags)
    out[:, _wreg_unit_order(image.device)] = frags
    packed = out.view(-1).view(torch.uint8)
    assert packed.numel() == npad * kpad // 2
    return packed


def unpack_codes(packed: torch.Tensor, wfmt: int, npad: int, kpad: int) -> torch.Tensor:
    """The integer codes of a packed weight image, fp32 [npad, kpad]: the inverse of qvit_pack_weight's layout
    (quant_kernels.hip: packed_offset, perm_row) in torch index ops, exact. Per (256-row block, 64-k stage) tile, row
    r holds its 16-k chunk c at position c ^ (2 if r & 8 else 0) (W4, 8 bytes: byte b of each half = codes b and
    b + 4 as low and high nibble) or c ^ (2 if r & 4 else 0) (W8, 16 bytes); packed row rho is weight row rho with
    bits [3:2] and [5:4] swapped; W16 / W24 are two / three W8 images of base-256 digits, most significant first."""
    dev = packed.device
    if wfmt in (_lib.W16, _lib.W24):
        digits = packed.view(-1, npad * kpad)
        out = torch.zeros((npad, kpad), dtype=torch.float32, device=dev)
        for img in digits:     # exact in fp32: |codes| < 2^23
            out = out * 256.0 + unpack_codes(img, _lib.W8, npad, kpad)
        return out
    nb, st = npad // 256, kpad // 64
    r = torch.arange(256, device=dev)
    pos = torch.arange(4, device=dev)
    if wfmt == _lib.W4:
        b = packed.view(nb, st, 256, 4, 2, 4).to(torch.int16)
        nib = torch.stack([b & 15, b >> 4], dim=-2)                  # [..., half, low / high nibble, byte]
        vals = ((nib ^ 8) - 8).reshape(nb, st, 256, 4, 16)           # sign-extended, k order within the chunk
        swz = ((r >> 3) & 1) << 1
    elif wfmt == _lib.W8:
        vals = packed.view(torch.int8).view(nb, st, 256, 4, 16).to(torch.int16)
        swz = ((r >> 2) & 1) << 1
    else:
        raise ValueError(f"unpack_codes: wfmt {wfmt}")
    chunk_at = pos[None, :] ^ swz[:, None]                            # [row, chunk] -> position
    vals = vals.gather(3, chunk_at[None, None, :, :, None].expand(nb, st, 256, 4, 16))
    rows = vals.permute(0, 2, 1, 3, 4).reshape(npad, kpad)            # packed rows x k
    rho = torch.arange(npad, device=dev)
    perm = (rho & ~63) | (((rho >> 2) & 3) << 4) | (((rho >> 4) & 3) << 2) | (rho & 3)   # an involution
    return rows[perm].float()


@dataclass
class QuantPlan:
    """Per-layer device state derived from the parameters (rebuilt when any of them changes). Every image the plan
    hands out, also one it builds later, is made from what the plan holds (the packed codes or the register image,
    its copies of the bias and its views of the quantizer scalars), never from the layer's live weight: after an
    edit the key cannot see (`.data`), the plan answers for the weights it was built from on every route until
    invalidate()."""
    key: tuple
    device: torch.device
    qtype: int
    n: int
    k: int
    npad: int
    kpad: int
    wfmt: int                       # _lib.W4 / _lib.W8 / 0 (fp32 fake-quant path)
    int_path: bool                  # activation codes fit int8 and the weight was packed
    level_wt: float
    level_act: float
    packed: Optional[torch.Tensor] = None
    bias_pad: Optional[torch.Tensor] = None
    w_fakequant: Optional[torch.Tensor] = None
    d_wt: Optional[torch.Tensor] = None
    qm_wt: Optional[torch.Tensor] = None
    t_wt: Optional[torch.Tensor] = None
    d_act: Optional[torch.Tensor] = None
    qm_act: Optional[torch.Tensor] = None
    t_act: Optional[torch.Tensor] = None
    extra: dict = field(default_factory=dict)
    # views of every tensor the key names by address: while the plan lives their storage cannot be freed and handed
    # to a new parameter, so an equal key always means the same tensors
    held: tuple = ()

    @property
    def has_codes(self) -> bool:
        """The plan holds packed weight codes (integer path or weight-only GEMM), so packed_t() can transpose them."""
        return self.int_path or bool(self.extra.get("wonly"))

    @property
    def act_q(self) -> tuple:
        """The activation quantizer as the kernels' wrappers take it: (qtype, d, q_m, t)."""
        return self.qtype, self.d_act, self.qm_act, self.t_act

    @property
    def wt_q(self) -> tuple:
        """The weight quantizer, in the same order."""
        return self.qtype, self.d_wt, self.qm_wt, self.t_wt

    def __deepcopy__(self, memo):
        # a copied layer has parameters at other addresses: it builds its own plan (and copies no device images)
        return None

    def gemm_weights(self) -> Tuple[torch.Tensor, int]:
        """(image, wfmt) the int path's GEMM reads: the register image (W4R / W8R) of a W4 plan, else the packed
        codes. The register image is built on the first call and the packed codes it is made from are then
        released, so a layer holds its int4 weights once. Every int-path layer comes through here (QuantizeLinear,
        and QuantizeConv2d by conv_codes_gemm -> gemm_codes); the fused qkv + attention kernel, the residual GEMM
        with LayerNorm and the weight-stationary fc1 GEMM read the packed codes, which `packed_codes()` gives
        back."""
        if self.int_path and self.wfmt == _lib.W4 and GEMM_WREG != "w4" and "wreg" not in self.extra:
            src = self.packed_codes()
            pack = _lib.pack_weight_w4r if GEMM_WREG == "w4r" else _lib.pack_weight_w8r
            image, fmt = pack(src, self.npad, self.kpad), _lib.W4R if GEMM_WREG == "w4r" else _lib.W8R
            self.extra["wreg"] = (image, fmt)
            # how the packed codes come back: un-permuted from the register image (the closure holds that image,
            # not the layer's weights)
            npad, kpad = self.npad, self.kpad
            self.extra["repack"] = lambda: unpack_wreg(image, fmt, npad, kpad)
            self.packed = None
        wreg = self.extra.get("wreg")
        return wreg if wreg is not None else (self.packed_codes(), self.wfmt)

    def packed_codes(self) -> torch.Tensor:
        """The packed weight codes (qvit_pack_weight layout); if gemm_weights() released them, un-permuted from
        the register image it kept (unpack_wreg: the same bytes) and held from then on."""
        if self.packed is None:
            self.packed = self.extra["repack"]()
        return self.packed

    def codes(self) -> torch.Tensor:
        """The plan's integer weight codes, fp32 [n, k], read back from the packed image it holds (unpack_codes).
        Serves the images built after the plan (packed_t, w_fakequant, weight_codes), so they hold the codes of the
        forward whatever became of the layer's weight."""
        if not self.has_codes:
            raise _lib.QvitError("QuantPlan.codes: the plan holds no packed codes")
        packed = self.packed if self.packed is not None else self.extra["repack"]()   # a released image: not kept
        return unpack_codes(packed, self.wfmt, self.npad, self.kpad)[:self.n, :self.k]

    def packed_t(self) -> Tuple[torch.Tensor, int, int]:
        """(image, npad, kpad) of the TRANSPOSED weight codes in the plan's wfmt (rows = in-features padded to
        TILE_N, reduction = out-features padded to TILE_K): the operand of the input gradient on qvit_gemm_wonly.
        Packed from codes() on the first backward (_lib.pack_codes: exact) and kept with the plan (whose key follows
        every parameter update)."""
        if "packed_t" not in self.extra:
            npad_t, kpad_t = _lib.round_up(self.k, _lib.TILE_N), _lib.round_up(self.n, _lib.TILE_K)
            if "t_src" in self.extra:   # a training-mode plan: the weight of this very step (_build_plan)
                src, qargs = self.extra["t_src"]
                overflow = torch.zeros(1, dtype=torch.int32, device=self.device)
                image = _lib.pack_weight(src.t().contiguous(), *qargs, self.wfmt, npad_t, kpad_t, overflow)
                self.extra["packed_t"] = (image, npad_t, kpad_t)
                return self.extra["packed_t"]
            ct = self.codes().t().contiguous()
            if self.wfmt in (_lib.W16, _lib.W24):   # the same largest code: the same digit count
                image, wfmt = _lib.pack_weight_wide(ct, npad_t, kpad_t)
                assert wfmt == self.wfmt
            else:
                image = _lib.pack_codes(ct, self.wfmt, npad_t, kpad_t)
            self.extra["packed_t"] = (image, npad_t, kpad_t)
        return self.extra["packed_t"]


class QuantizeMixin:
    """quant_layers.py:303-410 — parameters, quantize_weight/quantize_act, bit-width properties."""

    def init_quantization(
        self,
        d_quant_init: float = 1.0,
        t_quant_init: float = 1.0,
        q_m_init: float = 1.0,
        quant_type: QuantizationType = QuantizationType.SYMMETRIC_LINEAR,
        quant_mode: QuantizationMode = QuantizationMode.WEIGHT_ONLY,
        weight_clip_val: Tuple[float, float] = (-2.0, 2.0),
        act_clip_val: Tuple[float, float] = (-2.0, 2.0),
    ):
        self.d_quant_wt = nn.Parameter(torch.tensor([d_quant_init]))
        self.q_m_wt = nn.Parameter(torch.tensor([q_m_init]))
        if quant_type == QuantizationType.SYMMETRIC_NONLINEAR:
            self.t_quant_wt = nn.Parameter(torch.tensor([t_quant_init]))
        if quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION:
            self.d_quant_act = nn.Parameter(torch.tensor([d_quant_init]))
            self.q_m_act = nn.Parameter(torch.tensor([q_m_init]))
            if quant_type == QuantizationType.SYMMETRIC_NONLINEAR:
                self.t_quant_act = nn.Parameter(torch.tensor([t_quant_init]))
        self.quant_type = quant_type
        self.quant_mode = quant_mode
        self.weight_clip_val = weight_clip_val
        self.act_clip_val = act_clip_val
        self._qplan: Optional[QuantPlan] = None
        self._weight_codes: Optional[Tuple[tuple, torch.Tensor]] = None

    # -- reference API: fake-quant fp32 tensors (quant_layers.py:332-381) -------------------
    def _quantize_fn(self, x: torch.Tensor, which: str, clip_val) -> torch.Tensor:
        """The quantizer as an autograd function (quant_layers.py:336-354, 363-381)."""
        quantizer = _get_quantizer(self.quant_type)
        d, qm = getattr(self, f"d_quant_{which}"), getattr(self, f"q_m_{which}")
        if self.quant_type == QuantizationType.SYMMETRIC_LINEAR:
            return quantizer.apply(x, d, qm, clip_val, 0.0)
        return quantizer.apply(x, d, qm, getattr(self, f"t_quant_{which}"), clip_val, 0.0)

    def _records_grad(self, x: torch.Tensor) -> bool:
        """Autograd-live and a quantizer type the modules can differentiate (DGE through the modules has no
        backward, here as in the reference, :346-354: it is exposed as DGEQuantizer only)."""
        if not _autograd_live(self, x):
            return False
        if self.quant_type == QuantizationType.DGE:
            _warn_no_grad()
            return False
        return True

    def _fake_quant(self, x: torch.Tensor, which: str, clip_val) -> torch.Tensor:
        """The `which` ("wt" / "act") quantizer's values of x: the autograd function when history is wanted, else
        the bare kernel."""
        if self._records_grad(x):
            return self._quantize_fn(x, which, clip_val)
        d, qm, t = (_as_param_ptr(getattr(self, f"{name}_{which}", None), x.device)
                    for name in ("d_quant", "q_m", "t_quant"))
        return _lib.fake_quant_f32(x.detach(), _qtype_code(self.quant_type), d, qm, t)

    def quantize_weight(self, weight: torch.Tensor) -> torch.Tensor:
        return self._fake_quant(weight, "wt", self.weight_clip_val)

    def quantize_act(self, activation: torch.Tensor) -> torch.Tensor:
        if self.quant_mode != QuantizationMode.WEIGHT_AND_ACTIVATION:
            return activation
        return self._fake_quant(activation, "act", self.act_clip_val)

    def _bit_width(self, which: str) -> int:
        """round(log2(|q_m|^t / |d| + 1) + 1) of the `which` ("wt" / "act") quantizer (quant_layers.py:383-410)."""
        d = getattr(self, f"d_quant_{which}").item()
        qmax = abs(getattr(self, f"q_m_{which}").item())
        if self.quant_type == QuantizationType.SYMMETRIC_LINEAR:
            t = 1.0
        elif self.quant_type == QuantizationType.SYMMETRIC_NONLINEAR:
            t = getattr(self, f"t_quant_{which}").item()
        else:
            raise NotImplementedError
        return round(math.log2(math.exp(t * math.log(qmax)) / abs(d) + 1) + 1)

    @property
    def weight_bit(self) -> int:
        return self._bit_width("wt")

    @property
    def activation_bit(self) -> int:
        if self.quant_mode != QuantizationMode.WEIGHT_AND_ACTIVATION:
            return 32
        return self._bit_width("act")

    # -- MI355X state ---------------------------------------------------------------------------
    def prepare(self):
        """Packs the weight codes (and bias, code tables' inputs) on the device now instead of at the first
        forward: the reference re-quantizes on every call; here the packed form is cached per
        parameter version, so this only moves the one-time cost out of the first timed call. Returns self."""
        self.quant_plan()
        return self

    def invalidate(self) -> None:
        """Drops the cached quantized weight. Needed only after editing parameters through
        `.data` (which bypasses the version counter the cache keys on)."""
        self._qplan = None

    def load_weight_codes(self, codes: Optional[torch.Tensor]) -> None:
        """Uses the given integer weight codes k (quantize_weight(W) == d_quant_wt * k, quant_layers.py:332-354)
        instead of deriving them on the device — e.g. the codes the reference's own host computed, so that
        both sides run on identical int4 weights. The codes stay bound to the current parameter versions:
        editing any parameter drops them (the device derives the codes again). `None` unbinds them."""
        if codes is None:
            self._weight_codes = None
        else:
            c = torch.as_tensor(codes).detach()
            if c.is_floating_point() and not torch.equal(c, c.round()):
                raise ValueError("weight codes must be integers")
            if tuple(c.shape) != tuple(self.weight.shape):
                raise ValueError(f"weight codes of shape {tuple(c.shape)} for a weight of shape "
                                 f"{tuple(self.weight.shape)}")
            self._weight_codes = (self._plan_key(), c.reshape(c.shape[0], -1).to(torch.int16), self._held_tensors())
        self._qplan = None

    def _bound_weight_codes(self, key: tuple) -> Optional[torch.Tensor]:
        wc = self._weight_codes
        if wc is None:
            return None
        if (wc[0][0],) + wc[0][3:] != (key[0],) + key[3:]:   # type or a parameter changed since the load
            self._weight_codes = None
            return None
        return wc[1]

    def _quant_param_tensors(self):
        names = ["weight", "bias", "d_quant_wt", "q_m_wt", "t_quant_wt", "d_quant_act", "q_m_act", "t_quant_act"]
        return [getattr(self, n, None) for n in names]

    def _held_tensors(self) -> tuple:
        """A view of every tensor _plan_key names by address, for whoever keeps such a key: the storage stays
        allocated, so no later parameter can take the address at the same version."""
        return tuple(None if p is None else p.detach() for p in self._quant_param_tensors())

    def _plan_key(self) -> tuple:
        key = [self.quant_type, self.quant_mode, self.training]
        for p in self._quant_param_tensors():
            key.append(None if p is None else (p.data_ptr(), p._version, p.device, p.dtype, tuple(p.shape)))
        return tuple(key)

    def _weight_2d(self) -> torch.Tensor:
        w = self.weight.detach()
        return w.reshape(w.shape[0], -1)

    def quant_plan(self) -> QuantPlan:
        """Builds (or returns the cached) device plan. Building syncs the host once (it reads the
        scalar quantizer parameters to choose int4 / int8 / fp32 storage)."""
        key = self._plan_key()
        plan = self._qplan
        if plan is not None and plan.key == key and not self.training:
            return plan
        plan = self._build_plan(key)
        self._qplan = plan
        return plan

    def _build_plan(self, key: tuple) -> QuantPlan:
        w2 = self._weight_2d()
        dev = w2.device
        if not w2.is_cuda:
            raise _lib.QvitError(f"{type(self).__name__}: weights are on {dev}; move the model to a ROCm "
                                 "device (the HIP path has no CPU fallback)")
        qt = _qtype_code(self.quant_type)
        n, k = w2.shape
        npad, kpad = _lib.round_up(n, _lib.TILE_N), _lib.round_up(k, _lib.TILE_K)
        d_wt = _as_param_ptr(self.d_quant_wt, dev)
        qm_wt = _as_param_ptr(self.q_m_wt, dev)
        t_wt = _as_param_ptr(getattr(self, "t_quant_wt", None), dev)
        wa = self.quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION
        d_act = _as_param_ptr(getattr(self, "d_quant_act", None), dev) if wa else None
        qm_act = _as_param_ptr(getattr(self, "q_m_act", None), dev) if wa else None
        t_act = _as_param_ptr(getattr(self, "t_quant_act", None), dev) if wa else None
        # one host sync: the scalar parameters decide the storage format
        bias_max = (self.bias.detach().abs().max().float().reshape(1).to(dev) if self.bias is not None
                    else torch.zeros(1, device=dev))
        scal = torch.stack([x.reshape(-1)[0] for x in (d_wt, qm_wt, t_wt if t_wt is not None else d_wt)]
                           + ([d_act.reshape(-1)[0], qm_act.reshape(-1)[0],
                               (t_act if t_act is not None else d_act).reshape(-1)[0]] if wa else [])
                           + [bias_max[0]]).cpu()
        s = scal.tolist()
        lw = saturation_level(qt, s[0], s[1], s[2] if t_wt is not None else 1.0)
        la = saturation_level(qt, s[3], s[4], s[5] if t_act is not None else 1.0) if wa else float("inf")
        plan = QuantPlan(key=key, device=dev, qtype=qt, n=n, k=k, npad=npad, kpad=kpad, wfmt=0, int_path=False,
                         level_wt=lw, level_act=la, d_wt=d_wt, qm_wt=qm_wt, t_wt=t_wt, d_act=d_act,
                         qm_act=qm_act, t_act=t_act, held=self._held_tensors())
        w32 = w2 if (w2.dtype == torch.float32 and w2.is_contiguous()) else w2.float().contiguous()
        act_ok = wa and abs(la) <= 127
        codes = self._bound_weight_codes(key)
        if codes is not None:
            cmax = int(codes.abs().max().item()) if codes.numel() else 0
            if cmax > abs(lw):
                raise ValueError(f"{type(self).__name__}: loaded weight code {cmax} exceeds the quantizer's "
                                 f"saturation level {lw}")
            plan.extra["weight_codes"] = True
            w32 = codes.to(device=dev, dtype=torch.float32).contiguous()
            qt_pack, d_pack, qm_pack, t_pack = _lib.code_quantizer(dev)
        else:
            qt_pack, d_pack, qm_pack, t_pack = qt, d_wt, qm_wt, t_wt
        if act_ok and abs(lw) <= 127:
            overflow = torch.zeros(1, dtype=torch.int32, device=dev)
            for wfmt in ((_lib.W4, _lib.W8) if abs(lw) <= 7 else (_lib.W8,)):
                overflow.zero_()
                packed = _lib.pack_weight(w32, qt_pack, d_pack, qm_pack, t_pack, wfmt, npad, kpad, overflow)
                if int(overflow.item()) == 0:
                    plan.packed, plan.wfmt, plan.int_path = packed, wfmt, True
                    break
        if not plan.int_path and abs(lw) <= 65536:
            # fp32 activations against the packed weight codes (qvit_gemm_wonly, QuantizeLinear): the weight-only
            # mode (the reference's default) and W+A layers off the int path (levels beyond int8: their
            # activations are fake-quantized to fp32 first); int4 / int8 codes as on the int path, wider ones
            # (e.g. the default num_bits = 16) as balanced base-256 digits (W16 / W24)
            if abs(lw) <= 127:
                overflow = torch.zeros(1, dtype=torch.int32, device=dev)
                for wfmt in ((_lib.W4, _lib.W8) if abs(lw) <= 7 else (_lib.W8,)):
                    overflow.zero_()
                    packed = _lib.pack_weight(w32, qt_pack, d_pack, qm_pack, t_pack, wfmt, npad, kpad, overflow)
                    if int(overflow.item()) == 0:
                        plan.packed, plan.wfmt = packed, wfmt
                        plan.extra["wonly"] = True
                        break
            else:
                wc = codes.to(device=dev, dtype=torch.float32) if codes is not None else \
                    (_lib.fake_quant_f32(w32, qt, d_wt, qm_wt, t_wt) / d_wt).round()
                plan.packed, plan.wfmt = _lib.pack_weight_wide(wc, npad, kpad)
                plan.extra["wonly"] = True
        if self.training and plan.wfmt in (_lib.W4, _lib.W8):
            # a training-mode plan is rebuilt on every call, so the weight it was built from is the live one for the
            # whole step: its backward packs the transposed codes straight from that weight (one transposing copy and
            # one pack kernel per step and layer, as before the plan learnt to decode its own image)
            plan.extra["t_src"] = (w32, (qt_pack, d_pack, qm_pack, t_pack))
        if plan.has_codes:
            bias = self.bias.detach() if self.bias is not None else None
            plan.bias_pad = _lib.pad_bias(bias, n, npad, dev)
            # |output| <= d_act d_wt sum_k |a_k||w_k| + |bias| <= d_act d_wt K L_a L_w + max|bias| (integer path
            # only: a weight-only plan has no activation scalars, and its output is unbounded a priori)
            plan.extra["out_bound"] = (abs(s[3] * s[0]) * k * abs(la) * abs(lw) + s[-1]) if plan.int_path \
                else float("inf")
        if wa:   # host copies of the activation quantizer's scalars (epilogue code tables of the producer)
            plan.extra["act_host"] = (qt, s[3], s[4], s[5] if t_act is not None else 1.0, la)
        # the fp32 form, where the forward itself contracts it: levels that fit no packed format (beyond 65536), and
        # a convolution the code kernels do not take (groups, padding modes); otherwise it is filled lazily, from
        # the plan's codes (w_fakequant)
        if (not plan.int_path and not plan.extra.get("wonly")) or not self._codes_forward_ok():
            plan.w_fakequant = self._fake_quant_weight(plan)
        return plan

    def _codes_forward_ok(self) -> bool:
        """Whether the forward of a plan with packed codes runs on them (QuantizeConv2d: _int_conv_ok)."""
        return True

    def _fake_quant_weight(self, plan: QuantPlan) -> torch.Tensor:
        """quantize_weight(W) on the device, from the layer's weight: only while the plan is being built (the
        weight is then the one the key names); with codes bound by load_weight_codes, d_w * k of exactly those
        codes."""
        codes = self._bound_weight_codes(plan.key)
        if codes is not None:
            k = codes.to(device=plan.device, dtype=torch.float32)
            return (plan.d_wt * k).view_as(self.weight)      # d_w * k, as quantize_weight returns it
        return _lib.fake_quant_f32(self.weight.detach().float(), *plan.wt_q)

    def weight_codes(self) -> torch.Tensor:
        """The integer weight codes the device path uses ([N, K] float32 on the device): the loaded ones
        (load_weight_codes) or the device quantizer's."""
        plan = self.quant_plan()
        wc = self._bound_weight_codes(plan.key)
        if wc is not None:
            return wc.to(device=plan.device, dtype=torch.float32)
        if plan.int_path or plan.extra.get("wonly"):
            return plan.codes().contiguous()       # what the plan's kernels multiply by
        return (plan.w_fakequant.reshape(plan.n, plan.k) / plan.d_wt).round()

    def _wonly_rows(self, x2: torch.Tensor, plan: QuantPlan) -> torch.Tensor:
        """[M, k] fp32 rows (or rows already zero-padded to kpad columns) @ quantize_weight(W)^T + b on
        qvit_gemm_wonly (weight-only / wide-level plans)."""
        return _lib.gemm_wonly_rows(x2, plan.k, plan.kpad, plan.packed, plan.wfmt, plan.n, plan.npad, plan.d_wt,
                                    plan.bias_pad)

    def w_fakequant(self, plan: QuantPlan) -> torch.Tensor:
        """The reference's quantize_weight(W) (quant_layers.py:332-354), cached on the plan: d_w * k of the plan's
        own codes (qvit_fake_quant_f32's value, fake_quant_value in qvit_common.h, for every finite weight up to the
        sign of zero: a negative weight with code 0 gives +0.0 here and -0.0 there, which no contraction with finite
        operands can tell apart; a NaN weight has the code 0 the kernels contract, where qvit_fake_quant_f32 passes
        the NaN on)."""
        if plan.w_fakequant is None:
            plan.w_fakequant = (plan.d_wt * plan.codes()).view(self.weight.shape)
        return plan.w_fakequant

    def _check_input(self, x: torch.Tensor) -> None:
        if not x.is_cuda:
            raise _lib.QvitError(f"{type(self).__name__}: input on {x.device}; the HIP path needs a ROCm "
                                 "device tensor (no CPU fallback)")

    # -- autograd (quant_layers.py:71-125, 163-205 behind F.linear / F.conv2d's own backward) ------
    def _forward_autograd(self, input_: torch.Tensor, plan: QuantPlan) -> torch.Tensor:
        g = lambda n: getattr(self, n, None)
        return _QuantLayerFunction.apply(self, plan, input_, self.weight, self.bias, g("d_quant_wt"), g("q_m_wt"),
                                         g("t_quant_wt"), g("d_quant_act"), g("q_m_act"), g("t_quant_act"))

    def _gemm_grads(self, plan: QuantPlan, xshape: tuple, x_q: Optional[torch.Tensor],
                    w_q: Optional[torch.Tensor], G: torch.Tensor):
        """Gradients of the contraction on torch's fp32 GEMM / convolution: (w.r.t. the quantized input, when
        w_q is given; w.r.t. the quantized weight, when x_q is given), contiguous fp32."""
        raise NotImplementedError

    def _backward_gemm_routes(self, plan: QuantPlan, need_xq: bool, need_wq: bool) -> Tuple[bool, bool]:
        """(dgrad, wgrad) on the HIP kernels (BACKWARD_GEMM for QuantizeLinear, CONV_BACKWARD_GEMM for
        QuantizeConv2d)."""
        return False, False

    def _gemm_grads_hip(self, plan: QuantPlan, xf: torch.Tensor, x_q: Optional[torch.Tensor],
                        w_q: Optional[torch.Tensor], G: torch.Tensor, hip_x: bool, hip_w: bool):
        """_gemm_grads with the ops flagged by _backward_gemm_routes on the HIP kernels. A third element, when
        returned, holds the activation quantizer's device scalars: the first is then already the gradient of the
        layer's input (QuantizeConv2d's dgrad folds and applies that quantizer's backward in one kernel)."""
        raise NotImplementedError

    def _grad_out_layout(self, G: torch.Tensor, library_op: bool) -> torch.Tensor:
        """The fp32 output gradient as the GEMM gradients read it; `library_op`: an op on torch's route reads it."""
        return G.contiguous()

    def _dgrad_hip(self, plan: QuantPlan, G2: torch.Tensor) -> torch.Tensor:
        """G2 @ (d_wt k_w), contiguous [M, k]: qvit_gemm_wonly on the transposed codes (rows = in-features,
        reduction = out-features)."""
        packed_t, npad_t, kpad_t = plan.packed_t()
        if G2.shape[0] == 0:
            return torch.empty((0, plan.k), dtype=torch.float32, device=G2.device)
        return _lib.gemm_wonly_rows(G2, plan.n, kpad_t, packed_t, plan.wfmt, plan.k, npad_t, plan.d_wt,
                                    None).contiguous()

    def _backward_plan(self, plan: QuantPlan, x: torch.Tensor, weight: torch.Tensor, G: torch.Tensor,
                       needs: tuple) -> tuple:
        """Gradients of _forward_plan's output for (input, weight, bias, d_quant_wt, q_m_wt, t_quant_wt,
        d_quant_act, q_m_act, t_quant_act); None where `needs` is false (that work is skipped)."""
        wa = self.quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION
        need_x, need_w, need_b = needs[0], needs[1], needs[2]
        need_wq = need_w or any(needs[3:6])          # the weight quantizer's backward runs
        need_aq = wa and (need_x or any(needs[6:9]))   # the activation quantizer's backward runs
        need_xq = need_aq or need_x
        hip_x, hip_w = self._backward_gemm_routes(plan, need_xq, need_wq)
        G = self._grad_out_layout(G.detach().float(), (need_xq and not hip_x) or (need_wq and not hip_w))
        xf = x.detach().float().contiguous()
        grad_b = None
        if need_b:
            grad_b = (G.sum((0, 2, 3)) if isinstance(self, nn.Conv2d) else G.reshape(-1, plan.n).sum(0)) \
                .to(self.bias.dtype)
        # the operands the forward contracted: quantize_weight(W), and d_act * codes (fake_quant_f32 and the int8
        # paths share quant_code) or the input itself in weight-only mode
        # (an op on its HIP route reads the integer codes instead: BACKWARD_GEMM)
        w_q = self.w_fakequant(plan).view_as(weight) if need_xq and not hip_x else None
        x_q = None
        if need_wq and not hip_w:
            x_q = _lib.fake_quant_f32(xf, *plan.act_q) if wa else xf
        act_done = ()   # QuantizeConv2d's dgrad: the activation quantizer's backward ran with it, (its scalars,)
        if hip_x or hip_w:
            grad_xq, grad_wq, *act_done = self._gemm_grads_hip(plan, xf, x_q, w_q, G, hip_x, hip_w)
        else:
            grad_xq, grad_wq = self._gemm_grads(plan, tuple(xf.shape), x_q, w_q, G)
        quantizers = []   # (which, grad through the quantizer, device scalars)
        grad_x = grad_xq
        if need_aq and act_done:
            quantizers.append(("act", act_done[0]))
        elif need_aq:
            grad_x, scal = _lib.quant_backward(xf, grad_xq, *plan.act_q, self.act_clip_val[0], self.act_clip_val[1],
                                               grad_x=grad_xq)
            quantizers.append(("act", scal))
        grad_w = None
        if need_wq:
            wf = weight.detach().float().contiguous()
            grad_w, scal = _lib.quant_backward(wf, grad_wq, *plan.wt_q, self.weight_clip_val[0],
                                               self.weight_clip_val[1], grad_x=grad_wq)
            quantizers.append(("wt", scal))
        scalars = self._checked_scalars(plan, quantizers)
        out = [grad_x.view_as(x).to(x.dtype) if need_x else None,
               grad_w.view_as(weight).to(weight.dtype) if need_w else None,
               grad_b]
        return tuple(out) + self._scalar_grads(scalars, needs[3:9])

    def _checked_scalars(self, plan: QuantPlan, quantizers: list) -> dict:
        """{which: device scalars} of the quantizer backwards that ran, after the one host readback behind both
        quantizers' NaN checks (:108-123 grad_t, :190-204 grad_d)."""
        scalars = {}
        if quantizers:
            host = torch.cat([sc for _, sc in quantizers]).cpu().tolist()
            chk = 2 if plan.qtype == _lib.QT_NONLINEAR else 0
            for i, (which, sc) in enumerate(quantizers):
                scalars[which] = sc
                h = host[3 * i:3 * i + 3]
                if math.isnan(h[chk]):
                    params = [getattr(self, f"{n}_{which}", None) for n in ("d_quant", "q_m", "t_quant")]
                    raise NanInGradientError(_nan_message(
                        f"{type(self).__name__} {which} quantizer, {'grad_t' if chk else 'grad_d'}",
                        ("d", "q_m", "t"), params, h))
        return scalars

    def _scalar_grads(self, scalars: dict, needs: tuple) -> tuple:
        """Gradients of (d_quant_wt, q_m_wt, t_quant_wt, d_quant_act, q_m_act, t_quant_act) shaped as the
        parameters; None where `needs` (six flags, that order) is false."""
        out = []
        for j, which in ((0, "wt"), (3, "act")):
            for i, name in enumerate(("d_quant", "q_m", "t_quant")):
                p = getattr(self, f"{name}_{which}", None)
                out.append(scalars[which][i:i + 1].reshape(p.shape).to(p.dtype) if needs[j + i] else None)
        return tuple(out)

    def _act_codes(self, x2d: torch.Tensor, plan: QuantPlan) -> torch.Tensor:
        M = x2d.shape[0]
        codes = torch.empty((M, plan.kpad), dtype=torch.int8, device=x2d.device)
        _lib.quantize_act_i8(x2d, *plan.act_q, 0, codes, plan.kpad)
        return codes

    def gemm_codes(self, codes: torch.Tensor, plan: QuantPlan, epilogue: int = _lib.EPI_F32,
                   out: Optional[torch.Tensor] = None, next_layer: Optional["QuantizeMixin"] = None) -> torch.Tensor:
        """Runs the contraction on activation codes (int8 [M, kpad]) with the given epilogue.
        EPI_I8 / EPI_I8_GELU quantize the result with `next_layer`'s activation quantizer."""
        if torch.is_grad_enabled() and _autograd_live(self, codes):
            _warn_no_grad()   # a direct low-level call: only the modules' forward() records autograd history
        M = codes.shape[0]
        dev = codes.device
        out_q, table = (0, None, None, None), None
        if epilogue in (_lib.EPI_I8, _lib.EPI_I8_GELU):
            nplan = next_layer.quant_plan()
            if out is None:
                out = torch.empty((M, _lib.round_up(plan.n, 16)), dtype=torch.int8, device=dev)
            out_q, table = nplan.act_q, epilogue_table(nplan, epilogue)
        elif epilogue == _lib.EPI_I32:
            if out is None:
                out = torch.empty((M, _lib.round_up(plan.n, 4)), dtype=torch.int32, device=dev)
        elif out is None:
            out = torch.empty((M, _lib.round_up(plan.n, 4)), dtype=torch.float32, device=dev)
        wimg, wfmt = plan.gemm_weights()
        _lib.gemm(codes, M, plan.kpad, wimg, wfmt, plan.n, plan.npad, plan.d_act, plan.d_wt,
                  plan.bias_pad, epilogue, out, *out_q, epi_table=table)
        return out

    def a32_fits(self, plan: QuantPlan, epilogue: int) -> bool:
        """Whether gemm_codes_a32 runs this layer (qvit_gemm_a32_fits: the fc1 shape class)."""
        return _lib.gemm_a32_fits(plan.kpad, plan.wfmt, plan.n, plan.npad, epilogue)

    def gemm_codes_a32(self, codes_t32: torch.Tensor, M: int, plan: QuantPlan, epilogue: int, out: torch.Tensor,
                       next_layer: "QuantizeMixin") -> torch.Tensor:
        """gemm_codes for the int8-code epilogues on QVIT_ACT_T32 activation codes (qvit_gemm_a32: weight-stationary
        schedule, same codes as gemm_codes on the row-major codes)."""
        nplan = next_layer.quant_plan()
        _lib.gemm_a32(codes_t32, M, plan.kpad, plan.packed_codes(), plan.wfmt, plan.n, plan.npad, plan.d_act, plan.d_wt,
                      plan.bias_pad, epilogue, out, *nplan.act_q, epi_table=epilogue_table(nplan, epilogue))
        return out


_GELU_MAX_SLOPE = 1.1289   # max of d/dv [v Phi(v)] (at v ~ 1.41)


def _gelu(v: float) -> float:
    return 0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0)))


def epilogue_table_geometry(qtype: int, d: float, qm: float, t: float, level: float, gelu: bool):
    """(v_lo, w, nb) of the int8-epilogue code table for an activation quantizer (host scalars), or None
    when the table would be too large (the GEMM then evaluates every element directly). Only the
    speed depends on this choice: the device validates the table and falls back on its own."""
    if qtype == _lib.QT_ULTRA_ACT or not (d > 0 and math.isfinite(d) and math.isfinite(qm) and qm != 0):
        return None
    L = int(abs(level))
    if L < 1 or L > 127:
        return None
    p = (lambda x: x) if qtype == _lib.QT_LINEAR else (lambda x: x ** (1.0 / t) if x > 0 else 0.0)
    if qtype == _lib.QT_NONLINEAR and not (t > 0 and math.isfinite(t)):
        return None
    # magnitude thresholds of the codes 1..L in x = gelu(v) (or v): x_k = p((k - 1/2) d), capped at |q_m|
    xs = [min(p((k - 0.5) * d), abs(qm)) for k in range(1, L + 1)]
    gaps = [b - a for a, b in zip(xs, xs[1:]) if b > a]
    min_gap = min(gaps + [2.0 * xs[0]])   # change points +-x_1 around the zero code are 2 x_1 apart
    x_sat, x_one = xs[-1], xs[0]
    if gelu:
        lo_v, hi_v = 0.0, max(1.0, x_sat)      # gelu(v) >= x_sat: v_hi
        while _gelu(hi_v) < x_sat * 1.02:
            hi_v *= 1.5
        v_hi = hi_v + 0.05
        if x_one >= 0.17:                       # min gelu = -0.17: no negative codes
            v_lo = -0.05
        else:                                   # most negative v with |gelu(v)| >= x_1
            a, b = -40.0, -0.7518
            for _ in range(80):
                mid = 0.5 * (a + b)
                if abs(_gelu(mid)) >= x_one * 0.98:
                    b = mid
                else:
                    a = mid
            v_lo = a - 0.05
        w = 0.8 * min_gap / _GELU_MAX_SLOPE
    else:
        v_hi, v_lo = x_sat * 1.02 + 1e-3, -(x_sat * 1.02 + 1e-3)
        w = 0.8 * min_gap
    # one more bucket below the first change point: bucket 0 then holds one code only, which frees its `lo` byte for
    # the code of a NaN (the device rejects a table whose bucket 0 has a change point)
    v_lo -= w
    nb = int(math.ceil((v_hi - v_lo) / w)) + 1
    if nb > _lib.EPI_TABLE_MAX_NB:
        return None
    return v_lo, w, nb


def epilogue_table(nplan: QuantPlan, epilogue: int) -> Optional[torch.Tensor]:
    """Device code table for a GEMM epilogue that quantizes with `nplan`'s activation quantizer (cached
    on that plan: it depends only on the quantizer's scalars)."""
    key = "epi_table_gelu" if epilogue == _lib.EPI_I8_GELU else "epi_table"
    if key not in nplan.extra:
        host = nplan.extra.get("act_host")
        geo = epilogue_table_geometry(*host, gelu=epilogue == _lib.EPI_I8_GELU) if host else None
        nplan.extra[key] = None if geo is None else _lib.epi_table_build(
            epilogue, *nplan.act_q, 0, geo[0], geo[1], geo[2], nplan.device)
    return nplan.extra[key]


class _QuantLayerFunction(torch.autograd.Function):
    """One autograd node around a layer's forward: the value is _forward_plan's (the code that runs under
    no_grad, on whichever path the plan selects), the backward is QuantizeMixin._backward_plan."""

    @staticmethod
    def forward(ctx, module, plan, input_, weight, bias, d_wt, qm_wt, t_wt, d_act, qm_act, t_act):
        ctx.module, ctx.plan = module, plan
        ctx.save_for_backward(input_, weight)
        return module._forward_plan(input_, plan)

    @staticmethod
    def backward(ctx, grad_output):
        input_, weight = ctx.saved_tensors
        grads = ctx.module._backward_plan(ctx.plan, input_, weight, grad_output, tuple(ctx.needs_input_grad[2:]))
        return (None, None) + grads


def initialize_quant_layer(layer, num_bits: int = 16,
                           quant_type: QuantizationType = QuantizationType.SYMMETRIC_LINEAR,
                           quant_mode: QuantizationMode = QuantizationMode.WEIGHT_ONLY) -> None:
    """quant_layers.py:413-440: q_m = max|W|, d = q_m / (2^(b-1) - 1), t = 1; the activation
    parameters start from the same weight statistics (:436-438)."""
    if not isinstance(layer, (QuantizeConv2d, QuantizeLinear)):
        return
    num_bits = float(num_bits)
    t_quant_init = 1.0
    q_s = torch.tensor(0.0, device=layer.weight.device)
    qm_quant_init = torch.max(torch.abs(layer.weight))
    d_quant_init = (qm_quant_init - q_s) / (2 ** (num_bits - 1) - 1)
    nn.init.constant_(layer.d_quant_wt, d_quant_init)
    nn.init.constant_(layer.q_m_wt, qm_quant_init)
    if quant_type == QuantizationType.SYMMETRIC_NONLINEAR:
        nn.init.constant_(layer.t_quant_wt, t_quant_init)
    if quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION:
        nn.init.constant_(layer.d_quant_act, d_quant_init)
        nn.init.constant_(layer.q_m_act, qm_quant_init)
        if quant_type == QuantizationType.SYMMETRIC_NONLINEAR:
            nn.init.constant_(layer.t_quant_act, t_quant_init)
    layer.invalidate()


class QuantizeLinear(nn.Linear, QuantizeMixin):
    """quant_layers.py:443-499."""

    def __init__(self, in_features, out_features, bias=True, d_quant_init=1.0, t_quant_init=1.0, q_m_init=1.0,
                 quant_type=QuantizationType.SYMMETRIC_LINEAR, quant_mode=QuantizationMode.WEIGHT_ONLY):
        nn.Linear.__init__(self, in_features, out_features, bias)
        self.init_quantization(d_quant_init, t_quant_init, q_m_init, quant_type, quant_mode)

    @staticmethod
    def from_module(module=None, d_quant_init=1.0, t_quant_init=1.0, q_m_init=1.0,
                    quant_type=QuantizationType.SYMMETRIC_LINEAR, quant_mode=QuantizationMode.WEIGHT_ONLY,
                    quant_init_by_module=True, num_bits=8):
        q = QuantizeLinear(in_features=module.in_features, out_features=module.out_features,
                           bias=module.bias is not None, d_quant_init=d_quant_init, t_quant_init=t_quant_init,
                           q_m_init=q_m_init, quant_type=quant_type, quant_mode=quant_mode)
        q = q.to(device=module.weight.device)
        q.weight.data.copy_(module.weight.data)
        if module.bias is not None:
            q.bias.data.copy_(module.bias.data)
        if quant_init_by_module:
            initialize_quant_layer(q, num_bits=num_bits, quant_type=quant_type, quant_mode=quant_mode)
        return q

    def forward(self, input_: torch.Tensor) -> torch.Tensor:
        self._check_input(input_)
        plan = self.quant_plan()
        if self._records_grad(input_):
            return self._forward_autograd(input_, plan)
        return self._forward_plan(input_, plan)

    def _gemm_grads(self, plan, xshape, x_q, w_q, G):
        G2 = G.reshape(-1, plan.n)
        grad_xq = torch.mm(G2, w_q.reshape(plan.n, plan.k)) if w_q is not None else None
        grad_wq = torch.mm(G2.t(), x_q.reshape(-1, plan.k)) if x_q is not None else None
        return grad_xq, grad_wq

    def _backward_gemm_routes(self, plan, need_xq, need_wq):
        ops = _backward_gemm_ops()
        has_codes = plan.int_path or bool(plan.extra.get("wonly"))
        return (need_xq and "dgrad" in ops and has_codes,
                need_wq and "wgrad" in ops and plan.int_path)

    def _gemm_grads_hip(self, plan, xf, x_q, w_q, G, hip_x, hip_w):
        G2 = G.reshape(-1, plan.n)
        M = G2.shape[0]
        grad_xq, grad_wq = self._gemm_grads(plan, tuple(xf.shape), None if hip_w else x_q, None if hip_x else w_q, G)
        if hip_x:
            grad_xq = self._dgrad_hip(plan, G2)
        if hip_w:
            # G^T @ (d_act codes): the int8 codes the forward contracted (the same quant_code)
            x2 = xf.reshape(-1, plan.k)
            grad_wq = _lib.gemm_wgrad(G2, self._act_codes(x2, plan), plan.k, plan.d_act)
        return grad_xq, grad_wq

    def _backward_preop(self, plan: QuantPlan, eps: Optional[float], x: torch.Tensor, gamma, beta,
                        weight: torch.Tensor, codes: torch.Tensor, G: torch.Tensor, needs: tuple) -> tuple:
        """Backward of _PreOpLinearFunction: gradients for (x, gamma, beta, weight, bias, d_quant_wt, q_m_wt,
        t_quant_wt, d_quant_act, q_m_act, t_quant_act); None where `needs` is false (that work is skipped). The
        pre-op is LayerNorm (eps given) or GELU (eps None); `codes` are the forward's activation codes."""
        need_x, need_g, need_bt, need_w, need_b = needs[:5]
        need_wq = need_w or any(needs[5:8])                        # wgrad and the weight quantizer's backward run
        need_pre = need_x or need_g or need_bt or any(needs[8:11])   # dgrad and the fused pre-op backward run
        G2 = G.detach().float().reshape(-1, plan.n).contiguous()
        grad_b = G2.sum(0).to(self.bias.dtype) if need_b else None
        quantizers = []   # (which, device scalars), in the order of _backward_plan
        grad_x = grad_g = grad_bt = None
        if need_pre:
            grad_xq = self._dgrad_hip(plan, G2)
            x2 = x.detach().reshape(-1, plan.k)
            qargs = (*plan.act_q, self.act_clip_val[0], self.act_clip_val[1])
            if eps is not None:
                grad_x, grad_g, grad_bt, scal = _lib.layernorm_quant_backward(
                    x2, gamma.detach(), beta.detach(), eps, *qargs, grad_y=grad_xq, grad_x=grad_xq,
                    want_gamma=need_g, want_beta=need_bt)
            else:
                grad_x, scal = _lib.gelu_quant_backward(x2, grad_xq, *qargs, grad_h=grad_xq)
            quantizers.append(("act", scal))
        grad_w = None
        if need_wq:
            grad_wq = _lib.gemm_wgrad(G2, codes, plan.k, plan.d_act)
            wf = weight.detach().float().contiguous()
            grad_w, scal = _lib.quant_backward(wf, grad_wq, *plan.wt_q, self.weight_clip_val[0],
                                               self.weight_clip_val[1], grad_x=grad_wq)
            quantizers.append(("wt", scal))
        scalars = self._checked_scalars(plan, quantizers)
        return (grad_x.view_as(x).to(x.dtype) if need_x else None,
                grad_g.to(gamma.dtype) if need_g else None,
                grad_bt.to(beta.dtype) if need_bt else None,
                grad_w.view_as(weight).to(weight.dtype) if need_w else None,
                grad_b) + self._scalar_grads(scalars, needs[5:11])

    def _forward_plan(self, input_: torch.Tensor, plan: QuantPlan) -> torch.Tensor:
        if plan.int_path:
            x2 = input_.detach().reshape(-1, plan.k)
            if x2.dtype != torch.float32 or x2.stride(-1) != 1:
                x2 = x2.float().contiguous()
            codes = self._act_codes(x2, plan)
            trace_codes(self, codes, plan.k)
            out = self.gemm_codes(codes, plan, _lib.EPI_F32)
            if out.shape[1] != plan.n:
                out = out[:, :plan.n].contiguous()
            return out.view(*input_.shape[:-1], plan.n)
        if plan.extra.get("wonly"):
            x = self.quantize_act(input_.float()) if self.quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION \
                else input_
            y = self._wonly_rows(x.detach().reshape(-1, plan.k), plan)
            return y.reshape(*input_.shape[:-1], plan.n)
        x = self.quantize_act(input_.float()) if self.quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION \
            else input_.float()
        return F.linear(x.detach(), self.w_fakequant(plan), None if self.bias is None else self.bias.detach())


# ---- train-time fusion: LayerNorm / GELU feeding a QuantizeLinear as one autograd node -------------------------
# layer(norm(x)) and layer(gelu(h)) under autograd, without the fp32 tensor between the two modules: the forward
# writes the layer's int8 activation codes straight from the pre-op's input (qvit_layernorm_quant_i8 /
# qvit_gelu_quant_i8, the kernels of the inference pipeline) and keeps them for wgrad; the backward runs dgrad,
# then one kernel for quantizer backward + pre-op backward (qvit_layernorm_quant_backward /
# qvit_gelu_quant_backward). The codes come from the kernels' own LayerNorm / GELU values, which can differ from
# torch's in the last bit, so a code at a rounding tie can differ from the modules route's.
def _preop_plan(layer) -> Optional[QuantPlan]:
    """The layer's plan if the fused nodes can run it: integer-path QuantizeLinear, weight + activation mode,
    linear or nonlinear quantizer, both backward GEMMs on the HIP kernels."""
    if not isinstance(layer, QuantizeLinear) or layer.quant_mode != QuantizationMode.WEIGHT_AND_ACTIVATION:
        return None
    if layer.quant_type not in (QuantizationType.SYMMETRIC_LINEAR, QuantizationType.SYMMETRIC_NONLINEAR):
        return None
    if set(_backward_gemm_ops()) != {"dgrad", "wgrad"}:
        return None
    plan = layer.quant_plan()
    return plan if plan.int_path and plan.k % 4 == 0 else None


class _PreOpLinearFunction(torch.autograd.Function):
    """codes = quantize(pre(x)); out = contraction(codes): pre = LayerNorm (eps given) or GELU (eps None). Saves
    the pre-op's input and the int8 codes."""

    @staticmethod
    def forward(ctx, layer, plan, eps, x, gamma, beta, weight, bias, d_wt, qm_wt, t_wt, d_act, qm_act, t_act):
        x2 = x.detach().reshape(-1, plan.k)
        M = x2.shape[0]
        codes = torch.empty((M, plan.kpad), dtype=torch.int8, device=x2.device)
        if eps is not None:
            _lib.layernorm_quant_i8(x2, gamma.detach(), beta.detach(), eps, *plan.act_q, 0, codes, plan.kpad)
        else:
            _lib.gelu_quant_i8(x2, *plan.act_q, 0, codes, plan.kpad)
        trace_codes(layer, codes, plan.k)
        out = layer.gemm_codes(codes, plan, _lib.EPI_F32)
        if out.shape[1] != plan.n:
            out = out[:, :plan.n].contiguous()
        ctx.layer, ctx.plan, ctx.eps = layer, plan, eps
        ctx.save_for_backward(x, gamma, beta, weight, codes)
        return out.view(*x.shape[:-1], plan.n)

    @staticmethod
    def backward(ctx, grad_output):
        x, gamma, beta, weight, codes = ctx.saved_tensors
        grads = ctx.layer._backward_preop(ctx.plan, ctx.eps, x, gamma, beta, weight, codes, grad_output,
                                          tuple(ctx.needs_input_grad[3:]))
        return (None, None, None) + grads


def _preop_apply(layer, plan, eps, x, gamma, beta):
    g = lambda n: getattr(layer, n, None)
    return _PreOpLinearFunction.apply(layer, plan, eps, x, gamma, beta, layer.weight, layer.bias, g("d_quant_wt"),
                                      g("q_m_wt"), g("t_quant_wt"), g("d_quant_act"), g("q_m_act"),
                                      g("t_quant_act"))


def _preop_input_ok(x: torch.Tensor, plan: QuantPlan) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2 and x.shape[-1] == plan.k
            and x.numel() > 0 and x.is_contiguous() and x.data_ptr() % 16 == 0)


def layernorm_linear(norm: nn.LayerNorm, layer: "QuantizeLinear", x: torch.Tensor) -> torch.Tensor:
    """layer(norm(x)). With autograd live and an eligible pair (see _preop_plan; an affine LayerNorm over the last
    dimension; the alignment rules of qvit_layernorm_quant_backward) this is one autograd node that never forms
    norm(x) in fp32; otherwise the two modules are composed as they are."""
    plan = _preop_plan(layer) if torch.is_grad_enabled() else None
    if (plan is not None and isinstance(norm, nn.LayerNorm) and norm.elementwise_affine and norm.bias is not None
            and tuple(norm.normalized_shape) == (plan.k,) and _preop_input_ok(x, plan)
            and (_autograd_live(layer, x) or _autograd_live(norm, x))
            and _lib.layernorm_quant_backward_fits(x.detach().reshape(-1, plan.k), norm.weight.detach(),
                                                   norm.bias.detach())):
        return _preop_apply(layer, plan, float(norm.eps), x, norm.weight, norm.bias)
    return layer(norm(x))


def gelu_linear(layer: "QuantizeLinear", h: torch.Tensor, act: Optional[nn.Module] = None) -> torch.Tensor:
    """layer(gelu(h)) for the exact GELU (`act`, when given, must be nn.GELU(approximate="none")), as one autograd
    node when the pair is eligible (see layernorm_linear); otherwise the modules are composed as they are."""
    exact = act is None or (isinstance(act, nn.GELU) and act.approximate == "none")
    plan = _preop_plan(layer) if torch.is_grad_enabled() and exact else None
    if plan is not None and _preop_input_ok(h, plan) and _autograd_live(layer, h):
        return _preop_apply(layer, plan, None, h, None, None)
    return layer(F.gelu(h) if act is None else act(h))


class QuantizeConv2d(nn.Conv2d, QuantizeMixin):
    """quant_layers.py:502-587."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=1, dilation=1, groups=1,
                 bias=False, d_quant_init=1.0, t_quant_init=1.0, q_m_init=1.0,
                 quant_type=QuantizationType.SYMMETRIC_LINEAR, quant_mode=QuantizationMode.WEIGHT_ONLY):
        nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups,
                           bias=bias)
        self.init_quantization(d_quant_init, t_quant_init, q_m_init, quant_type, quant_mode)
        self._u8_input = None   # (mean, std) of set_uint8_input

    @staticmethod
    def from_module(module=None, d_quant_init=1.0, t_quant_init=1.0, q_m_init=1.0,
                    quant_type=QuantizationType.SYMMETRIC_LINEAR, quant_mode=QuantizationMode.WEIGHT_ONLY,
                    quant_init_by_module=True, num_bits=8):
        q = QuantizeConv2d(in_channels=module.in_channels, out_channels=module.out_channels,
                           kernel_size=module.kernel_size, stride=module.stride, padding=module.padding,
                           dilation=module.dilation, groups=module.groups, bias=module.bias is not None,
                           d_quant_init=d_quant_init, t_quant_init=t_quant_init, q_m_init=q_m_init,
                           quant_type=quant_type, quant_mode=quant_mode)
        q = q.to(device=module.weight.device)
        q.weight.data.copy_(module.weight.data)
        if module.bias is not None:
            q.bias.data.copy_(module.bias.data)
        if quant_init_by_module:
            initialize_quant_layer(q, num_bits=num_bits, quant_type=quant_type, quant_mode=quant_mode)
        return q

    def _int_conv_ok(self) -> bool:
        return (self.groups == 1 and self.padding_mode == "zeros" and not isinstance(self.padding, str))

    _codes_forward_ok = _int_conv_ok

    # -- uint8 image input: ToTensor + Normalize (predict.py:18-19) and quantize_act as tables of 256 entries --------
    def set_uint8_input(self, mean, std) -> None:
        """From now on a torch.uint8 input [B, C, H, W] (contiguous, or channels_last: a decoder's [B, H, W, C]
        seen through permute) stands for the fp32 image (input / 255 - mean_c) / std_c, torchvision's ToTensor then
        Normalize, every step rounded to fp32. `mean` and `std` are a scalar or one value per input channel. The
        result equals forward() on that fp32 image bit for bit; a float input is taken as already normalised. The
        setting is a plain attribute: it is not part of state_dict()."""
        C = self.in_channels
        if C > _lib.U8_MAX_C:
            raise ValueError(f"uint8 input takes at most {_lib.U8_MAX_C} input channels, this layer has {C}")

        def per_channel(v, name):
            vals = torch.as_tensor(v, dtype=torch.float64).detach().cpu().reshape(-1)
            if vals.numel() == 1 and not isinstance(v, (tuple, list)):
                vals = vals.expand(C)
            if vals.numel() != C:
                raise ValueError(f"{name}: {vals.numel()} values for {C} input channels")
            vals = vals.to(torch.float32)   # as the table will hold them
            if not bool(torch.isfinite(vals).all()):
                raise ValueError(f"{name} must be finite, got {v!r}")
            return tuple(vals.tolist())

        mean, std = per_channel(mean, "mean"), per_channel(std, "std")
        if any(s == 0.0 for s in std):
            raise ValueError(f"std must not be zero, got {std!r}")
        self._u8_input = (mean, std)

    def clear_uint8_input(self) -> None:
        self._u8_input = None

    @property
    def uint8_input(self):
        """(mean, std), each a tuple of in_channels floats, or None."""
        return getattr(self, "_u8_input", None)

    def _u8_tables(self, plan: QuantPlan):
        """(V, T) on the device for the current setting, kept with the plan: V fp32 [C, 256], the normalised value
        of every byte; T int8 [C, 256] = the layer's activation codes of V through qvit_quantize_act_i8, the
        quant_code every other producer of codes runs (None off the integer path)."""
        key = self.uint8_input
        cached = plan.extra.get("u8_tables")
        if cached is not None and cached[0] == key:
            return cached[1], cached[2]
        mean, std = (torch.tensor(v, dtype=torch.float32) for v in key)
        V = ((torch.arange(256, dtype=torch.float32).div(255)[None, :] - mean[:, None]) / std[:, None]) \
            .contiguous().to(plan.device)
        T = None
        if plan.int_path:
            T = torch.empty((V.shape[0], 256), dtype=torch.int8, device=plan.device)
            _lib.quantize_act_i8(V, *plan.act_q, 0, T, 256)
        plan.extra["u8_tables"] = (key, V, T)
        return V, T

    def conv_codes_gemm(self, input_: torch.Tensor, epilogue: int = _lib.EPI_F32):
        """im2col + quantize + contraction. Returns ([B*OH*OW, Cout] NHWC rows, (B, OH, OW))."""
        plan = self.quant_plan()
        x = input_.detach()
        u8 = x.dtype == torch.uint8 and self.uint8_input is not None
        if not u8 and (x.dtype != torch.float32 or not x.is_contiguous()):
            x = x.float().contiguous()
        B, C, H, W = x.shape
        kh, kw = self.kernel_size
        sh, sw = self.stride
        ph, pw = self.padding
        dh, dw = self.dilation
        OH, OW = _lib.conv_out_hw(H, W, self.kernel_size, self.stride, self.padding, self.dilation)
        codes = torch.empty((B * OH * OW, plan.kpad), dtype=torch.int8, device=x.device)
        if u8:
            _lib.im2col_u8_i8(x, kh, kw, sh, sw, ph, pw, dh, dw, self._u8_tables(plan)[1], codes, plan.kpad)
        else:
            _lib.im2col_quant_i8(x, kh, kw, sh, sw, ph, pw, dh, dw, *plan.act_q, 0, codes, plan.kpad)
        trace_codes(self, codes, plan.k)
        out = self.gemm_codes(codes, plan, epilogue)
        return out, (B, OH, OW)

    def forward(self, input_: torch.Tensor) -> torch.Tensor:
        self._check_input(input_)
        plan = self.quant_plan()
        live = self._records_grad(input_)
        if input_.dtype == torch.uint8 and self.uint8_input is not None and \
                (live or not (plan.int_path and self._int_conv_ok())):
            # every route but the integer path reads fp32 (and the autograd node saves it): the normalised image
            input_ = _lib.u8_normalize_f32(input_, self._u8_tables(plan)[0])
        if live:
            return self._forward_autograd(input_, plan)
        return self._forward_plan(input_, plan)

    def _gemm_grads(self, plan, xshape, x_q, w_q, G):
        need_xq, need_wq = w_q is not None, x_q is not None
        if isinstance(self.padding, str) or self.padding_mode != "zeros":
            # paddings torch.nn.grad does not take: differentiate the library convolution itself
            with torch.enable_grad():
                xin = (x_q if need_wq else torch.zeros(xshape, device=G.device)).detach().requires_grad_(need_xq)
                win = (w_q if need_xq else torch.zeros_like(self.weight, dtype=torch.float32)).detach() \
                    .requires_grad_(need_wq)
                y = self._conv_forward(xin, win, None)
                got = list(torch.autograd.grad(y, [t for t in (xin, win) if t.requires_grad], G))
            grad_xq = got.pop(0).contiguous() if need_xq else None
            grad_wq = got.pop(0).contiguous() if need_wq else None
            return grad_xq, grad_wq
        args = (self.stride, self.padding, self.dilation, self.groups)
        grad_xq = torch.nn.grad.conv2d_input(xshape, w_q, G, *args).contiguous() if need_xq else None
        grad_wq = torch.nn.grad.conv2d_weight(x_q, tuple(self.weight.shape), G, *args).contiguous() \
            if need_wq else None
        return grad_xq, grad_wq

    def _taps_overlap(self) -> bool:
        """Whether two kernel taps can reach the same input element (a stride below the dilated kernel extent on an
        axis): the patch rows then hold kh kw / (sh sw) times the image."""
        return any(s < d * (k - 1) + 1 for k, s, d in zip(self.kernel_size, self.stride, self.dilation))

    def _backward_gemm_routes(self, plan, need_xq, need_wq):
        ops = _conv_backward_gemm_ops(self._taps_overlap())
        if not self._int_conv_ok() or not plan.has_codes:
            return False, False   # groups, padding modes and levels the kernels do not take: the library, as before
        has_codes = plan.int_path or bool(plan.extra.get("wonly"))
        return need_xq and "dgrad" in ops and has_codes, need_wq and "wgrad" in ops and plan.int_path

    def _grad_out_layout(self, G, library_op):
        # the kernels read the [B OH OW, N] row view: a channels-last gradient (behind PatchEmbed's flatten +
        # transpose) already is one, and only torch's convolutions get the NCHW copy
        return G.contiguous() if library_op else G

    def _gemm_grads_hip(self, plan, xf, x_q, w_q, G, hip_x, hip_w):
        grad_xq, grad_wq = self._gemm_grads(plan, tuple(xf.shape), None if hip_w else x_q, None if hip_x else w_q, G)
        G2 = G.permute(0, 2, 3, 1).reshape(-1, plan.n)   # a view of a channels-last G, else the one transposing copy
        if G2.stride(1) != 1 or G2.stride(0) < plan.n:
            # reshape merged the strides into something that is not row-major rows (an expanded gradient, as
            # sum().backward() hands over, has strides (0, 0); a strided view keeps its inner stride): the kernels
            # take a row stride only, so such a G is copied, as _backward_plan's contiguous() did for it before
            G2 = G2.contiguous()
        geometry = (self.kernel_size, self.stride, self.padding, self.dilation)
        act_done = ()
        if hip_x:
            # P = G2 @ (d_wt k_w), then col2im; on a W+A layer the same pass applies quantize_act's backward
            P = self._dgrad_hip(plan, G2)
            if self.quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION:
                grad_xq, scal = _lib.col2im_quant_backward(P, xf, xf.shape, *geometry, *plan.act_q, *self.act_clip_val)
                act_done = (scal,)
            else:
                grad_xq, _ = _lib.col2im_quant_backward(P, None, xf.shape, *geometry)
        if hip_w:
            # G2^T @ (d_act codes): the forward's own im2col kernel recomputes the codes it contracted
            (kh, kw), (sh, sw), (ph, pw), (dh, dw) = geometry
            codes = torch.empty((G2.shape[0], plan.kpad), dtype=torch.int8, device=xf.device)
            _lib.im2col_quant_i8(xf, kh, kw, sh, sw, ph, pw, dh, dw, *plan.act_q, 0, codes, plan.kpad)
            grad_wq = _lib.gemm_wgrad(G2, codes, plan.k, plan.d_act).view(self.weight.shape)
        return (grad_xq, grad_wq) + act_done

    def _forward_plan(self, input_: torch.Tensor, plan: QuantPlan) -> torch.Tensor:
        if plan.int_path and self._int_conv_ok():
            out, (B, OH, OW) = self.conv_codes_gemm(input_)
            n = plan.n
            return out[:, :n].reshape(B, OH, OW, n).permute(0, 3, 1, 2).contiguous()
        x = self.quantize_act(input_.float()) if self.quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION \
            else input_.float()
        if plan.extra.get("wonly") and self._int_conv_ok():
            # weight-only / wide levels: an implicit GEMM of the NCHW input against the packed codes
            # (qvit_conv_wonly: patches gathered in the kernel, NCHW out)
            return _lib.conv_wonly(x.detach(), self.kernel_size, self.stride, self.padding, self.dilation,
                                   plan.packed, plan.wfmt, plan.n, plan.npad, plan.kpad, plan.d_wt, plan.bias_pad)
        w = self.w_fakequant(plan).view_as(self.weight)
        return F.conv2d(x.detach(), w, None if self.bias is None else self.bias.detach(), self.stride,
                        self.padding, self.dilation, self.groups)


LAYER_TO_QUANTLAYER = {"Linear": QuantizeLinear, "Conv2d": QuantizeConv2d}
