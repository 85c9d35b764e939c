"""Vision Transformer caller of the quantized path — mirrors QViT_with_GETA/vit_model.py.

Same classes, constructor arguments, attribute names and state_dict keys as the reference
(PatchEmbed 46-103, ViTAttention 106-153, Mlp 156-177, Block 180-208, VisionTransformer 211-328,
_init_vit_weights 331-346, factories 351-483), so reference checkpoints / state_dicts load as-is and
model_to_quantize_model swaps the same 50 layers (ViT-B/16).

When every GEMM site is a QuantizeLinear / QuantizeConv2d on its integer path and the input is on
a ROCm device, forward() runs the fused MI355X pipeline per block (one residual buffer, updated in
place by the GEMM epilogues):
    LayerNorm+act-quant -> qkv projection + attention + proj's act-quant in one kernel
    (qvit_qkv_attention, N <= 208; longer sequences: qkv GEMM to fp16 hi/lo head planes -> streaming
    attention) -> proj GEMM (+= residual) -> LayerNorm+act-quant -> fc1 GEMM with GELU and fc2's
    act-quant fused (int8 codes out) -> fc2 GEMM (+= residual)
Otherwise each module runs on its own (still the HIP kernels for every quantized layer). That is also the
route when the call records autograd history (gradients enabled and the input or a parameter requires grad):
the fused pipeline and the in-place token buffer have no backward, so every module runs on its own: the
quantized layers differentiate through quant_layers' autograd node and the attention core through _AttentionCore
(qvit_attention forward, qvit_attention_backward).
"""
from __future__ import annotations

from collections import OrderedDict
from contextlib import nullcontext
from functools import partial
from typing import Optional

import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import quant_layers as _ql
from .quant_layers import (QuantizationMode, QuantizeConv2d, QuantizeLinear, _autograd_live, epilogue_table,
                           trace_codes)

# The residual GEMMs (proj, fc2) run the following LayerNorm + quantizer behind their tiles (qvit_gemm_resid_ln)
# instead of as a separate launch when QVIT_FUSE_LN=1 (or FUSE_RESID_LN = True). Off by default: the fused
# form is bit-identical but measured slower (the LayerNorm of a 128-row block
# runs on the one workgroup that completes the block and stalls its tile pipeline).
FUSE_RESID_LN = os.environ.get("QVIT_FUSE_LN", "0") == "1"
# fc1 on the weight-stationary schedule (norm2 writes QVIT_ACT_T32 codes, qvit_gemm_a32) instead of the tile
# schedule when QVIT_FC1_A32=1 (or FC1_WEIGHT_STATIONARY = True). Off by default: bit-identical, faster on
# full-range random codes but 2-3 % slower on the model's own activations, and its LayerNorm 4 % slower
# (profiles/r05_fc1_weight_stationary_ab.txt).
FC1_WEIGHT_STATIONARY = os.environ.get("QVIT_FC1_A32", "0") == "1"
# Under autograd, a Block runs norm1 -> qkv, norm2 -> fc1 and GELU -> fc2 as one autograd node each
# (quant_layers.layernorm_linear / gelu_linear: no fp32 LayerNorm / GELU output is formed or saved, the backward is
# one fused HIP kernel per site) when QVIT_TRAIN_FUSE=1 (or TRAIN_FUSE = True). Off by default: the fused forward
# quantizes the kernels' own LayerNorm / GELU values, which can differ from torch's in the last bit, so a code at a
# rounding tie can differ from the modules route's.
TRAIN_FUSE = os.environ.get("QVIT_TRAIN_FUSE", "0") == "1"
# The heads read only the class (and distillation) token rows of the last block, and everything after its attention
# is row-independent, so the last fused block computes only those rows: qvit_qkv_attention_q (all keys and values, the
# first num_tokens queries), then proj, norm2, fc1 and fc2 at M = B * num_tokens. The logits are bit-identical. On by
# default; QVIT_CLS_PRUNE=0 (or LAST_BLOCK_CLS_ONLY = False) runs the whole last block, for A/B runs. Off while codes
# are traced (quant_layers.CODE_TRACE), so parity reports keep seeing every row of every layer.
LAST_BLOCK_CLS_ONLY = os.environ.get("QVIT_CLS_PRUNE", "1") != "0"

# Benchmark instrumentation: when KERNEL_TIMING[name] is a list (name in "fc1", "fc2", "proj",
# "qkv_attn", "ln"), the fused block appends a (start, end) HIP event pair recorded on the launch
# stream (torch's current stream, which every _lib entry point launches on) around each such launch.
# The class-token launches of the last block (LAST_BLOCK_CLS_ONLY) do other work per launch, so they are recorded
# under names of their own ("qkv_attn_cls", "proj_cls", "ln_cls", "fc1_cls", "fc2_cls") and never under the above.
KERNEL_TIMING: dict = {}


class _timed:
    __slots__ = ("ev", "e0")

    def __init__(self, name: str):
        self.ev = KERNEL_TIMING.get(name)

    def __enter__(self):
        if self.ev is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if self.ev is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.ev.append((self.e0, e1))


def _code_buffer(rows: int, kpad: int, valid: int, device) -> torch.Tensor:
    """int8 [rows, kpad] for a kernel that writes the codes of columns < valid: the padding columns are zeroed here."""
    buf = torch.empty((rows, kpad), dtype=torch.int8, device=device)
    if kpad != valid:
        buf[:, valid:].zero_()
    return buf


def _ln_args(norm: nn.LayerNorm, p) -> tuple:
    """`norm` followed by plan p's activation quantizer, as the LayerNorm kernels' wrappers take them."""
    return (norm.weight, norm.bias, norm.eps, *p.act_q, 0)


def _ln_codes(norm: nn.LayerNorm, x2: torch.Tensor, p, name: str) -> torch.Tensor:
    """norm(x2) quantized for plan p -> fresh int8 codes [rows, p.kpad]; timed as `name` ("ln" or "ln_cls")."""
    codes = torch.empty((x2.shape[0], p.kpad), dtype=torch.int8, device=x2.device)
    with _timed(name):
        _lib.layernorm_quant_i8(x2, *_ln_args(norm, p), codes, p.kpad, code_table=epilogue_table(p, _lib.EPI_I8))
    return codes


def drop_path(x, drop_prob: float = 0., training: bool = False):
    """vit_model.py:14-30."""
    if drop_prob == 0. or not training:
        return x
    keep_prob = 1 - drop_prob
    shape = (x.shape[0],) + (1,) * (x.ndim - 1)
    random_tensor = keep_prob + torch.rand(shape, dtype=x.dtype, device=x.device)
    random_tensor.floor_()
    return x.div(keep_prob) * random_tensor


class DropPath(nn.Module):
    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        return drop_path(x, self.drop_prob, self.training)


class PatchEmbed(nn.Module):
    """vit_model.py:46-103."""

    def __init__(self, img_size=224, patch_size=16, in_c=3, embed_dim=768, norm_layer=None):
        super().__init__()
        img_size = (img_size, img_size)
        patch_size = (patch_size, patch_size)
        self.img_size = img_size
        self.patch_size = patch_size
        self.grid_size = (img_size[0] // patch_size[0], img_size[1] // patch_size[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.proj = nn.Conv2d(in_c, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer else nn.Identity()

    def forward(self, x):
        B, C, H, W = x.shape
        if not torch.jit.is_tracing():
            assert H == self.img_size[0] and W == self.img_size[1], \
                f"Input image size ({H}*{W}) doesn't match model ({self.img_size[0]}*{self.img_size[1]})."
        if _conv_int_path(self.proj, x) and not _autograd_live(self.proj, x):
            # im2col+quant -> GEMM rows are already (b, patch) x embed: no flatten/transpose copy
            out, (B, OH, OW) = self.proj.conv_codes_gemm(x)
            n = self.proj.quant_plan().n
            x = out[:, :n].reshape(B, OH * OW, n)
        else:
            x = self.proj(x).flatten(2).transpose(1, 2)
        x = self.norm(x)
        return x


def _pow2_scale(amax: float) -> float:
    """Power of two s with amax * s <= 16384 (the fp16 hi/lo split's range); 1 unless amax exceeds it."""
    return 1.0 if amax <= 16384.0 else 2.0 ** -math.ceil(math.log2(amax / 16384.0))


def _pow2_grad_scale(gmax: float) -> float:
    """qvit_attention_backward's g_scale: the largest power of two s with gmax * s <= 16384 (gradients are
    scaled up as well as down: 1e-8 would flush in the fp16 split), kept inside fp32's exponent range."""
    if not math.isfinite(gmax) or gmax == 0.0:
        return 1.0
    return 2.0 ** max(-100, min(100, 14 - math.ceil(math.log2(gmax))))


HIP_HEAD_DIMS = (64, 80)   # head sizes of qvit_attention (fp32 output) and qvit_attention_backward
ROUTE_FUSED, ROUTE_SPLIT, ROUTE_ATTENTION_I8, ROUTE_CORE = "fused", "split", "attention_i8", "core"   # fused_route


def _attention_core_forward(q2: torch.Tensor, B: int, N: int, H: int, scale: float, hd: int):
    """qvit_attention (fp32 out) on the [B*N, 3*H*hd] qkv projection. Returns (out, in_scale)."""
    out = torch.empty((B * N, H * hd), dtype=torch.float32, device=q2.device)
    amax = float(q2.abs().max()) if q2.numel() else 0.0   # unfused path: no plan bound, one sync
    in_scale = _pow2_scale(amax)
    _lib.attention(q2, B, N, H, hd, scale, out, _lib.ATT_F32, in_scale)
    return out, in_scale


class _AttentionCore(torch.autograd.Function):
    """ViTAttention.core on the HIP kernels under autograd: the forward is the no_grad call (same bits), the
    backward one qvit_attention_backward. Saves qkv and the output only: nothing of size N x N."""

    @staticmethod
    def forward(ctx, q2, B, N, H, scale, hd):
        q2 = q2.detach()
        if q2.stride(1) != 1 or q2.stride(0) % 4 or q2.data_ptr() % 16:
            q2 = q2.contiguous()
        out, in_scale = _attention_core_forward(q2, B, N, H, scale, hd)
        ctx.save_for_backward(q2, out)
        ctx.meta = (B, N, H, scale, in_scale, hd)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q2, out = ctx.saved_tensors
        B, N, H, scale, in_scale, hd = ctx.meta
        g = grad_out.detach()
        if g.dtype != torch.float32 or g.dim() != 2 or g.stride(1) != 1 or g.stride(0) % 4 or g.data_ptr() % 16:
            g = g.float().contiguous()
        gmax = float(g.abs().max()) if g.numel() else 0.0      # one sync, as in_scale in the forward
        g_scale = _pow2_grad_scale(gmax)
        dqkv = torch.empty((B * N, q2.shape[1]), dtype=torch.float32, device=q2.device)
        if q2.shape[1] > 3 * H * hd:
            dqkv[:, 3 * H * hd:] = 0
        _lib.attention_backward(q2, out, g, B, N, H, hd, scale, in_scale, g_scale, dqkv)
        return dqkv, None, None, None, None, None


class ViTAttention(nn.Module):
    """vit_model.py:106-153."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop_ratio=0., proj_drop_ratio=0.):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.head_dim = head_dim
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop_ratio)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop_ratio)

    def hip_ok(self, qkv: torch.Tensor) -> bool:
        return (qkv.is_cuda and qkv.dtype == torch.float32 and self.head_dim in HIP_HEAD_DIMS and qkv.dim() == 2
                and qkv.stride(1) == 1 and not (self.training and self.attn_drop.p > 0))

    def split_ok(self, p_qkv) -> bool:
        """The fused block can take the split-operand path (qvit_gemm_qkv_split -> qvit_attention_split)."""
        return (self.head_dim in (64, 80) and p_qkv.n == 3 * self.num_heads * self.head_dim
                and not (self.training and self.attn_drop.p > 0))

    def fused_route(self, p_qkv, N: int) -> str:
        """How the fused block gets from norm1's codes to proj's, for qkv plan `p_qkv` and N tokens:
          ROUTE_FUSED         qvit_qkv_attention (last block: qvit_qkv_attention_q), all in one kernel
          ROUTE_SPLIT         qvit_gemm_qkv_split (fp16 hi/lo head planes) -> qvit_attention_split
          ROUTE_ATTENTION_I8  qvit_gemm (fp32 qkv) -> qvit_attention writing proj's codes
          ROUTE_CORE          qvit_gemm (fp32 qkv) -> core() in fp32 -> proj's quantizer (qvit_quantize_act_i8)"""
        if self.split_ok(p_qkv):
            fused = (self.head_dim == 64 and N <= _lib.QKV_ATT_MAX_N and p_qkv.wfmt == _lib.W4
                     and p_qkv.kpad <= 65536 and p_qkv.kpad % 256 == 0 and self.num_heads * 64 <= _lib.QKV_ATT_MAX_C)
            return ROUTE_FUSED if fused else ROUTE_SPLIT
        # hip_ok(qkv) and head_dim == 64, ahead of the GEMM: its fp32 output is a fresh [M, >= n] device buffer with
        # unit column stride, so only hip_ok's conditions on the module are open (the chain asserts the rest)
        hip = self.head_dim == 64 and not (self.training and self.attn_drop.p > 0)
        return ROUTE_ATTENTION_I8 if hip else ROUTE_CORE

    def core_hip(self, qkv: torch.Tensor, B: int, N: int, out: torch.Tensor, out_mode: int = _lib.ATT_F32,
                 in_scale: float = 1.0, plan=None) -> torch.Tensor:
        """The same op on the fused HIP kernel (qvit_attention); with out_mode ATT_I8 it also applies the
        activation quantizer of `plan` (the proj layer) and writes its int8 codes (head_dim 64 only)."""
        out_q = plan.act_q if out_mode == _lib.ATT_I8 else ()
        return _lib.attention(qkv, B, N, self.num_heads, self.head_dim, self.scale, out, out_mode, in_scale, *out_q)

    def core(self, qkv: torch.Tensor, B: int, N: int) -> torch.Tensor:
        """softmax(q k^T * scale) v on the qkv projection (vit_model.py:133-149), fp32."""
        if self.hip_ok(qkv.reshape(B * N, -1)):
            if torch.is_grad_enabled() and qkv.requires_grad:   # same kernel, with qvit_attention_backward behind it
                return _AttentionCore.apply(qkv.reshape(B * N, -1), B, N, self.num_heads, self.scale,
                                            self.head_dim).reshape(B, N, -1)
            return _attention_core_forward(qkv.reshape(B * N, -1), B, N, self.num_heads, self.scale,
                                           self.head_dim)[0].reshape(B, N, -1)
        qkv = qkv.reshape(B, N, 3, self.num_heads, -1).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        attn = (q @ k.transpose(-2, -1)) * self.scale
        attn = attn.softmax(dim=-1)
        attn = self.attn_drop(attn)
        return (attn @ v).transpose(1, 2).reshape(B, N, -1)

    def forward(self, x):
        B, N, C = x.shape
        x = self.core(self.qkv(x), B, N)
        x = self.proj(x)
        x = self.proj_drop(x)
        return x


class Mlp(nn.Module):
    """vit_model.py:156-177."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        x = self.fc1(x)
        x = self.act(x)
        x = self.drop(x)
        x = self.fc2(x)
        x = self.drop(x)
        return x


def attention_in_scale(p_qkv) -> float:
    """Power of two that keeps the qkv projection (|x| <= its plan's output bound) inside the fp16
    range of the attention kernel's hi/lo split (qvit_attention's in_scale)."""
    bound = p_qkv.extra.get("out_bound", float("inf"))
    if bound <= 16384.0:
        return 1.0
    if not math.isfinite(bound):
        raise _lib.QvitError("qkv projection has no finite output bound; cannot size the attention input scale")
    return 2.0 ** -math.ceil(math.log2(bound / 16384.0))


def _qlinear_int(m: nn.Module) -> bool:
    return (isinstance(m, QuantizeLinear) and m.quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION
            and m.quant_plan().int_path)


def _conv_int_path(m: nn.Module, x: torch.Tensor) -> bool:
    return (isinstance(m, QuantizeConv2d) and x.is_cuda and m.quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION
            and m._int_conv_ok() and m.quant_plan().int_path)


def _inactive(m: nn.Module) -> bool:
    """Dropout / DropPath / Identity that does nothing in the current mode."""
    if isinstance(m, nn.Identity):
        return True
    if isinstance(m, nn.Dropout):
        return m.p == 0.0 or not m.training
    if isinstance(m, DropPath):
        return not m.drop_prob or not m.training
    return False


class Block(nn.Module):
    """vit_model.py:180-208."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop_ratio=0.,
                 attn_drop_ratio=0., drop_path_ratio=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = ViTAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                 attn_drop_ratio=attn_drop_ratio, proj_drop_ratio=drop_ratio)
        self.drop_path = DropPath(drop_path_ratio) if drop_path_ratio > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop_ratio)

    def fused_ok(self, x: torch.Tensor) -> bool:
        a, m = self.attn, self.mlp
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
                and not _autograd_live(self, x)
                and isinstance(self.norm1, nn.LayerNorm) and isinstance(self.norm2, nn.LayerNorm)
                and self.norm1.elementwise_affine and self.norm2.elementwise_affine
                and isinstance(m.act, nn.GELU) and m.act.approximate == "none"
                and _inactive(self.drop_path) and _inactive(a.attn_drop) and _inactive(a.proj_drop)
                and _inactive(m.drop)
                and all(_qlinear_int(l) for l in (a.qkv, a.proj, m.fc1, m.fc2)))

    def forward_fused_(self, x: torch.Tensor) -> torch.Tensor:
        """In-place fused block on a contiguous [B, N, C] fp32 residual buffer (owned by caller)."""
        return self.forward_fused_chain_(x)[0]

    def ln_fusable(self, x2: torch.Tensor, norm: nn.LayerNorm, p_res: QuantPlan) -> bool:
        """Whether the residual GEMM with plan p_res can run `norm` (+ the next quantizer) behind its tiles."""
        C = x2.shape[1]
        return (FUSE_RESID_LN and p_res.n == C and C % 4 == 0 and C <= 1024 and x2.stride(0) == C
                and x2.shape[0] * C * 4 < 2 ** 31 and norm.weight is not None and norm.bias is not None
                and norm.weight.is_contiguous() and norm.bias.is_contiguous())

    def resid_ln_(self, codes_in: torch.Tensor, p_res: QuantPlan, x2: torch.Tensor, norm: nn.LayerNorm,
                  p_next: QuantPlan) -> torch.Tensor:
        """x2 += layer(codes_in) (the proj / fc2 contraction), then norm(x2) quantized with p_next's activation
        quantizer -> int8 codes [M, p_next.kpad] (qvit_gemm_resid_ln: one launch)."""
        M, C = x2.shape
        out = torch.empty((M, p_next.kpad), dtype=torch.int8, device=x2.device)
        _lib.gemm_resid_ln(codes_in, M, p_res.kpad, p_res.packed_codes(), p_res.wfmt, p_res.n, p_res.npad, p_res.d_act,
                           p_res.d_wt, p_res.bias_pad, x2, *_ln_args(norm, p_next), epilogue_table(p_next, _lib.EPI_I8),
                           out, p_next.kpad)
        return out

    def _resid_gemm_(self, layer: QuantizeLinear, p: QuantPlan, codes: torch.Tensor, x2: torch.Tensor,
                     norm: Optional[nn.LayerNorm] = None, next_layer: Optional[QuantizeLinear] = None):
        """x2 += layer(codes) (proj / fc2, plan p). Given `norm` and ln_fusable (FUSE_RESID_LN), the same launch also runs
        norm + next_layer's activation quantizer on the new rows and its codes are returned; else None."""
        if norm is not None and self.ln_fusable(x2, norm, p):
            return self.resid_ln_(codes, p, x2, norm, next_layer.quant_plan())
        layer.gemm_codes(codes, p, _lib.EPI_F32_RESID, out=x2)
        return None

    def _cls_tail_(self, x: torch.Tensor, cls_codes: torch.Tensor, nt: int):
        """The rest of the last block (proj, norm2, fc1, fc2) on the first `nt` token rows of every image only:
        `cls_codes` [B*nt, >= proj.kpad] are proj's activation codes of those rows (any row stride). nt = 1 updates
        the class rows of the residual buffer in place through a strided view (row stride N*C) and returns x; nt > 1
        gathers the rows into a compact buffer and returns it as [B, nt, C]. The other rows of x are left as they
        were after the previous block: nothing downstream reads them."""
        B, N, C = x.shape
        a, m = self.attn, self.mlp
        p_proj, p_fc1, p_fc2 = a.proj.quant_plan(), m.fc1.quant_plan(), m.fc2.quant_plan()
        xc = x[:, 0] if nt == 1 else x[:, :nt].reshape(B * nt, C)
        with _timed("proj_cls"):
            self._resid_gemm_(a.proj, p_proj, cls_codes, xc)
        codes = _ln_codes(self.norm2, xc, p_fc1, "ln_cls")
        hid = _code_buffer(B * nt, p_fc2.kpad, p_fc1.n, x.device)
        with _timed("fc1_cls"):
            m.fc1.gemm_codes(codes, p_fc1, _lib.EPI_I8_GELU, out=hid, next_layer=m.fc2)
        with _timed("fc2_cls"):
            self._resid_gemm_(m.fc2, p_fc2, hid, xc)
        return (x if nt == 1 else xc.view(B, nt, C)), None

    def forward_fused_chain_(self, x: torch.Tensor, codes_in: Optional[torch.Tensor] = None,
                             next_block: Optional["Block"] = None, last: bool = False, num_tokens: int = 1):
        """The fused block in place on the residual buffer x: norm1's codes (`codes_in` when the previous block's fc2
        produced them, FUSE_RESID_LN), the attention launches of ViTAttention.fused_route (_attention_codes_), then one
        tail: proj into x and _mlp_fused_, whose fc2 can produce `next_block`'s norm1 codes. Returns (x, those or None).
        `last`: this is the model's last block and only the first `num_tokens` token rows of its output are read
        (LAST_BLOCK_CLS_ONLY): everything after the keys and values is computed for those rows only (_cls_tail_),
        and only they are valid in the returned x ([B, N, C] for num_tokens = 1, else [B, num_tokens, C])."""
        B, N, C = x.shape
        x2 = x.view(B * N, C)
        a = self.attn
        p_qkv = a.qkv.quant_plan()
        # x + attn(norm1(x))
        ln_codes = codes_in if codes_in is not None else _ln_codes(self.norm1, x2, p_qkv, "ln")
        trace_codes(a.qkv, ln_codes, C)   # (ln_codes is held to the end of the block: DESIGN.md section 4, lifetimes)
        p_proj = a.proj.quant_plan()
        route = a.fused_route(p_qkv, N)
        codes = self._attention_codes_(route, ln_codes, p_qkv, p_proj, B, N, last, num_tokens)
        if last:
            return self._cls_tail_(x, codes, num_tokens)
        # Known oddities: only the fused route's proj carries the "proj" timing events and may
        # run norm2 behind its tiles; on the other routes it is the plain GEMM whatever FUSE_RESID_LN says.
        fused = route == ROUTE_FUSED
        with _timed("proj") if fused else nullcontext():
            norm2_codes = self._resid_gemm_(a.proj, p_proj, codes, x2, norm=self.norm2 if fused else None,
                                            next_layer=self.mlp.fc1)
        return self._mlp_fused_(x, x2, norm2_codes, next_block)

    def _attention_codes_(self, route: str, codes: torch.Tensor, p_qkv: QuantPlan, p_proj: QuantPlan, B: int, N: int,
                          last: bool, num_tokens: int) -> torch.Tensor:
        """The qkv projection and the attention core on norm1's `codes` by `route`. Returns proj's activation codes, of
        every row or with `last` of the first `num_tokens` tokens of each image: compact from qvit_qkv_attention_q on
        the fused route; on the others the attention runs in full and the rows are a view of its codes."""
        a = self.attn
        M, dev = B * N, codes.device
        width = a.num_heads * a.head_dim   # proj's input columns; the rest of its kpad stays zero
        if route == ROUTE_FUSED:   # q/k/v stay on chip
            out = _code_buffer(B * num_tokens if last else M, p_proj.kpad, width, dev)
            in_scale, tab = attention_in_scale(p_qkv), epilogue_table(p_proj, _lib.EPI_I8)
            args = (p_qkv.kpad, p_qkv.packed_codes(), p_qkv.npad, p_qkv.d_act, p_qkv.d_wt, p_qkv.bias_pad,
                    a.num_heads, a.scale, out, _lib.ATT_I8, in_scale, *p_proj.act_q)
            if last:   # the wanted queries only; not traced (last is off while codes are traced)
                with _timed("qkv_attn_cls"):
                    _lib.qkv_attention_q(codes, B, N, num_tokens, *args, epi_table=tab)
                return out
            with _timed("qkv_attn"):
                _lib.qkv_attention(codes, B, N, *args, epi_table=tab)
        elif route == ROUTE_SPLIT:   # qkv as pre-scaled fp16 hi/lo head planes
            in_scale = attention_in_scale(p_qkv)
            hi = torch.empty(M * p_qkv.n, dtype=torch.float16, device=dev)
            lo = torch.empty(M * p_qkv.n, dtype=torch.float16, device=dev)
            wimg, wfmt = p_qkv.gemm_weights()
            _lib.gemm_qkv_split(codes, M, p_qkv.kpad, wimg, wfmt, p_qkv.n, p_qkv.npad, p_qkv.d_act,
                                p_qkv.d_wt, p_qkv.bias_pad, N, in_scale, hi, lo, head_dim=a.head_dim)
            out = _code_buffer(M, p_proj.kpad, width, dev)
            _lib.attention_split(hi, lo, B, N, a.num_heads, a.head_dim, a.scale, out, _lib.ATT_I8, in_scale,
                                 *p_proj.act_q, epi_table=epilogue_table(p_proj, _lib.EPI_I8))
        else:
            qkv = a.qkv.gemm_codes(codes, p_qkv, _lib.EPI_F32)[:, :p_qkv.n]
            if route == ROUTE_ATTENTION_I8:
                assert a.hip_ok(qkv), "fused_route chose qvit_attention for a qkv layout it cannot read"
                out = _code_buffer(M, p_proj.kpad, width, dev)
                a.core_hip(qkv, B, N, out, _lib.ATT_I8, attention_in_scale(p_qkv), p_proj)
            else:
                h = a.core(qkv, B, N).reshape(M, -1)
                out = a.proj._act_codes(h if h.is_contiguous() else h.contiguous(), p_proj)
        trace_codes(a.proj, out, p_proj.k)
        if last:   # the first num_tokens rows of every image of the full-M codes: a strided view (lda = N * kpad) for one
            c3 = out.view(B, N, out.shape[1])
            out = c3[:, 0] if num_tokens == 1 else c3[:, :num_tokens].reshape(B * num_tokens, out.shape[1])
        return out

    def _mlp_fused_(self, x: torch.Tensor, x2: torch.Tensor, codes_in: Optional[torch.Tensor] = None,
                    next_block: Optional["Block"] = None):
        """x + mlp(norm2(x)) in place on the residual buffer (codes_in: norm2's codes, from the proj GEMM).
        Returns (x, next_block's norm1 codes when fc2 produced them, else None)."""
        m = self.mlp
        p_fc1, p_fc2 = m.fc1.quant_plan(), m.fc2.quant_plan()
        hid = _code_buffer(x2.shape[0], p_fc2.kpad, p_fc1.n, x.device)
        if (FC1_WEIGHT_STATIONARY and codes_in is None and m.fc1.a32_fits(p_fc1, _lib.EPI_I8_GELU)
                and self.norm2.weight.is_contiguous()):
            self._fc1_weight_stationary_(x2, p_fc1, hid)
        else:
            codes = codes_in if codes_in is not None else _ln_codes(self.norm2, x2, p_fc1, "ln")
            trace_codes(m.fc1, codes, p_fc1.k)
            with _timed("fc1"):
                m.fc1.gemm_codes(codes, p_fc1, _lib.EPI_I8_GELU, out=hid, next_layer=m.fc2)
        trace_codes(m.fc2, hid, p_fc2.k)
        with _timed("fc2"):
            if next_block is None:
                return x, self._resid_gemm_(m.fc2, p_fc2, hid, x2)
            return x, self._resid_gemm_(m.fc2, p_fc2, hid, x2, norm=next_block.norm1, next_layer=next_block.attn.qkv)

    def _fc1_weight_stationary_(self, x2: torch.Tensor, p_fc1: QuantPlan, hid: torch.Tensor) -> None:
        """FC1_WEIGHT_STATIONARY: norm2 writes its codes in the MFMA operand order of qvit_gemm_a32 (every fragment load
        of that GEMM one contiguous KiB), which runs fc1 into `hid`."""
        m = self.mlp
        M = x2.shape[0]
        codes = torch.empty(_lib.t32_rows(M) * p_fc1.kpad, dtype=torch.int8, device=x2.device)
        with _timed("ln"):
            _lib.layernorm_quant_i8_t32(x2, *_ln_args(self.norm2, p_fc1), codes, p_fc1.kpad,
                                        code_table=epilogue_table(p_fc1, _lib.EPI_I8))
        if _ql.CODE_TRACE is not None:
            trace_codes(m.fc1, _lib.t32_to_rows(codes, M, p_fc1.kpad), p_fc1.k)
        with _timed("fc1"):
            m.fc1.gemm_codes_a32(codes, M, p_fc1, _lib.EPI_I8_GELU, hid, m.fc2)

    def forward_train_fused(self, x: torch.Tensor) -> torch.Tensor:
        """The modules route with the three LayerNorm / GELU -> QuantizeLinear sites as fused autograd nodes
        (TRAIN_FUSE); the attention core, the dropouts and the residual adds are the modules' own."""
        a, m = self.attn, self.mlp
        B, N, _ = x.shape
        y = a.core(_ql.layernorm_linear(self.norm1, a.qkv, x), B, N)
        x = x + self.drop_path(a.proj_drop(a.proj(y)))
        h = _ql.layernorm_linear(self.norm2, m.fc1, x)
        if _inactive(m.drop):   # nothing between GELU and fc2
            y = _ql.gelu_linear(m.fc2, h, m.act)
        else:
            y = m.fc2(m.drop(m.act(h)))
        return x + self.drop_path(m.drop(y))

    def forward(self, x):
        if self.fused_ok(x):
            return self.forward_fused_(x.contiguous().clone())
        if TRAIN_FUSE and x.dim() == 3 and _autograd_live(self, x):
            return self.forward_train_fused(x)
        x = x + self.drop_path(self.attn(self.norm1(x)))
        x = x + self.drop_path(self.mlp(self.norm2(x)))
        return x


class VisionTransformer(nn.Module):
    """vit_model.py:211-328."""

    def __init__(self, img_size=224, patch_size=16, in_c=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, representation_size=None,
                 distilled=False, drop_ratio=0., attn_drop_ratio=0., drop_path_ratio=0., embed_layer=PatchEmbed,
                 norm_layer=None, act_layer=None):
        super().__init__()
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.num_tokens = 2 if distilled else 1
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        act_layer = act_layer or nn.GELU
        self.patch_embed = embed_layer(img_size=img_size, patch_size=patch_size, in_c=in_c, embed_dim=embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.dist_token = nn.Parameter(torch.zeros(1, 1, embed_dim)) if distilled else None
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + self.num_tokens, embed_dim))
        self.pos_drop = nn.Dropout(p=drop_ratio)
        dpr = [x.item() for x in torch.linspace(0, drop_path_ratio, depth)]
        self.blocks = nn.Sequential(*[
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop_ratio=drop_ratio, attn_drop_ratio=attn_drop_ratio, drop_path_ratio=dpr[i],
                  norm_layer=norm_layer, act_layer=act_layer)
            for i in range(depth)
        ])
        self.norm = norm_layer(embed_dim)
        if representation_size and not distilled:
            self.has_logits = True
            self.num_features = representation_size
            self.pre_logits = nn.Sequential(OrderedDict([
                ("fc", nn.Linear(embed_dim, representation_size)),
                ("act", nn.Tanh())
            ]))
        else:
            self.has_logits = False
            self.pre_logits = nn.Identity()
        self.head = nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity()
        self.head_dist = None
        if distilled:
            self.head_dist = nn.Linear(self.embed_dim, self.num_classes) if num_classes > 0 else nn.Identity()
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        if self.dist_token is not None:
            nn.init.trunc_normal_(self.dist_token, std=0.02)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        self.apply(_init_vit_weights)

    def set_uint8_input(self, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)) -> None:
        """Lets forward() take the image as torch.uint8 [B, C, H, W] (contiguous or channels_last): the patch
        embedding then applies ToTensor + Normalize(mean, std) itself (QuantizeConv2d.set_uint8_input; the defaults
        are predict.py:19's). Needs the quantized model: the patch embedding must be a QuantizeConv2d."""
        proj = getattr(self.patch_embed, "proj", None)
        if not isinstance(proj, QuantizeConv2d):
            raise TypeError(f"set_uint8_input: patch_embed.proj is {type(proj).__name__}, not a QuantizeConv2d "
                            "(swap the model's layers with model_to_quantize_model first)")
        proj.set_uint8_input(mean, std)

    def forward_features(self, x):
        x = self.patch_embed(x)
        live = torch.is_grad_enabled() and (x.requires_grad or any(
            p is not None and p.requires_grad for p in (self.pos_embed, self.cls_token, self.dist_token)))
        if x.is_cuda and _inactive(self.pos_drop) and not live:
            # cat((cls[, dist], x)) + pos_embed in one pass: the token rows are written straight into the
            # residual buffer (the same fp32 additions as the reference's cat-then-add)
            B, T, C = x.shape
            nt = self.num_tokens
            buf = torch.empty((B, T + nt, C), dtype=x.dtype, device=x.device)
            torch.add(x, self.pos_embed[:, nt:], out=buf[:, nt:])
            buf[:, 0] = self.cls_token[:, 0] + self.pos_embed[:, 0]
            if self.dist_token is not None:
                buf[:, 1] = self.dist_token[:, 0] + self.pos_embed[:, 1]
            x = buf
        else:
            cls_token = self.cls_token.expand(x.shape[0], -1, -1)
            if self.dist_token is None:
                x = torch.cat((cls_token, x), dim=1)
            else:
                x = torch.cat((cls_token, self.dist_token.expand(x.shape[0], -1, -1), x), dim=1)
            x = self.pos_drop(x + self.pos_embed)
        # the residual stream is a fresh buffer here, so fused blocks may update it in place; a fused block's
        # fc2 also runs the next fused block's norm1 (+ its qkv quantizer)
        blocks = list(self.blocks)
        codes = None
        for i, blk in enumerate(blocks):
            if isinstance(blk, Block) and blk.fused_ok(x):
                nb = blocks[i + 1] if i + 1 < len(blocks) else None
                nb = nb if isinstance(nb, Block) and nb.fused_ok(x) else None
                # the last block: only the token rows the heads read (bit-identical; off while codes are traced)
                last = (LAST_BLOCK_CLS_ONLY and i + 1 == len(blocks) and _ql.CODE_TRACE is None
                        and not torch.is_grad_enabled() and x.shape[1] >= self.num_tokens)
                x, codes = blk.forward_fused_chain_(x.contiguous(), codes, nb, last=last,
                                                    num_tokens=self.num_tokens)
            else:
                codes = None
                x = blk(x)
        # LayerNorm is per token: only the class (and distillation) token rows reach the heads
        if self.dist_token is None:
            return self.pre_logits(self.norm(x[:, 0]))
        else:
            x = self.norm(x[:, :2])
            return x[:, 0], x[:, 1]

    def forward(self, x):
        x = self.forward_features(x)
        if self.head_dist is not None:
            x, x_dist = self.head(x[0]), self.head_dist(x[1])
            if self.training and not torch.jit.is_scripting():
                return x, x_dist
            else:
                return (x + x_dist) / 2
        else:
            x = self.head(x)
        return x


def _init_vit_weights(m):
    """vit_model.py:331-346."""
    if isinstance(m, nn.Linear):
        nn.init.trunc_normal_(m.weight, std=.01)
        if m.bias is not None:
            nn.init.zeros_(m.bias)
    elif isinstance(m, nn.Conv2d):
        nn.init.kaiming_normal_(m.weight, mode="fan_out")
        if m.bias is not None:
            nn.init.zeros_(m.bias)
    elif isinstance(m, nn.LayerNorm):
        nn.init.zeros_(m.bias)
        nn.init.ones_(m.weight)


# ---- factories (vit_model.py:351-483) -------------------------------------------------------------
def vit_base_patch16_224(num_classes: int = 1000):
    return VisionTransformer(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12,
                             representation_size=None, num_classes=num_classes)


def vit_base_patch16_224_in21k(num_classes: int = 21843, has_logits: bool = True):
    return VisionTransformer(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12,
                             representation_size=768 if has_logits else None, num_classes=num_classes)


def vit_base_patch32_224(num_classes: int = 1000):
    return VisionTransformer(img_size=224, patch_size=32, embed_dim=768, depth=12, num_heads=12,
                             representation_size=None, num_classes=num_classes)


def vit_base_patch32_224_in21k(num_classes: int = 21843, has_logits: bool = True):
    return VisionTransformer(img_size=224, patch_size=32, embed_dim=768, depth=12, num_heads=12,
                             representation_size=768 if has_logits else None, num_classes=num_classes)


def vit_large_patch16_224(num_classes: int = 1000):
    return VisionTransformer(img_size=224, patch_size=16, embed_dim=1024, depth=24, num_heads=16,
                             representation_size=None, num_classes=num_classes)


def vit_large_patch16_224_in21k(num_classes: int = 21843, has_logits: bool = True):
    return VisionTransformer(img_size=224, patch_size=16, embed_dim=1024, depth=24, num_heads=16,
                             representation_size=1024 if has_logits else None, num_classes=num_classes)


def vit_large_patch32_224_in21k(num_classes: int = 21843, has_logits: bool = True):
    return VisionTransformer(img_size=224, patch_size=32, embed_dim=1024, depth=24, num_heads=16,
                             representation_size=1024 if has_logits else None, num_classes=num_classes)


def vit_huge_patch14_224_in21k(num_classes: int = 21843, has_logits: bool = True):
    return VisionTransformer(img_size=224, patch_size=14, embed_dim=1280, depth=32, num_heads=16,
                             representation_size=1280 if has_logits else None, num_classes=num_classes)


def vit_tiny_patch16_224(num_classes: int = 1000):
    """ViT-Tiny/16 (BASELINE config 1; no reference factory — built from VisionTransformer(...))."""
    return VisionTransformer(img_size=224, patch_size=16, embed_dim=192, depth=12, num_heads=3,
                             representation_size=None, num_classes=num_classes)


def vit_large_patch16_384(num_classes: int = 1000):
    """ViT-L/16 @384 (BASELINE config 4; no reference factory — built from VisionTransformer(...))."""
    return VisionTransformer(img_size=384, patch_size=16, embed_dim=1024, depth=24, num_heads=16,
                             representation_size=None, num_classes=num_classes)
