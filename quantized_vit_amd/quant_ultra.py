"""Mirror of the reference's `4-bit quantization/quant_ultra.py` (DoReFa-style 4-bit quantizers of
UltraNet): same factory / class names and forward semantics, computed on the ROCm device.

  uniform_quantize(k)        quant_ultra.py:8-27   round(x * (2^k - 1)) / (2^k - 1)  (k = 1: sign, 32: identity)
  weight_quantize_fn(w_bit)  :30-56   tanh -> / max|tanh| -> (w_bit-1)-bit uniform quantizer (HIP codes)
  activation_quantize_fn     :59-73   clamp(x, 0, 1) -> a_bit uniform quantizer (HIP)
  conv2d_Q_fn(w_bit)         :76-91   Conv2d_Q: conv with quantized weights -- qvit_conv_wonly (implicit GEMM of the
                                      fp32 input against the int weight codes, d_w = 1/(2^(w_bit-1)-1); <= 64
                                      output channels: the narrow schedule); forward_bn_act fuses a following
                                      eval BatchNorm2d + activation_quantize_fn (qvit_conv_wonly_bn_act)
  linear_Q_fn(w_bit)         :210-222 Linear_Q -- qvit_gemm_wonly on the same codes
  batchNorm2d_Q_fn / batchNorm1d_Q_fn  :94-207 (not used by UltraNetQua; kept for API parity)

Conv2d_Q / Linear_Q with 2 <= w_bit <= 8 (UltraNet: 4) run on the hand-written kernels; their weight codes are
packed once per weight version. w_bit 32 (no quantization: a plain conv / linear) and w_bit 1 (the reference's
k = 0 quantizer divides by zero) keep the library call on the device, as do grouped or non-zero-padded convs.

The network-level fused path (conv + BN + quantizer + max pool on codes) is in ultranet.py; these
modules are the per-layer surface.

Training: under autograd every quantizer carries the reference's straight-through backward
(uniform_quantize.backward, quant_ultra.py:23-25). The forward stays the no_grad HIP call, bit for bit, with one
autograd node around it; the node's backward runs qvit_ultra_weight_quant_backward (tanh and max|.| behind the
straight-through rounding), qvit_ultra_act_quant_backward (the clamp mask), and for Conv2d_Q / Linear_Q the input
gradient as qvit_conv_wonly / qvit_gemm_wonly on the transposed (and, for a conv, flipped) codes and the weight
gradient as qvit_conv_wgrad when the caller states that the input holds activation codes (`in_levels`).
QVIT_ULTRA_BWD=hip|torch|dgrad|wgrad selects which of the two contractions run on these kernels (torch: both on
the library; the quantizer backwards stay in HIP).

QVIT_ULTRA_TRAIN_FUSE=1 (default 0) lets UltraNetQua.forward_modules run each training-mode
BatchNorm2d -> activation_quantize_fn (-> MaxPool2d(2, 2)) run as one node, bn_act_pool, on ultra_bn_fuse.hip.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


def _check_gpu(x: torch.Tensor, what: str) -> None:
    if not x.is_cuda:
        raise _lib.QvitError(f"{what} on {x.device}: the UltraNet path runs on a ROCm device (no CPU fallback)")


# The two contractions behind Conv2d_Q / Linear_Q's backward: "hip" runs the input gradient (dgrad) on
# qvit_conv_wonly / qvit_gemm_wonly and a conv's weight gradient (wgrad) on qvit_conv_wgrad; "torch" keeps both on
# the library (torch.nn.grad / torch.mm); "dgrad" / "wgrad" select one op. The quantizer backwards are HIP on every
# setting. Measured at 416 x 416 b64 only (profiles/ultra_train_bench.txt): qvit_conv_wgrad
# is slower than the library at every UltraNet layer shape, and the input gradient on qvit_conv_wonly is slower on
# maps of 104 x 104 and more, faster from 52 x 52 down. So under "hip" the ops named in ULTRA_BWD_DEFAULT_TORCH stay
# on the library and dgrad runs on HIP only where the conv's input (the gradient it produces) has at most
# DGRAD_HIP_MAX_PIXELS pixels per image: a cutoff between the two measured sizes, not measured at other batch
# sizes. Naming an op ("dgrad" / "wgrad") runs it on HIP at every shape.
ULTRA_BWD = os.environ.get("QVIT_ULTRA_BWD", "hip")
ULTRA_BWD_DEFAULT_TORCH = ("wgrad",)
DGRAD_HIP_MAX_PIXELS = 64 * 64
_lib.backward_ops(ULTRA_BWD, "QVIT_ULTRA_BWD")   # an unknown value stops the import


# "1": UltraNetQua.forward_modules routes BatchNorm2d (batch statistics) -> activation_quantize_fn -> MaxPool2d(2, 2)
# through bn_act_pool under autograd. Off by default: the fused y = fmaf(x - mean, gamma invstd, beta) is not ATen's
# batch-norm arithmetic bit for bit, so a code at a rounding tie may differ from the module route's.
ULTRA_TRAIN_FUSE = os.environ.get("QVIT_ULTRA_TRAIN_FUSE", "0")
if ULTRA_TRAIN_FUSE not in ("0", "1"):
    raise ValueError(f"QVIT_ULTRA_TRAIN_FUSE={ULTRA_TRAIN_FUSE!r}: expected 0 or 1")


def train_fuse_enabled() -> bool:
    if ULTRA_TRAIN_FUSE not in ("0", "1"):
        raise ValueError(f"ULTRA_TRAIN_FUSE = {ULTRA_TRAIN_FUSE!r}: expected 0 or 1")
    return ULTRA_TRAIN_FUSE == "1"


def _backward_gemm_ops() -> tuple:
    ops = _lib.backward_ops(ULTRA_BWD, "ULTRA_BWD")
    return tuple(o for o in ops if o not in ULTRA_BWD_DEFAULT_TORCH) if ULTRA_BWD == "hip" else ops


class _UniformSTE(torch.autograd.Function):
    """quant_ultra.py:11-27: the k-bit uniform quantizer with the straight-through backward."""

    @staticmethod
    def forward(ctx, x, k):
        if k == 32:
            return x.view_as(x)
        if k == 1:
            return torch.sign(x)
        n = float(2 ** k - 1)
        return torch.round(x * n) / n

    @staticmethod
    def backward(ctx, grad_output):
        return grad_output.clone(), None   # :24-25


def uniform_quantize(k):
    """quant_ultra.py:8-27. Returns the quantizer function, an autograd apply as the reference's."""

    def qfn(x: torch.Tensor) -> torch.Tensor:
        return _UniformSTE.apply(x, k)

    return qfn


class _WeightQuantSTE(torch.autograd.Function):
    """weight_quantize_fn.forward for 2 <= w_bit <= 8 (quant_ultra.py:50-55) as one node: the HIP quantizer's
    values forward, qvit_ultra_weight_quant_backward backward."""

    @staticmethod
    def forward(ctx, x, w_bit):
        ctx.save_for_backward(x)
        ctx.w_bit = w_bit
        return _weight_values(x, w_bit)

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        return _lib.ultra_weight_quant_backward(x, grad_output, ctx.w_bit).reshape(x.shape).to(x.dtype), None


class _ActQuantSTE(torch.autograd.Function):
    """activation_quantize_fn.forward for a_bit <= 7 (quant_ultra.py:71) as one node: the HIP quantizer forward,
    the clamp mask (qvit_ultra_act_quant_backward) backward."""

    @staticmethod
    def forward(ctx, x, levels):
        ctx.save_for_backward(x)
        return _lib.fake_quant_f32(x, _lib.QT_ULTRA_ACT, None, None, None, levels).reshape(x.shape)

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        return _lib.ultra_act_quant_backward(x, grad_output).reshape(x.shape).to(x.dtype), None


class _BnActPoolFunction(torch.autograd.Function):
    """BatchNorm2d on batch statistics -> activation_quantize_fn -> optional MaxPool2d(2, 2) as one node
    (ultra_bn_fuse.hip). Saved for the backward: x, mean, invstd, one flag byte per output
    element (the clamp's pass bit and, pooled, the window's winner) and gamma; no batch-norm output, no quantizer
    input, no pool indices. The backward recomputes xhat from x."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mean, invstd, levels, pool):
        out, flags = _lib.bn_act_pool_forward(x, mean, invstd, gamma, beta, levels, pool)
        ctx.save_for_backward(x, mean, invstd, flags, gamma)
        ctx.pool = pool
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, mean, invstd, flags, gamma = ctx.saved_tensors
        need_x, need_g, need_b = ctx.needs_input_grad[:3]
        dx, dgamma, dbeta, _ = _lib.bn_act_pool_backward(x, grad_out, flags, mean, invstd, gamma, ctx.pool,
                                                         need_g, need_b)
        return (dx.to(x.dtype) if need_x else None, dgamma if need_g else None, dbeta if need_b else None, None, None,
                None, None)


def _pool_fits(pool) -> bool:
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    return (isinstance(pool, nn.MaxPool2d) and pair(pool.kernel_size) == (2, 2) and pair(pool.stride) == (2, 2)
            and pair(pool.padding) == (0, 0) and pair(pool.dilation) == (1, 1) and not pool.ceil_mode
            and not pool.return_indices)


def bn_act_pool(x: torch.Tensor, bn, act, pool=None):
    """pool(act(bn(x))) for an nn.BatchNorm2d on batch statistics (training mode, or no running statistics), an
    activation_quantize_fn with 1 <= a_bit <= 7 and `pool` None or MaxPool2d(2, 2): qvit_bn_stats (which also makes
    the module's running-statistics update; num_batches_tracked is bumped here), then one autograd node,
    _BnActPoolFunction. x: a 4-D fp32 ROCm tensor. Returns None when the modules do not fit (the caller then runs
    them one by one)."""
    if not (type(bn) is nn.BatchNorm2d and (bn.training or (bn.running_mean is None and bn.running_var is None))
            and isinstance(act, activation_quantize_fn) and 1 <= act.a_bit <= 7
            and (pool is None or _pool_fits(pool))
            and isinstance(x, torch.Tensor) and x.dim() == 4 and x.is_cuda and x.dtype == torch.float32
            and x.shape[1] == bn.num_features and x.numel() > 0):
        return None
    B, C, H, W = x.shape
    if B * H * W < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")
    if pool is not None and (H < 2 or W < 2):
        return None
    factor, rmean, rvar = 0.0, None, None
    if bn.training and bn.track_running_stats:   # nn.BatchNorm2d.forward
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
            factor = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
        else:
            factor = 0.0 if bn.momentum is None else bn.momentum
        rmean, rvar = bn.running_mean, bn.running_var
    xc = x if x.is_contiguous() else x.contiguous()
    mean, _, invstd = _lib.bn_stats(xc, bn.eps, factor, rmean, rvar)
    return _BnActPoolFunction.apply(xc, bn.weight, bn.bias, mean, invstd, 2 ** act.a_bit - 1, pool is not None)


def weight_codes(weight: torch.Tensor, w_bit: int, kpad: int = None, cout_pad: int = None) -> torch.Tensor:
    """Integer weight codes of weight_quantize_fn (HIP), [cout_pad][kpad] in K order (ky, kx, c)."""
    _check_gpu(weight, "weight")
    w4 = weight if weight.dim() == 4 else weight.reshape(weight.shape[0], -1, 1, 1)
    cout, cin, ks, _ = w4.shape
    kpad = kpad or _lib.round_up(ks * ks * cin, 16)
    cout_pad = cout_pad or cout
    return _lib.ultra_weight_codes(w4, w_bit, kpad, cout_pad)


def _weight_values(x: torch.Tensor, w_bit: int) -> torch.Tensor:
    """The fake-quant weight round(.) / n (:20) of the HIP quantizer, divided on the device as IEEE fp32."""
    w4 = x if x.dim() == 4 else x.reshape(x.shape[0], -1, 1, 1)
    cout, cin, ks, _ = w4.shape
    _, vals = _lib.ultra_weight_codes(w4, w_bit, _lib.round_up(ks * ks * cin, 16), cout, values=True)
    return vals.reshape(x.shape)


class weight_quantize_fn(nn.Module):
    """quant_ultra.py:30-56."""

    def __init__(self, w_bit):
        super().__init__()
        assert w_bit <= 8 or w_bit == 32
        self.w_bit = w_bit
        self.uniform_q = uniform_quantize(k=w_bit - 1)

    def forward(self, x):
        if self.w_bit == 32:
            return x
        if self.w_bit == 1:   # reference behaviour kept as is (its k = 0 quantizer divides by zero)
            E = torch.mean(torch.abs(x)).detach()
            return (self.uniform_q(x / E) + 1) / 2 * E
        _check_gpu(x, "weight")
        if torch.is_grad_enabled() and x.requires_grad:
            return _WeightQuantSTE.apply(x, self.w_bit)
        return _weight_values(x, self.w_bit)


class activation_quantize_fn(nn.Module):
    """quant_ultra.py:59-73."""

    def __init__(self, a_bit):
        super().__init__()
        assert a_bit <= 8 or a_bit == 32
        self.a_bit = a_bit
        self.uniform_q = uniform_quantize(k=a_bit)

    def forward(self, x):
        if self.a_bit == 32:
            return x
        _check_gpu(x, "activation")
        if self.a_bit > 7:   # levels beyond the int8 code range: the reference arithmetic on the device
            return self.uniform_q(torch.clamp(x, 0, 1))
        if torch.is_grad_enabled() and x.requires_grad:
            return _ActQuantSTE.apply(x, 2 ** self.a_bit - 1)
        return _lib.fake_quant_f32(x, _lib.QT_ULTRA_ACT, None, None, None, 2 ** self.a_bit - 1).reshape(x.shape)


class _PackedCodes:
    """Packed weight codes of weight_quantize_fn for qvit_gemm_wonly / qvit_conv_wonly: the HIP quantizer's codes
    k (values k / n, n = 2^(w_bit-1) - 1) re-ordered to the weight's flattening (c, kh, kw), packed int4 (n <= 7)
    or int8, with d_w = 1/n. Rebuilt when the weight or bias changes (in place or replaced)."""

    def __init__(self):
        self.key = None

    def get(self, weight: torch.Tensor, bias, w_bit: int):
        key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.device,
               None if bias is None else (bias.data_ptr(), bias._version))
        if key == self.key:
            return self
        w4 = weight.detach() if weight.dim() == 4 else weight.detach().reshape(weight.shape[0], -1, 1, 1)
        cout, cin, kh, kw = w4.shape
        k = cin * kh * kw
        self.n, self.npad, self.kpad = cout, _lib.round_up(cout, _lib.TILE_N), _lib.round_up(k, _lib.TILE_K)
        codes = _lib.ultra_weight_codes(w4, w_bit, _lib.round_up(k, 16), cout)       # (ky, kx, c) order
        codes = codes[:, :k].view(cout, kh, kw, cin).permute(0, 3, 1, 2).reshape(cout, k).float().contiguous()
        n_lvl = 2 ** (w_bit - 1) - 1
        dev = weight.device
        self.wfmt = _lib.W4 if n_lvl <= 7 else _lib.W8
        self.packed = _lib.pack_codes(codes, self.wfmt, self.npad, self.kpad)
        self.d_wt = torch.full((1,), 1.0 / n_lvl, dtype=torch.float32, device=dev)
        self.bias_pad = _lib.pad_bias(bias, cout, self.npad, dev)
        self._shape4, self._w_bit, self._packed_t = (cout, cin, kh, kw), w_bit, None
        # views of the tensors the key names by address: their storage stays allocated while the key is kept, so a
        # replaced parameter cannot take the address (and the key) of the one these codes were made from
        self._held = (weight.detach(), None if bias is None else bias.detach())
        self.key = key
        return self

    def packed_t(self, weight: torch.Tensor):
        """(image, rows, npad, kpad) of the codes for the input gradient: transposed (rows = input channels,
        reduction = (output channel, ky, kx)) and flipped in (ky, kx), one qvit_pack_weight call in the forward's
        wfmt. Built from `weight` (the tensor get() was last called with) on the first backward that needs it and
        kept until the weight changes (get() drops it); nothing is held for it before that."""
        if self._packed_t is None:
            cout, cin, kh, kw = self._shape4
            k = cin * kh * kw
            codes = _lib.ultra_weight_codes(weight.detach().reshape(cout, cin, kh, kw), self._w_bit,
                                            _lib.round_up(k, 16), cout)       # (ky, kx, c) order, as get()
            ct = codes[:, :k].view(cout, kh, kw, cin).float().flip(1, 2).permute(3, 0, 1, 2).reshape(cin, cout * kh * kw)
            npad_t, kpad_t = _lib.round_up(cin, _lib.TILE_N), _lib.round_up(cout * kh * kw, _lib.TILE_K)
            img = _lib.pack_codes(ct.contiguous(), self.wfmt, npad_t, kpad_t)
            self._packed_t = (img, cin, npad_t, kpad_t)
        return self._packed_t


def _codes_path(w_bit: int) -> bool:
    return 2 <= w_bit <= 8


def _needs_grad(module: nn.Module, input: torch.Tensor) -> bool:
    """Autograd wants this call's history: the packed-codes kernels record none, so such calls go
    through one autograd node around the same kernel (_ConvQFunction / _LinearQFunction)."""
    return torch.is_grad_enabled() and (input.requires_grad or any(p.requires_grad for p in module.parameters()))


def _conv_codes_forward(module, input: torch.Tensor) -> torch.Tensor:
    c = module._codes.get(module.weight, module.bias, module.w_bit)
    return _lib.conv_wonly(input.detach(), module.kernel_size, module.stride, module.padding, module.dilation,
                           c.packed, c.wfmt, c.n, c.npad, c.kpad, c.d_wt, c.bias_pad)


class _ConvQFunction(torch.autograd.Function):
    """Conv2d_Q.forward on the codes path (quant_ultra.py:85-89) as one node: forward the qvit_conv_wonly call the
    module makes under no_grad; backward grad_bias = sum G, the input gradient on qvit_conv_wonly with the
    transposed and flipped codes (stride 1 and p <= d (k - 1); else torch.nn.grad.conv2d_input), the quantized
    weight's gradient on qvit_conv_wgrad (input declared as k / in_levels; else torch.nn.grad.conv2d_weight), and
    qvit_ultra_weight_quant_backward on it. Each only when its gradient is needed."""

    @staticmethod
    def forward(ctx, input, weight, bias, module, in_levels):
        ctx.module, ctx.in_levels = module, in_levels
        ctx.save_for_backward(input, weight)
        return _conv_codes_forward(module, input)

    @staticmethod
    def backward(ctx, G):
        input, weight = ctx.saved_tensors
        mod = ctx.module
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        ops = _backward_gemm_ops()
        G = G.detach().float().contiguous()
        ks, st, pd, dl = mod.kernel_size, mod.stride, mod.padding, mod.dilation
        grad_x = grad_w = grad_b = None
        if need_b:
            grad_b = G.sum((0, 2, 3)).to(mod.bias.dtype)
        if need_x:
            pad_t = tuple(d * (k - 1) - p for d, k, p in zip(dl, ks, pd))
            small = ULTRA_BWD != "hip" or input.shape[2] * input.shape[3] <= DGRAD_HIP_MAX_PIXELS
            if "dgrad" in ops and small and st == (1, 1) and min(pad_t) >= 0:
                c = mod._codes.get(weight, mod.bias, mod.w_bit)
                img, rows, npad_t, kpad_t = c.packed_t(weight)
                grad_x = _lib.conv_wonly(G, ks, st, pad_t, dl, img, c.wfmt, rows, npad_t, kpad_t, c.d_wt, None)
            else:
                with torch.no_grad():
                    grad_x = torch.nn.grad.conv2d_input(input.shape, _weight_values(weight, mod.w_bit), G, st, pd,
                                                        dl, 1)
            grad_x = grad_x.to(input.dtype)
        if need_w:
            xd = input.detach()
            if "wgrad" in ops and ctx.in_levels:
                grad_wq = _lib.conv_wgrad(G, xd, ks, st, pd, dl, ctx.in_levels)
            else:
                with torch.no_grad():
                    grad_wq = torch.nn.grad.conv2d_weight(xd.float(), weight.shape, G, st, pd, dl, 1)
            grad_w = _lib.ultra_weight_quant_backward(weight, grad_wq, mod.w_bit).reshape(weight.shape).to(
                weight.dtype)
        return grad_x, grad_w, grad_b, None, None


def _linear_codes_forward(module, input: torch.Tensor) -> torch.Tensor:
    c = module._codes.get(module.weight, module.bias, module.w_bit)
    y = _lib.gemm_wonly_rows(input.detach().reshape(-1, module.in_features), module.in_features, c.kpad, c.packed,
                             c.wfmt, c.n, c.npad, c.d_wt, c.bias_pad)
    return y.reshape(*input.shape[:-1], c.n)


class _LinearQFunction(torch.autograd.Function):
    """Linear_Q.forward on the codes path (quant_ultra.py:219-222) as one node: forward the qvit_gemm_wonly call;
    backward the input gradient on qvit_gemm_wonly with the transposed codes (as QuantizeLinear's), the quantized
    weight's gradient on torch.mm (the input is fp32) and qvit_ultra_weight_quant_backward on it."""

    @staticmethod
    def forward(ctx, input, weight, bias, module):
        ctx.module = module
        ctx.save_for_backward(input, weight)
        return _linear_codes_forward(module, input)

    @staticmethod
    def backward(ctx, G):
        input, weight = ctx.saved_tensors
        mod = ctx.module
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        G2 = G.detach().float().reshape(-1, mod.out_features).contiguous()
        M = G2.shape[0]
        grad_x = grad_w = grad_b = None
        if need_b:
            grad_b = G2.sum(0).to(mod.bias.dtype)
        if need_x:
            if "dgrad" in _backward_gemm_ops() and M:
                c = mod._codes.get(weight, mod.bias, mod.w_bit)
                img, rows, npad_t, kpad_t = c.packed_t(weight)
                gx2 = _lib.gemm_wonly_rows(G2, mod.out_features, kpad_t, img, c.wfmt, rows, npad_t, c.d_wt, None)
            else:
                gx2 = torch.mm(G2, _weight_values(weight, mod.w_bit))
            grad_x = gx2.reshape(input.shape).to(input.dtype)
        if need_w:
            grad_wq = torch.mm(G2.t(), input.detach().reshape(-1, mod.in_features).float())
            grad_w = _lib.ultra_weight_quant_backward(weight, grad_wq, mod.w_bit).reshape(weight.shape).to(
                weight.dtype)
        return grad_x, grad_w, grad_b, None


def conv2d_Q_fn(w_bit):
    """quant_ultra.py:76-91."""

    class Conv2d_Q(nn.Conv2d):
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                     bias=True):
            super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias)
            self.w_bit = w_bit
            self.quantize_fn = weight_quantize_fn(w_bit=w_bit)
            self._codes = _PackedCodes()
            self._bn_fold = None   # (key, alpha, shift) of the BatchNorm2d forward_bn_act last fused

        def prepare(self):
            """Packs the weight codes now (cached per weight version; see QuantizeMixin.prepare)."""
            if _codes_path(self.w_bit) and self.weight.is_cuda:
                self._codes.get(self.weight, self.bias, self.w_bit)
            return self

        def invalidate(self):
            """Drops the packed codes (and the fused BatchNorm fold): needed only after editing the weight, bias or BN
            statistics through `.data` (which bypasses the version counter the caches key on; QuantizeMixin.invalidate
            alike)."""
            self._codes.key = None
            self._bn_fold = None
            return self

        def forward(self, input, order=None, _in_levels=None):
            """`_in_levels` (private; UltraNetQua.forward_modules passes it): the caller's statement that `input`
            holds k / _in_levels with integer 0 <= k <= _in_levels, the output of an activation_quantize_fn
            (max-pooled or not), which puts the weight gradient on qvit_conv_wgrad."""
            if _codes_path(self.w_bit):
                _check_gpu(input, "input")
            if _codes_path(self.w_bit) and self.groups == 1 and self.padding_mode == "zeros" and \
                    not isinstance(self.padding, str) and input.dim() == 4:
                if _needs_grad(self, input):
                    return _ConvQFunction.apply(input, self.weight, self.bias, self, _in_levels)
                return _conv_codes_forward(self, input)
            weight_q = self.quantize_fn(self.weight)
            return F.conv2d(input, weight_q, self.bias, self.stride, self.padding, self.dilation, self.groups)

        def forward_bn_act(self, input, bn, act):
            """act(bn(self(input))) in one launch when `bn` is a BatchNorm2d in eval mode on running statistics and
            `act` an activation_quantize_fn with 1 <= a_bit <= 7 (UltraNet's conv -> BN -> quantizer blocks,
            mymodel.py:71-124): qvit_conv_wonly_bn_act, BN as y alpha + shift (alpha = gamma / sqrt(var + eps),
            shift = beta - mean alpha: the fused network's fold, ultra_bn_fold) and the quantizer's values
            round(clamp(., 0, 1) n) / n. Returns None when the three modules do not fit that launch (the caller then
            runs them one by one)."""
            if not (_codes_path(self.w_bit) and self.groups == 1 and self.padding_mode == "zeros"
                    and not isinstance(self.padding, str) and input.dim() == 4 and input.is_cuda
                    and isinstance(bn, nn.BatchNorm2d) and not bn.training and bn.track_running_stats
                    and bn.running_mean is not None and bn.running_var is not None
                    and bn.num_features == self.out_channels
                    and isinstance(act, activation_quantize_fn) and 1 <= act.a_bit <= 7
                    and not _needs_grad(self, input) and not _needs_grad(bn, input)):
                return None
            c = self._codes.get(self.weight, self.bias, self.w_bit)
            # num_batches_tracked stands for the running statistics: a library batch norm updates those through raw
            # pointers (no version bump), the module's own counter increment is always seen
            tensors = [t for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked)
                       if t is not None]
            key = tuple((t.data_ptr(), t._version) for t in tensors) + (bn.eps, input.device)
            if self._bn_fold is None or self._bn_fold[0] != key:
                # (key, alpha, shift, views that keep the addresses in the key from being reused)
                self._bn_fold = (key, *_lib.ultra_bn_fold(bn, input.device), tuple(t.detach() for t in tensors))
            return _lib.conv_wonly_bn_act(input.detach(), self.kernel_size, self.stride, self.padding, self.dilation,
                                          c.packed, c.wfmt, c.n, c.npad, c.kpad, c.d_wt, c.bias_pad, self._bn_fold[1],
                                          self._bn_fold[2], 2 ** act.a_bit - 1)

    return Conv2d_Q


def batchNorm2d_Q_fn(w_bit):
    """quant_ultra.py:94-132 (BN with quantized folded scale/shift)."""

    class BatchNorm2d_Q(nn.BatchNorm2d):
        def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
            super().__init__(num_features, eps, momentum, affine, track_running_stats)
            self.w_bit = w_bit
            self.quantize_fn = uniform_quantize(k=w_bit)

        def forward(self, input):
            gamma, var, mean, eps, bias = self.weight, self.running_var, self.running_mean, self.eps, self.bias
            w = gamma / (torch.sqrt(var) + eps)
            b = bias - (mean / (torch.sqrt(var) + eps)) * gamma
            w = torch.clamp(w, -1, 1) / 2 + 0.5
            w_q = 2 * self.quantize_fn(w) - 1
            b = torch.clamp(b, -1, 1) / 2 + 0.5
            b_q = 2 * self.quantize_fn(b) - 1
            return F.batch_norm(input, running_mean=mean * 0, running_var=torch.sign(torch.abs(var) + 1),
                                weight=w_q, bias=b_q, eps=eps * 0)

    return BatchNorm2d_Q


def batchNorm1d_Q_fn(w_bit):
    """quant_ultra.py:135-207 (eval form)."""

    class BatchNorm1d_Q(nn.BatchNorm1d):
        def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
            super().__init__(num_features, eps, momentum, affine, track_running_stats)
            self.w_bit = w_bit
            self.quantize_fn = uniform_quantize(k=w_bit)

        def forward(self, input):
            self._check_input_dim(input)
            gamma, var, mean, eps, bias = self.weight, self.running_var, self.running_mean, self.eps, self.bias
            w = gamma / (torch.sqrt(var) + eps)
            b = bias - (mean / (torch.sqrt(var) + eps)) * gamma
            return F.batch_norm(input, mean * 0, torch.sign(var + 1), w, b,
                                self.training or not self.track_running_stats, self.momentum or 0.0, eps * 0)

    return BatchNorm1d_Q


def linear_Q_fn(w_bit):
    """quant_ultra.py:210-222."""

    class Linear_Q(nn.Linear):
        def __init__(self, in_features, out_features, bias=True):
            super().__init__(in_features, out_features, bias)
            self.w_bit = w_bit
            self.quantize_fn = weight_quantize_fn(w_bit=w_bit)
            self._codes = _PackedCodes()

        def prepare(self):
            """Packs the weight codes now (cached per weight version; see QuantizeMixin.prepare)."""
            if _codes_path(self.w_bit) and self.weight.is_cuda:
                self._codes.get(self.weight, self.bias, self.w_bit)
            return self

        def invalidate(self):
            """Drops the packed codes (see Conv2d_Q.invalidate)."""
            self._codes.key = None
            return self

        def forward(self, input):
            if not _codes_path(self.w_bit):
                return F.linear(input, self.quantize_fn(self.weight), self.bias)
            _check_gpu(input, "input")
            if _needs_grad(self, input):
                return _LinearQFunction.apply(input, self.weight, self.bias, self)
            return _linear_codes_forward(self, input)

    return Linear_Q
