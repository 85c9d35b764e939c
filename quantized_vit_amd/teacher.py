"""The full-precision distillation teacher on HIP.

The reference's driver distils from a ViT it never quantizes: train.py:290-316 builds create_model(...), puts it in
eval() and freezes its parameters; utils.py:268-274 runs it once per step under no_grad. Its weights never change, so
their bf16 split (the weight half of qvit_gemm_f32_nt's work) is done once, into a QVIT_WB3 image, and every forward
runs qvit_gemm_f32w on it:

    teacher = prepare_teacher(create_model(...).to(device))          # fp32-GEMM accuracy, six bf16 products
    teacher = prepare_teacher(..., precision="bf16x2")               # three products, about 2^-13 relative

prepare_teacher swaps every plain nn.Linear for a FrozenLinear (same parameters, same state_dict keys); a vit_model
Block whose four linears are FrozenLinear then runs norm1 -> qkv -> attention core -> proj (+= residual) -> norm2 ->
fc1 (GELU fused) -> fc2 (+= residual) on one residual buffer. QuantizeLinear layers are left alone.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .quant_layers import _autograd_live

PRECISIONS = {"fp32": 6, "bf16x2": 3}   # precision -> qvit_gemm_f32w's `terms`


class FrozenLinear(nn.Linear):
    """nn.Linear whose weight is not being trained. On a ROCm fp32 input of at least MIN_ROWS rows, with no autograd
    history to record, forward() is qvit_gemm_f32w on a cached QVIT_WB3 image of the weight; anywhere else (autograd
    live, CPU, other dtypes, few rows: the kernel has no split of K) it is F.linear. The image is keyed on (data_ptr,
    _version, device, shape) of weight and bias, so an in-place update, a load_state_dict or a .to() rebuilds it on the
    next call; invalidate() drops it (after a write that bypasses the version counter)."""

    MIN_ROWS = 64

    def __init__(self, in_features: int, out_features: int, bias: bool = True, device=None, dtype=None,
                 precision: str = "fp32"):
        super().__init__(in_features, out_features, bias, device=device, dtype=dtype)
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
        self.precision = precision
        self._image: Optional[torch.Tensor] = None
        self._image_key: Optional[tuple] = None

    @classmethod
    def from_linear(cls, lin: nn.Linear, precision: str = "fp32") -> "FrozenLinear":
        """A FrozenLinear on `lin`'s own parameters (shared, not copied)."""
        m = cls(lin.in_features, lin.out_features, lin.bias is not None, device="meta", precision=precision)
        m.weight, m.bias = lin.weight, lin.bias
        m.train(lin.training)
        return m

    def invalidate(self) -> None:
        self._image = self._image_key = None

    def _key(self) -> tuple:
        return tuple(None if p is None else (p.data_ptr(), p._version, p.device, tuple(p.shape))
                     for p in (self.weight, self.bias)) + (self.precision,)

    def image(self) -> torch.Tensor:
        key = self._key()
        if self._image is None or self._image_key != key:
            self._image = _lib.pack_weight_b3(self.weight, 3 if PRECISIONS[self.precision] == 6 else 2)
            self._image_key = key
        return self._image

    def hip_ok(self, x: torch.Tensor) -> bool:
        """Whether a call on `x` may run the kernel at all (device, dtypes, nothing for autograd to record)."""
        w = self.weight
        return (x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32 and w.device == x.device
                and (self.bias is None or self.bias.dtype == torch.float32) and not _autograd_live(self, x))

    def gemm(self, x2: torch.Tensor, epilogue: int = _lib.EPI_F32, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """epi(x2 @ W^T + b) for rows x2 [M, in_features] (hip_ok is the caller's to check)."""
        return _lib.gemm_f32w(x2, self.image(), self.out_features, PRECISIONS[self.precision], self.bias, epilogue,
                              out)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.hip_ok(x) or x.numel() < self.MIN_ROWS * self.in_features:
            return F.linear(x, self.weight, self.bias)
        y = self.gemm(x.reshape(-1, self.in_features))
        return y.reshape(*x.shape[:-1], self.out_features)

    def extra_repr(self) -> str:
        return f"{super().extra_repr()}, precision={self.precision}"


def prepare_teacher(model: nn.Module, precision: str = "fp32") -> nn.Module:
    """Freezes `model` as a distillation teacher: every module whose type is exactly nn.Linear becomes a
    FrozenLinear on the same parameters (subclasses such as QuantizeLinear stay), then eval() and
    requires_grad_(False). Returns `model`."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(PRECISIONS)}, got {precision!r}")
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if type(child) is nn.Linear:
                setattr(parent, name, FrozenLinear.from_linear(child, precision))
    if type(model) is nn.Linear:
        model = FrozenLinear.from_linear(model, precision)
    model.eval()
    model.requires_grad_(False)
    return model
