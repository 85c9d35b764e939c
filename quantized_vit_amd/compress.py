"""Model surgery after pruning: a ViT's layers rebuilt without the MLP hidden units and attention heads that
QuantAwareOptimizer's pruning stages (qat_prune.py) left as zeros. Reads the weights alone; needs no optimizer."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .qat_optim import _SCALARS, _SIDES
from .qat_prune import unit_rows_of, units_view
from .quant_layers import QuantizeLinear


def _resized_linear(src: nn.Linear, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> nn.Linear:
    """A layer of src's kind around the given weight and bias, src's quantizer scalars and clip values carried over."""
    out_f, in_f = weight.shape
    if isinstance(src, QuantizeLinear):
        new = QuantizeLinear(in_f, out_f, bias=bias is not None, quant_type=src.quant_type, quant_mode=src.quant_mode)
        new.weight_clip_val, new.act_clip_val = src.weight_clip_val, src.act_clip_val
    else:
        new = nn.Linear(in_f, out_f, bias=bias is not None)
    new = new.to(device=weight.device, dtype=weight.dtype)
    new.weight.data.copy_(weight)
    new.weight.requires_grad_(src.weight.requires_grad)
    if bias is not None:
        new.bias.data.copy_(bias)
        new.bias.requires_grad_(src.bias.requires_grad)
    for side in _SIDES:
        for sc in _SCALARS:
            a, b = getattr(src, f"{sc}_{side}", None), getattr(new, f"{sc}_{side}", None)
            if a is not None and b is not None:
                b.data.copy_(a.data)
                b.requires_grad_(a.requires_grad)
    new.train(src.training)
    if callable(getattr(new, "invalidate", None)):
        new.invalidate()
    return new


@torch.no_grad()
def compress_pruned_mlp(model: nn.Module) -> nn.Module:
    """Removes every all-zero fc1 row (weight row and bias entry both zero) of every blocks[i].mlp together with its
    fc2 column, in place, and returns the model: this project's counterpart of the reference's construct_subnet for
    this one structure. The quantizer scalars are carried over and the plans start afresh. An optimizer built over
    the model before the call no longer matches it."""
    for blk in model.blocks:
        fc1, fc2 = blk.mlp.fc1, blk.mlp.fc2
        dead = (fc1.weight == 0).all(dim=1)
        if fc1.bias is not None:
            dead &= fc1.bias == 0
        keep = (~dead).nonzero().flatten()
        if keep.numel() == fc1.out_features:
            continue
        if keep.numel() == 0:
            raise ValueError("compress_pruned_mlp: a block's MLP has no hidden unit left")
        blk.mlp.fc1 = _resized_linear(fc1, fc1.weight[keep], None if fc1.bias is None else fc1.bias[keep])
        blk.mlp.fc2 = _resized_linear(fc2, fc2.weight[:, keep], fc2.bias)
    return model


@torch.no_grad()
def compress_pruned_heads(model: nn.Module) -> nn.Module:
    """Removes every attention head whose q, k and v rows of attn.qkv.weight and entries of attn.qkv.bias are all
    zero, together with the matching columns of attn.proj.weight, in place, and returns the model; sets
    attn.num_heads and leaves head_dim and the softmax scale as they are. The quantizer scalars are carried over and
    the plans start afresh. A removed head's bias entries are zero, so the qkv layer's output bound, and with it the
    attention input scale, is the uncompressed layer's. Composes with compress_pruned_mlp in either order. An
    optimizer built over the model before the call no longer matches it."""
    for blk in model.blocks:
        a = blk.attn
        H, hd = int(a.num_heads), int(a.head_dim)
        if a.qkv.out_features != 3 * H * hd or a.proj.in_features != H * hd:
            raise ValueError(f"compress_pruned_heads: qkv has {a.qkv.out_features} outputs and proj {a.proj.in_features} "
                             f"inputs, not 3 x {H} x {hd} and {H} x {hd}")
        dead = (units_view(a.qkv.weight, H, 3, hd) == 0).all(dim=1)
        if a.qkv.bias is not None:
            dead &= (units_view(a.qkv.bias, H, 3, hd) == 0).all(dim=1)
        keep = (~dead).nonzero().flatten().tolist()
        if len(keep) == H:
            continue
        if not keep:
            raise ValueError("compress_pruned_heads: a block's attention has no head left")
        rows = torch.from_numpy(unit_rows_of(keep, H, 3, hd).reshape(len(keep), 3, hd).transpose(1, 0, 2).reshape(-1)
                                ).to(a.qkv.weight.device)   # section-major again: [3, kept heads, hd]
        cols = torch.from_numpy(unit_rows_of(keep, H, 1, hd)).to(a.qkv.weight.device)
        a.qkv = _resized_linear(a.qkv, a.qkv.weight[rows], None if a.qkv.bias is None else a.qkv.bias[rows])
        a.proj = _resized_linear(a.proj, a.proj.weight[:, cols], a.proj.bias)
        a.num_heads = len(keep)
    return model
