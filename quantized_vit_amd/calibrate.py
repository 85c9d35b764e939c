"""Synthetic-model setup: activation-range calibration and quantized ViT construction.

The reference initialises a layer's activation quantizer from the WEIGHT statistics
(quant_layers.py:436-438), which saturates almost every activation; trained GETA checkpoints carry
learned values instead. For synthetic benchmarks and parity tests we set them the way GETA's
projection does (optimizer/geta.py:788-804, d = exp(t log|q_m|) / (2^(b-1) - 1)) from q_m = max|x|
of each layer's input on a calibration batch of the un-quantized model.

For a pretrained fp32 model there is an error-minimising clip search on the device besides (search_activation_quant,
search_weight_quant, quantize_pretrained, further down): the same family of quantizers, with q_m chosen per tensor
by the quantization error instead of set to max|x|.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .quant_layers import (QuantizationMode, QuantizationType, QuantizeConv2d, QuantizeLinear, _qtype_code,
                           saturation_level)
from .quant_model import model_to_quantize_model
from . import vit_model


@torch.no_grad()
def collect_input_absmax(model: nn.Module, x: torch.Tensor) -> Dict[str, float]:
    """max|input| of every nn.Linear / nn.Conv2d (by module name) over one forward of `x`."""
    stats: Dict[str, float] = {}
    hooks = []
    for name, mod in model.named_modules():
        if isinstance(mod, (nn.Linear, nn.Conv2d)):
            def hook(m, inp, out, name=name):
                v = float(inp[0].detach().abs().max())
                stats[name] = max(stats.get(name, 0.0), v)
            hooks.append(mod.register_forward_hook(hook))
    try:
        model(x)
    finally:
        for h in hooks:
            h.remove()
    return stats


def d_quant_for_bits(bits: int, q_m: float, t: float = 1.0) -> float:
    """GETA._d_quant_helper, optimizer/geta.py:788-804."""
    return math.exp(t * math.log(abs(q_m))) / (2 ** (bits - 1) - 1)


@torch.no_grad()
def set_activation_quant(model: nn.Module, absmax: Dict[str, float], bits: int = 8, t: float = 1.0) -> None:
    for name, mod in model.named_modules():
        if isinstance(mod, (QuantizeLinear, QuantizeConv2d)) and \
                mod.quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION and name in absmax:
            qm = max(absmax[name], 1e-8)
            mod.q_m_act.fill_(qm)
            mod.d_quant_act.fill_(d_quant_for_bits(bits, qm, t))
            if hasattr(mod, "t_quant_act"):
                mod.t_quant_act.fill_(t)
            mod.invalidate()


@torch.no_grad()
def set_weight_quant_t(model: nn.Module, t: float, bits: int = 4) -> None:
    """Re-derives the weight quantizer for a given t (d = max|W|^t / (2^(b-1) - 1))."""
    for mod in model.modules():
        if isinstance(mod, (QuantizeLinear, QuantizeConv2d)) and hasattr(mod, "t_quant_wt"):
            qm = float(mod.q_m_wt)
            mod.t_quant_wt.fill_(t)
            mod.d_quant_wt.fill_(d_quant_for_bits(bits, qm, t))
            mod.invalidate()


@torch.no_grad()
def redraw_init_artifacts(model: nn.Module, limit: float = 1.0) -> int:
    """Re-draws the sampling artifacts of torch.nn.init.trunc_normal_ in a freshly initialised ViT.

    _init_vit_weights (vit_model.py:331-346) draws Linear weights from trunc_normal_(std=.01) and the class / position
    embeddings from trunc_normal_(std=.02), truncated at the absolute bounds [-2, 2] (200 / 100 sigma). torch samples it
    by inverse CDF: uniform_(-1, 1) then erfinv_; a uniform draw of exactly -1 (about 2^-24 per element) becomes -inf and
    is clamped to -2.0. So a ViT-L/16 holds a dozen weights of exactly +-2.0 (12 layers at seed 0, the head among
    them), values the intended distribution gives with probability ~0. Under the per-tensor max quantizer
    (initialize_quant_layer: d = max|W| / 7) such a layer's int4 codes are all 0 but one: the head then has one
    nonzero weight, the logits depend on a single activation code per image, and any logits comparison becomes a coin
    toss on that code's rounding. Every element with |w| >= `limit` (50-100 sigma) is re-drawn from the intended
    normal with the global generator (deterministic for a seed; a model without artifacts is left unchanged).
    Returns the number of elements re-drawn."""
    n = 0
    for name, p in model.named_parameters():
        std = 0.02 if name in ("pos_embed", "cls_token", "dist_token") else 0.01
        if not (name.endswith("weight") and p.dim() == 2) and std == 0.01:
            continue
        mask = p.abs() >= limit
        while bool(mask.any()):
            k = int(mask.sum())
            n += k
            p[mask] = torch.randn(k) * std
            mask = p.abs() >= limit
    return n


VIT_CONFIGS = {
    "vit_tiny_patch16_224": dict(img_size=224, patch_size=16, embed_dim=192, depth=12, num_heads=3),
    "vit_base_patch16_224": dict(img_size=224, patch_size=16, embed_dim=768, depth=12, num_heads=12),
    "vit_large_patch16_384": dict(img_size=384, patch_size=16, embed_dim=1024, depth=24, num_heads=16),
}


@torch.no_grad()
def build_quantized_vit(name: str = "vit_base_patch16_224", num_classes: int = 1000, seed: int = 0,
                        w_bits: int = 4, a_bits: int = 8,
                        quant_type: QuantizationType = QuantizationType.SYMMETRIC_NONLINEAR,
                        t_act: float = 1.0, t_wt: float = 1.0, calib_batch: int = 2, calib_seed: int = 1,
                        device: Optional[torch.device] = None, depth: Optional[int] = None) -> nn.Module:
    """Random-init ViT (reference init, vit_model.py:331-346), swapped to W{w_bits}A{a_bits} fake-quant
    layers (model_to_quantize_model with num_bits=w_bits, WEIGHT_AND_ACTIVATION) and calibrated.

    Calibration runs the fp32 model on `calib_batch` uniform[-1,1) images (seed calib_seed) on
    `device` (CPU if None) before the swap. Deterministic for a given seed and device."""
    cfg = dict(VIT_CONFIGS[name])
    if depth is not None:
        cfg["depth"] = depth
    g = torch.manual_seed(seed)
    model = vit_model.VisionTransformer(num_classes=num_classes, representation_size=None, **cfg)
    redraw_init_artifacts(model)
    dev = device or torch.device("cpu")
    model = model.to(dev).eval()
    gen = torch.Generator(device="cpu").manual_seed(calib_seed)
    img = (torch.rand(calib_batch, 3, cfg["img_size"], cfg["img_size"], generator=gen) * 2 - 1).to(dev)
    absmax = collect_input_absmax(model, img)
    model = model_to_quantize_model(model, num_bits=w_bits, quant_type=quant_type,
                                    quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    if t_wt != 1.0:
        set_weight_quant_t(model, t_wt, w_bits)
    set_activation_quant(model, absmax, bits=a_bits, t=t_act)
    del g
    return model.eval()


def synthetic_images(batch: int, img_size: int, seed: int = 0, device=None) -> torch.Tensor:
    """uniform[-1,1) NCHW images (predict.py:15-19 normalisation range), seeded on the CPU."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand(batch, 3, img_size, img_size, generator=gen) * 2 - 1
    return x.to(device) if device is not None else x


# ---- error-minimising clip search (qvit_quant_error) -----------------------------------------------------------
# For a pretrained fp32 model without a GETA run: per tensor, the quantization error of a grid of clip values q_m
# with d = q_m^t / (2^(b-1) - 1) (the family GETA's projection draws from), scored by one kernel that reads the
# tensor once per 16 candidates and accumulates across calibration batches; the minimum is kept. The last candidate
# is the absmax choice above, so by its own measure the search never does worse than set_activation_quant.
@dataclass
class QuantChoice:
    """The quantizer picked for one tensor. err / err_absmax: the summed squared error of the pick and of the absmax
    candidate over all calibration data; clipped: elements with |x| >= q_m; widened: d was stepped up after the
    search so that the saturation code fits the bit width (quantize_pretrained; fp32 rounding of d alone)."""
    q_m: float
    d: float
    t: float
    err: float
    err_absmax: float
    clipped: int
    numel: int
    widened: bool = False


def clip_candidates(absmax: float, bits: int, t: float = 1.0, num: int = 32,
                    min_frac: float = 0.2) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q_m [num], d [num]) fp32 on the CPU: q_m_c = absmax (min_frac + (1 - min_frac) c / (num - 1)), ascending, and
    d_c = d_quant_for_bits(bits, q_m_c, t). The last candidate is q_m = absmax itself."""
    if not 1 <= num <= _lib.QUANT_ERROR_MAX_CAND:
        raise ValueError(f"clip_candidates: num = {num}, expected 1 .. {_lib.QUANT_ERROR_MAX_CAND}")
    if not (0.0 < min_frac <= 1.0) or not (absmax > 0.0 and math.isfinite(absmax)):
        raise ValueError(f"clip_candidates: absmax = {absmax}, min_frac = {min_frac}")
    fracs = [1.0] if num == 1 else [min_frac + (1.0 - min_frac) * c / (num - 1) for c in range(num)]
    q_m = [absmax * f for f in fracs]
    d = [d_quant_for_bits(bits, q, t) for q in q_m]
    return torch.tensor(q_m, dtype=torch.float32), torch.tensor(d, dtype=torch.float32)


def _rows(x: torch.Tensor) -> torch.Tensor:
    """x as an fp32 matrix with unit column stride (a view where the layout allows one)."""
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    x2 = x.reshape(-1, x.shape[-1]) if x.dim() >= 2 else x.reshape(1, -1)
    return x2 if x2.shape[1] <= 1 or x2.stride(1) == 1 else x2.contiguous()


class _Search:
    """One tensor's candidates and its accumulators on the device."""

    def __init__(self, name: str, absmax: float, bits: int, t: float, qtype: int, num: int, min_frac: float, dev):
        self.name, self.t, self.qtype, self.numel = name, float(t), qtype, 0
        linear = qtype == _lib.QT_LINEAR
        self.q_m, self.d = clip_candidates(max(absmax, 1e-8), bits, 1.0 if linear else t, num, min_frac)
        self.q_m_dev, self.d_dev = self.q_m.to(dev), self.d.to(dev)
        self.t_dev = None if linear else torch.tensor([t], dtype=torch.float32, device=dev)
        self.err = torch.zeros(num, dtype=torch.float64, device=dev)
        self.nclip = torch.zeros(num, dtype=torch.int64, device=dev)

    def add(self, x: torch.Tensor) -> None:
        x2 = _rows(x)
        self.numel += x2.numel()
        _lib.quant_error(x2, self.qtype, self.d_dev, self.q_m_dev, self.t_dev, self.err, self.nclip, accumulate=True)

    def choice(self, err: torch.Tensor, nclip: torch.Tensor, what: str) -> QuantChoice:
        if not bool(torch.isfinite(err).all()):
            raise ValueError(f"{what} of layer {self.name!r}: the quantization error is not finite "
                             "(a NaN or infinite value in the tensor)")
        best = int((err == err.min()).nonzero().max())    # ties go to the larger q_m
        return QuantChoice(q_m=float(self.q_m[best]), d=float(self.d[best]), t=self.t, err=float(err[best]),
                           err_absmax=float(err[-1]), clipped=int(nclip[best]), numel=self.numel)


def _choices(searches: List[_Search], what: str) -> Dict[str, QuantChoice]:
    """Reads every accumulator with one host sync and takes the minima."""
    if not searches:
        return {}
    err = torch.stack([s.err for s in searches]).cpu()
    nclip = torch.stack([s.nclip for s in searches]).cpu()
    return {s.name: s.choice(err[i], nclip[i], what) for i, s in enumerate(searches)}


def _finite_absmax(names: List[str], absmax: List[torch.Tensor], what: str) -> List[float]:
    vals = torch.stack(absmax).cpu().tolist() if absmax else []
    for name, v in zip(names, vals):
        if not math.isfinite(v):
            raise ValueError(f"{what} of layer {name!r}: max|x| is {v} (a NaN or infinite value in the tensor)")
    return vals


def _device_of(model: nn.Module) -> torch.device:
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.QvitError(f"the clip search runs on a ROCm device (the model is on {dev}); the HIP path has no "
                             "CPU fallback")
    return dev


@torch.no_grad()
def search_activation_quant(model: nn.Module, batches: Iterable[torch.Tensor], bits: int = 8, t: float = 1.0,
                            quant_type: QuantizationType = QuantizationType.SYMMETRIC_NONLINEAR, num: int = 32,
                            min_frac: float = 0.2) -> Dict[str, QuantChoice]:
    """Error-minimising activation quantizer of every nn.Linear / nn.Conv2d input (by module name) of the
    un-quantized `model`, over `batches` (re-iterable: it is walked twice, first for max|x| per layer, then for the
    error of each candidate of clip_candidates, accumulated on the device across batches). Two host syncs in all:
    the maxima after the first pass, the errors after the second."""
    dev = _device_of(model)
    layers = [(name, mod) for name, mod in model.named_modules() if isinstance(mod, (nn.Linear, nn.Conv2d))]
    qtype = _qtype_code(quant_type)

    def run(hook_for) -> None:
        hooks = [mod.register_forward_hook(hook_for(name)) for name, mod in layers]
        try:
            for x in batches:
                model(x.to(dev))
        finally:
            for h in hooks:
                h.remove()

    absmax: Dict[str, torch.Tensor] = {}

    def absmax_hook(name):
        def hook(m, inp, out):
            v = inp[0].detach().abs().max().float()
            absmax[name] = torch.maximum(absmax[name], v) if name in absmax else v
        return hook

    def maxima() -> List[float]:
        return _finite_absmax(names, [absmax[n] for n in names], "activation")
    try:
        run(absmax_hook)
    except ValueError:     # a model that trips over a NaN of its own: name the first layer that was fed one
        names = [name for name, _ in layers if name in absmax]
        maxima()
        raise
    names = [name for name, _ in layers if name in absmax]
    vals = maxima()
    searches = {n: _Search(n, v, bits, t, qtype, num, min_frac, dev) for n, v in zip(names, vals)}

    def error_hook(name):
        def hook(m, inp, out):
            if name in searches:
                searches[name].add(inp[0])
        return hook
    run(error_hook)
    return _choices(list(searches.values()), "activation")


@torch.no_grad()
def search_weight_quant(model: nn.Module, bits: int = 4, num: int = 32, min_frac: float = 0.2) -> Dict[str, QuantChoice]:
    """The same search on the weight of every QuantizeLinear / QuantizeConv2d, per tensor as the reference quantizes
    (quant_layers.py:332-354). The nonlinear type reads the layer's own t_quant_wt."""
    dev = _device_of(model)
    layers = [(name, mod) for name, mod in model.named_modules() if isinstance(mod, (QuantizeLinear, QuantizeConv2d))]
    if not layers:
        return {}
    stats = torch.stack([torch.stack([mod.weight.detach().abs().max().float(),
                                      (mod.t_quant_wt.detach().reshape(-1)[0].float() if hasattr(mod, "t_quant_wt")
                                       else torch.ones((), device=mod.weight.device))]) for _, mod in layers]).cpu()
    vals = _finite_absmax([n for n, _ in layers], list(stats[:, 0]), "weight")
    searches = []
    for (name, mod), v, t in zip(layers, vals, stats[:, 1].tolist()):
        s = _Search(name, v, bits, t, _qtype_code(mod.quant_type), num, min_frac, dev)
        s.add(mod.weight.detach().reshape(mod.weight.shape[0], -1))
        searches.append(s)
    return _choices(searches, "weight")


@torch.no_grad()
def apply_quant_choices(model: nn.Module, act: Optional[Dict[str, QuantChoice]] = None,
                        wt: Optional[Dict[str, QuantChoice]] = None) -> None:
    """Writes the choices into q_m_*, d_quant_* and (where the layer has one) t_quant_* of the quantized layers they
    name; activation choices only into WEIGHT_AND_ACTIVATION layers."""
    for name, mod in model.named_modules():
        if not isinstance(mod, (QuantizeLinear, QuantizeConv2d)):
            continue
        touched = False
        for which, choices in (("act", act), ("wt", wt)):
            if not choices or name not in choices or not hasattr(mod, f"q_m_{which}"):
                continue
            c = choices[name]
            getattr(mod, f"q_m_{which}").fill_(c.q_m)
            getattr(mod, f"d_quant_{which}").fill_(c.d)
            if hasattr(mod, f"t_quant_{which}"):
                getattr(mod, f"t_quant_{which}").fill_(c.t)
            touched = True
        if touched:
            mod.invalidate()


def _fit_level(c: QuantChoice, qtype: int, bits: int) -> QuantChoice:
    """c, with d stepped up to the smallest fp32 value whose saturation code rne(p_sat / d) is at most
    2^(bits-1) - 1, when the chosen pair exceeds it. d = q_m^t / levels puts the quotient at the level exactly; only
    the rounding of d to fp32 (and the reference's + 1e-6 on a very small q_m) can push the code one past it."""
    levels = 2 ** (bits - 1) - 1
    t = 1.0 if qtype == _lib.QT_LINEAR else c.t
    if saturation_level(qtype, c.d, c.q_m, t) <= levels:
        return c
    f = np.float32
    p_sat = np.abs(f(c.q_m)) if qtype == _lib.QT_LINEAR else \
        np.exp(f(t) * np.log(np.abs(f(c.q_m)) + f(1e-6)), dtype=np.float32)
    d = max(f(c.d), f(p_sat / f(levels + 0.5)))
    while saturation_level(qtype, float(d), c.q_m, t) > levels:
        d = np.nextafter(d, f(np.inf), dtype=np.float32)
    return QuantChoice(**{**c.__dict__, "d": float(d), "widened": True})


@torch.no_grad()
def quantize_pretrained(model: nn.Module, batches: Iterable[torch.Tensor], w_bits: int = 4, a_bits: int = 8,
                        quant_type: QuantizationType = QuantizationType.SYMMETRIC_NONLINEAR, num: int = 32,
                        min_frac: float = 0.2) -> Tuple[nn.Module, Dict[str, Tuple[QuantChoice, QuantChoice]]]:
    """An fp32 model on a ROCm device to its W{w_bits}A{a_bits} form with searched quantizers: the activation search
    on the fp32 model, model_to_quantize_model (WEIGHT_AND_ACTIVATION), the weight search, apply_quant_choices, and
    prepare() on every layer. Returns (model, report), report[name] = (activation choice, weight choice); a choice
    whose step had to be widened to stay on the integer path says so (QuantChoice.widened)."""
    act = search_activation_quant(model, batches, bits=a_bits, t=1.0, quant_type=quant_type, num=num,
                                  min_frac=min_frac)
    model = model_to_quantize_model(model, num_bits=w_bits, quant_type=quant_type,
                                    quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    wt = search_weight_quant(model, bits=w_bits, num=num, min_frac=min_frac)
    layers = {name: mod for name, mod in model.named_modules() if isinstance(mod, (QuantizeLinear, QuantizeConv2d))}
    act = {n: _fit_level(c, _qtype_code(layers[n].quant_type), a_bits) for n, c in act.items() if n in layers}
    wt = {n: _fit_level(c, _qtype_code(layers[n].quant_type), w_bits) for n, c in wt.items()}
    apply_quant_choices(model, act=act, wt=wt)
    for mod in layers.values():
        mod.prepare()
    return model, {n: (act.get(n), wt[n]) for n in layers}
