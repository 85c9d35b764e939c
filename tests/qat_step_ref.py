"""Two restatements of the quantization-aware step of the reference's GETA optimizer, written from the formulas of
OTO/optimizer/base_optimizer.py:18-86 (moments, grad_variant) and OTO/optimizer/geta.py:571-596 (warm-up step),
:598-697 (range stage, weight pass then activation pass), :723-804 (fix stage, _bit_width_helper, _d_quant_helper)
and :873-943 (the stage machine and the bit schedule), with the pruning stages absent:

  (a) StepF64   the whole step in float64 NumPy;
  (b) StepTorch a per-parameter fp32 torch-CPU loop that reads q_m and t_quant back with .item(), as the reference
                does.

Both take `params`: an ordered {name: fp32 array / tensor}; a parameter named "<layer>.d_quant_wt" (q_m_wt,
t_quant_wt, d_quant_act, ...) is a quantizer scalar of <layer>. A layer's scalars are found by the exact layer name
(the reference tests `layer_name in p_name`, a substring test under which "l1" would also take the scalars of
"l10"). d(b) and the bit width are evaluated in double from the fp32 scalars; the clamp bounds are then rounded to
fp32 as torch's clamp rounds a Python float.
"""
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

WARMUP, RANGE, FIX = 0, 1, 2
SAFE_GUARD = 1e-8


@dataclass
class Hyper:
    variant: str = "sgd"
    lr: float = 1e-2
    lr_quant: float = 1e-3
    first_momentum: Optional[float] = None
    second_momentum: Optional[float] = None
    dampening: Optional[float] = None
    weight_decay: Optional[float] = None
    start_projection_step: int = 0
    projection_steps: int = 1
    projection_periods: int = 1
    fix_after_step: int = 2
    bit_reduction: int = 2
    min_bit_wt: int = 4
    max_bit_wt: int = 16
    min_bit_act: int = 4
    max_bit_act: int = 16
    grad_clip: Optional[Tuple[float, float]] = None


def is_scalar(name: str) -> bool:
    return any(k in name for k in ("d_quant", "t_quant", "q_m"))


def layer_of(name: str) -> str:
    return ".".join(name.split(".")[:-1])


def d_of_bits(bit_width: int, q_m: float, t_quant: Optional[float]) -> float:
    """_d_quant_helper (geta.py:787-804) on Python floats."""
    t = 1.0 if t_quant is None else t_quant
    q = max(abs(q_m), 1e-10)
    return math.exp(t * math.log(q)) / (2 ** (bit_width - 1) - 1)


def bit_width(d_quant: float, q_m: float, t_quant: Optional[float]) -> float:
    """_bit_width_helper (geta.py:774-785) on Python floats."""
    t = 1.0 if t_quant is None else t_quant
    return math.log2(math.exp(t * math.log(abs(q_m))) / abs(d_quant) + 1) + 1


class _Machine:
    """The stage machine and bit schedule of GETA.step (geta.py:881-943) without pruning; fix_after_step stands
    for start_pruning_step (+ pruning_steps = 0)."""

    def __init__(self, hp: Hyper):
        self.hp = hp
        self.num_steps = 0
        self.max_bit_wt, self.max_bit_act = hp.max_bit_wt, hp.max_bit_act
        self.period = hp.projection_steps // hp.projection_periods

    def advance(self) -> int:
        hp = self.hp
        self.num_steps += 1
        n = self.num_steps
        if hp.start_projection_step <= n <= hp.fix_after_step and hp.start_projection_step != hp.fix_after_step:
            s = n - hp.start_projection_step - 1
            if s % self.period == 0 and s != 0:
                self.max_bit_wt = max(hp.min_bit_wt, 6, self.max_bit_wt - hp.bit_reduction)
                self.max_bit_act = max(hp.min_bit_act, 6, self.max_bit_act - hp.bit_reduction)
        if n <= hp.start_projection_step:
            return WARMUP
        return FIX if n > hp.fix_after_step else RANGE

    def layers(self, names):
        out = []
        for n in names:
            if "d_quant" in n and layer_of(n) not in out:
                out.append(layer_of(n))
        return out


# ---- (a) float64 NumPy ------------------------------------------------------------------------------------------
class StepF64(_Machine):
    def __init__(self, params: Dict[str, np.ndarray], hp: Hyper):
        super().__init__(hp)
        self.p = {k: np.asarray(v, dtype=np.float64).copy() for k, v in params.items()}
        self.m: Dict[str, np.ndarray] = {}
        self.v: Dict[str, np.ndarray] = {}
        self.bits: Dict[str, Dict[str, int]] = {}

    def _variant(self, grads):
        hp, n = self.hp, self.num_steps
        adam = hp.variant in ("adam", "adamw")
        gv = {}
        for k, p in self.p.items():
            g = grads.get(k)
            if g is None:
                continue
            g = np.asarray(g, dtype=np.float64).copy()
            if hp.grad_clip is not None:
                g = np.clip(g, hp.grad_clip[0], hp.grad_clip[1])
            if hp.weight_decay is not None and hp.variant != "adamw":
                g = g + hp.weight_decay * p
            if not adam:
                b1, damp = hp.first_momentum or 0.0, hp.dampening or 0.0
                if b1 > 0.0:
                    self.m[k] = g.copy() if k not in self.m else self.m[k] * b1 + (1.0 - damp) * g
                    g = self.m[k]
                gv[k] = g
                continue
            b1, b2 = hp.first_momentum, hp.second_momentum
            m = g
            if b1 > 0:
                self.m[k] = g.copy() if k not in self.m else self.m[k] * b1 + (1.0 - b1) * g
                m = self.m[k]
            v = g * g
            if b2 > 0:
                self.v[k] = g * g if k not in self.v else self.v[k] * b2 + (1.0 - b2) * (g * g)
                v = self.v[k]
            gv[k] = (m / (1.0 - b1 ** n)) / (np.sqrt(v / (1.0 - b2 ** n)) + SAFE_GUARD)
        return gv

    def _descend(self, k, gv, lr):
        hp = self.hp
        if hp.weight_decay is not None and hp.variant == "adamw":
            self.p[k] = self.p[k] - lr * (hp.weight_decay * self.p[k])
        self.p[k] = self.p[k] - lr * gv

    def _scalars(self, layer, side):
        q = float(self.p[f"{layer}.q_m_{side}"].reshape(-1)[0])
        t = self.p.get(f"{layer}.t_quant_{side}")
        return q, (None if t is None else float(t.reshape(-1)[0]))

    def bounds(self, layer, side):
        """(d(max_bit), d(min_bit)) of the layer's current scalars, in double."""
        q, t = self._scalars(layer, side)
        lo_b, hi_b = (self.max_bit_wt, self.hp.min_bit_wt) if side == "wt" else (self.max_bit_act, self.hp.min_bit_act)
        return d_of_bits(lo_b, q, t), d_of_bits(hi_b, q, t)

    def step(self, grads):
        stage = self.advance()
        hp = self.hp
        gv = self._variant(grads)
        if stage == FIX and not self.bits:
            for layer in self.layers(self.p):
                self.bits[layer] = {}
                for side, key in (("wt", "weight"), ("act", "activation")):
                    if f"{layer}.d_quant_{side}" in self.p:
                        q, t = self._scalars(layer, side)
                        d = float(self.p[f"{layer}.d_quant_{side}"].reshape(-1)[0])
                        self.bits[layer][key] = round(bit_width(d, q, t))
        for k in self.p:
            if k not in gv:
                continue
            if stage == RANGE and is_scalar(k) and k.endswith("_act"):
                self._descend(k, gv[k], hp.lr)          # the weight pass takes it for a dense parameter
                self._descend(k, gv[k], hp.lr_quant)    # the activation pass steps it again
            else:
                self._descend(k, gv[k], hp.lr_quant if is_scalar(k) else hp.lr)
        if stage == WARMUP:
            return stage
        for layer in self.layers(self.p):
            for side, key in (("wt", "weight"), ("act", "activation")):
                dk = f"{layer}.d_quant_{side}"
                if dk not in self.p:
                    continue
                if stage == RANGE:
                    lo, hi = self.bounds(layer, side)
                else:
                    q, t = self._scalars(layer, side)
                    lo = hi = d_of_bits(self.bits[layer][key], q, t)
                # torch's clamp rounds a Python float bound to the tensor's fp32
                self.p[dk] = np.clip(self.p[dk], float(np.float32(lo)), float(np.float32(hi)))
        return stage


# ---- (b) fp32 torch on the CPU, one parameter at a time -----------------------------------------------------------
class StepTorch(_Machine):
    def __init__(self, params: Dict[str, torch.Tensor], hp: Hyper):
        super().__init__(hp)
        self.p = {k: torch.as_tensor(v, dtype=torch.float32).clone() for k, v in params.items()}
        self.m: Dict[str, torch.Tensor] = {}
        self.v: Dict[str, torch.Tensor] = {}
        self.bits: Dict[str, Dict[str, int]] = {}

    def _moment(self, store, k, mom, damp, g):
        if mom > 0:
            if k not in store:
                buf = store[k] = g
            else:
                buf = store[k]
                buf.mul_(mom).add_(g, alpha=(1.0 - damp))
            return buf
        return g

    def _variant(self, grads):
        hp, n = self.hp, self.num_steps
        adam = hp.variant in ("adam", "adamw")
        bc1 = 1.0 - hp.first_momentum ** n if adam else None
        bc2 = 1.0 - hp.second_momentum ** n if adam else None
        gv = {}
        for k, p in self.p.items():
            g = grads.get(k)
            if g is None:
                continue
            g = torch.as_tensor(g, dtype=torch.float32).clone()
            if hp.grad_clip is not None:
                g = g.clamp(min=hp.grad_clip[0], max=hp.grad_clip[1])
            if hp.weight_decay is not None and hp.variant != "adamw":
                g += hp.weight_decay * p
            if not adam:
                b1, damp = hp.first_momentum or 0.0, hp.dampening or 0.0
                if b1 > 0.0 or damp > 0.0:
                    g = self._moment(self.m, k, b1, damp, g)
                gv[k] = g
            else:
                m = self._moment(self.m, k, hp.first_momentum, hp.first_momentum, g)
                v = self._moment(self.v, k, hp.second_momentum, hp.second_momentum, g * g)
                denom = (v / bc2).sqrt().add_(SAFE_GUARD)
                gv[k] = (m / bc1) / denom
        return gv

    def _descend(self, k, gv, lr):
        hp, p = self.hp, self.p[k]
        if hp.weight_decay is not None and hp.variant == "adamw":
            p.add_(hp.weight_decay * p, alpha=-lr)
        p.add_(gv, alpha=-lr)

    def _scalars(self, layer, side):
        q = self.p[f"{layer}.q_m_{side}"].abs().max().item()
        t = self.p.get(f"{layer}.t_quant_{side}")
        return q, (None if t is None else t.item())

    def step(self, grads):
        stage = self.advance()
        hp = self.hp
        gv = self._variant(grads)
        if stage == FIX and not self.bits:
            for layer in self.layers(self.p):
                self.bits[layer] = {}
                for side, key in (("wt", "weight"), ("act", "activation")):
                    if f"{layer}.d_quant_{side}" in self.p:
                        q, t = self._scalars(layer, side)
                        self.bits[layer][key] = round(bit_width(self.p[f"{layer}.d_quant_{side}"].item(), q, t))
        for k in self.p:
            if k not in gv:
                continue
            if stage == RANGE and is_scalar(k) and k.endswith("_act"):
                self._descend(k, gv[k], hp.lr)
                self._descend(k, gv[k], hp.lr_quant)
            else:
                self._descend(k, gv[k], hp.lr_quant if is_scalar(k) else hp.lr)
        if stage == WARMUP:
            return stage
        for layer in self.layers(self.p):
            for side, key in (("wt", "weight"), ("act", "activation")):
                dk = f"{layer}.d_quant_{side}"
                if dk not in self.p:
                    continue
                q, t = self._scalars(layer, side)
                if stage == RANGE:
                    lo_b, hi_b = (self.max_bit_wt, hp.min_bit_wt) if side == "wt" else \
                        (self.max_bit_act, hp.min_bit_act)
                    lo, hi = d_of_bits(lo_b, q, t), d_of_bits(hi_b, q, t)
                else:
                    lo = hi = d_of_bits(self.bits[layer][key], q, t)
                self.p[dk].clamp_(min=lo, max=hi)
        return stage
