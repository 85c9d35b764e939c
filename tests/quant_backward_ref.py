"""Restatement of the reference's quantizer backwards, from their formulas, for the backward tests.

  SymQuantizerNonLinear.backward  OTO/quantization/quant_layers.py:71-125
  SymQuantizerLinear.backward     OTO/quantization/quant_layers.py:163-205
  DGEQuantizer.backward           OTO/quantization/quant_layers.py:248-290
(OTO = QViT_with_GETA/only_train_once), with q_s = 0 as in every caller (:335, :362). Runs on the CPU in the
dtype asked for: float64 is the yardstick, float32 shows what the reference's own arithmetic gives.

Also here: the tie-free input construction the tests share, the error floor of the three sums, and float64
autograd Functions (forward :41-69 / :137-161) for a CPU graph of a whole layer.
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np
import torch

LINEAR, NONLINEAR = "linear", "nonlinear"


def _scalar(v, dtype):
    # parameters are float32 in the reference (nn.Parameter): every dtype sees the same float32 value
    return torch.tensor(float(np.float32(v)), dtype=dtype)


def quant_forward_ref(x, kind, d, q_m, t=None, dtype=torch.float64):
    """The fake-quant forward (:41-69, :137-161): sign(x) d rne(p(|x|) / d), saturated where |x| >= q_m, zero
    where |x| <= 0."""
    x = x.to(dtype)
    d, q_m = _scalar(d, dtype), _scalar(q_m, dtype)
    a = x.abs()
    if kind == LINEAR:
        p, rp = a, q_m.abs()
    else:
        t = _scalar(t, dtype)
        p = torch.exp(t * torch.log(a))
        rp = torch.exp(t * torch.log(q_m.abs() + 1e-6))
    out = d * torch.round(p / d)
    out = torch.where(a >= q_m, d * torch.round(rp / d), out)
    out = torch.where(a <= 0, torch.zeros_like(out), out)
    return torch.sign(x) * out


def quant_backward_ref(x, g, kind, d, q_m, t=None, clip=(-2.0, 2.0), dge_k=0.0, dtype=torch.float64):
    """Returns a dict: grad_x; sums (d, q_m, t) of g * term; terms (the three per-element terms); abs_sums
    (sum |g * term|); q (the quotient each element's d term was formed from: p / d, range_pow / d where
    saturated, 0 where |x| <= 0); t_ln_a (t ln |x|, 0 at x = 0 and for the linear quantizer)."""
    x, g = x.to(dtype).reshape(-1), g.to(dtype).reshape(-1)
    d, q_m = _scalar(d, dtype), _scalar(q_m, dtype)
    a, sgn = x.abs(), torch.sign(x)
    zero = torch.zeros_like(x)
    is_zero, is_sat = a <= 0, a >= q_m

    # grad_x: straight-through inside the clip range (:77-79, :169-171, :255-257)
    grad_x = torch.where((x >= clip[1]) | (x <= clip[0]), zero, g)
    if dge_k > 0:   # :259-265, k = 5 * 4 / num_bits (:236) held in float32 by the reference
        k = _scalar(dge_k, dtype)
        scale = (1 / k) * torch.pow((x - d / 2).abs(), 1 / k - 1)
        grad_x = torch.clamp(grad_x * scale, -3.0, 3.0)

    if kind == LINEAR:
        p, rp = a, q_m.abs()                                     # :174-175
        qm_coef = torch.ones((), dtype=dtype)                    # :185
        ln_a = zero
        t_ln_a = zero
    else:
        t = _scalar(t, dtype)
        ln_a = torch.log(a)
        ln_qm = torch.log(q_m.abs() + 1e-6)
        p, rp = torch.exp(t * ln_a), torch.exp(t * ln_qm)        # :81-87
        qm_coef = t * torch.exp((t - 1) * ln_qm)                 # :84-86, :97
        t_ln_a = torch.where(is_zero, zero, t * ln_a)
    q = p / d
    sat_q = rp / d

    # d term (:89-94, :177-182); the masks select, in the reference's order (zero last)
    term_d = torch.round(q) - q
    term_d = torch.where(is_sat, torch.round(sat_q) - sat_q, term_d)
    term_d = sgn * torch.where(is_zero, zero, term_d)
    # q_m term (:97-98, :185-186): kept only where |x| > q_m
    term_qm = torch.where(a <= q_m, zero, sgn * qm_coef)
    # t term (:101-104)
    if kind == LINEAR:
        term_t = zero
    else:
        term_t = torch.where(is_sat, rp * ln_qm, p * ln_a)
        term_t = sgn * torch.where(is_zero, zero, term_t)

    terms = (term_d, term_qm, term_t)
    q_sel = torch.where(is_zero, zero, torch.where(is_sat, sat_q.expand_as(q), q))
    return {
        "grad_x": grad_x,
        "sums": tuple(torch.sum(g * tm) for tm in terms),        # :95, :99, :105, :183, :187
        "terms": terms,
        "abs_sums": tuple(torch.sum((g * tm).abs()) for tm in terms),
        "q": q_sel,
        "t_ln_a": t_ln_a,
    }


def sum_floor(ref64: dict, g, kind, c_scale: float = 1.0) -> float:
    """floor = 2^-23 sum |g_i| (1 + |q_i|) c_i from the float64 restatement: one rounding in q and one in the
    product, and for the nonlinear quantizer a few ulp through exp / log scaled by the exponent:
    c_i = 1 (linear), 4 (1 + |t ln a_i|) (nonlinear)."""
    g = g.double().reshape(-1)
    c = torch.ones_like(g) if kind == LINEAR else 4.0 * (1.0 + ref64["t_ln_a"].double().abs())
    return float(2.0 ** -23 * torch.sum(g.abs() * (1.0 + ref64["q"].double().abs()) * c)) * c_scale


def sum_bounds(x, g, kind, d, q_m, t=None, clip=(-2.0, 2.0)):
    """(ref64 dict, ref32 dict, floor, [bound for each of the three sums]) with
    bound = 4 max(|ref32 - ref64|, floor)."""
    r64 = quant_backward_ref(x, g, kind, d, q_m, t, clip, dtype=torch.float64)
    r32 = quant_backward_ref(x, g, kind, d, q_m, t, clip, dtype=torch.float32)
    floor = sum_floor(r64, g, kind)
    bounds = [4.0 * max(abs(float(s32) - float(s64)), floor) for s32, s64 in zip(r32["sums"], r64["sums"])]
    return r64, r32, floor, bounds


# ---- inputs ----------------------------------------------------------------------------------------
# (kind, d, q_m, t): the linear set, a negative q_m, and the t values tests/test_gpu_kernels.py uses
PARAM_SETS = [
    (LINEAR, 0.05, 0.37, None),
    (LINEAR, 0.05, -0.37, None),
    (NONLINEAR, 0.05, 0.37, 0.9),
    (NONLINEAR, 0.05, 0.37, 1.0),
    (NONLINEAR, 0.05, 0.37, 1.25),
]
CLIPS = [(-2.0, 2.0), (-0.2, 0.3)]
SIZES = [1, 63, 64, 65, 1023, 4099, 1024 * 256 * 4 + 4099]


def saturation_level(kind, d, q_m, t=None) -> int:
    d, q_m = float(np.float32(d)), float(np.float32(q_m))
    rp = abs(q_m) if kind == LINEAR else math.exp(float(np.float32(t)) * math.log(abs(q_m) + 1e-6))
    return int(round(rp / d))


def tie_free_values(shape, kind, d, q_m, t=None, seed=0) -> torch.Tensor:
    """x = sign P^-1(d (k + f)) rounded to float32: integer codes k over 0 .. L + 2 and f uniform in
    [-0.45, 0.45], so p(|x|) / d stays 0.05 away from every rounding tie by construction (a tie would make
    float32 and float64 disagree by a whole |g|). P^-1 is the identity or y^(1/t) in float64."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    L = saturation_level(kind, d, q_m, t)
    k = rng.integers(0, L + 3, size=n).astype(np.float64)
    f = rng.uniform(-0.45, 0.45, size=n)
    y = np.abs(float(np.float32(d)) * (k + f))
    if kind == NONLINEAR:
        y = y ** (1.0 / float(np.float32(t)))
    sign = rng.choice([-1.0, 1.0], size=n)
    return torch.from_numpy((sign * y).astype(np.float32)).reshape(shape)


def boundary_values(q_m, clip) -> torch.Tensor:
    f = np.float32
    qa = f(abs(float(q_m)))
    lo, hi = f(clip[0]), f(clip[1])
    inf = f(np.inf)
    vals = [f(0.0), f(-0.0), qa, -qa, np.nextafter(qa, inf), np.nextafter(qa, -inf), -np.nextafter(qa, inf),
            -np.nextafter(qa, -inf), lo, hi, np.nextafter(lo, -inf), np.nextafter(hi, inf)]
    return torch.from_numpy(np.array(vals, dtype=np.float32))


@lru_cache(maxsize=None)
def make_inputs(n: int, kind, d, q_m, t=None, clip=(-2.0, 2.0), seed=0):
    """(x, g) float32 of n elements: tie-free values with the boundary elements at the end (so they also run
    through the kernel's scalar tail) whenever n leaves room for them, and a normal grad_out."""
    x = tie_free_values((n,), kind, d, q_m, t, seed)
    b = boundary_values(q_m, clip)
    if n > b.numel():
        x[n - b.numel():] = b
    gen = torch.Generator().manual_seed(seed + 1)
    g = torch.randn(n, generator=gen, dtype=torch.float32)
    return x, g


# ---- float64 autograd graph of a layer -------------------------------------------------------------------
class RefQuantizer(torch.autograd.Function):
    """The quantizer as a CPU autograd Function in float64. `rec`, a dict, receives the grad_out the backward
    saw (the composed gradient the device quantizer has to be compared on)."""

    @staticmethod
    def forward(ctx, x, d, q_m, t, kind, clip, rec):
        ctx.save_for_backward(x, d, q_m, t)
        ctx.kind, ctx.clip, ctx.rec = kind, clip, rec
        return quant_forward_ref(x, kind, float(d), float(q_m), None if t is None else float(t))

    @staticmethod
    def backward(ctx, grad_out):
        x, d, q_m, t = ctx.saved_tensors
        tv = None if t is None else float(t)
        r = quant_backward_ref(x, grad_out, ctx.kind, float(d), float(q_m), tv, ctx.clip)
        ctx.rec["grad_out"] = grad_out.detach().clone()
        one = lambda v: v.reshape(1).to(torch.float64)
        return (r["grad_x"].view_as(x), one(r["sums"][0]), one(r["sums"][1]),
                None if t is None else one(r["sums"][2]), None, None, None)
