"""Restatement of LayerNorm -> activation quantizer and GELU -> activation quantizer backwards for the train-fusion
tests, on top of quant_backward_ref (the quantizer's own restatement). Runs on the CPU in the dtype asked for:
float64 is the yardstick, float32 shows what plain float32 arithmetic gives.

Also here: the input construction the tests share (rows whose LayerNorm / GELU value lies next to a rounding tie,
q_m or a clip bound are dropped: there float32 and float64 legitimately take different branches), and the error
floors.

Floors (eps = 2^-23, everything from the float64 restatement):
  * xhat = (x - mean) rstd carries xe eps with xe = 2 |xhat| + |mean| rstd + 1: its own two roundings, the row
    mean's error eps mean|x| <= eps (|mean| + spread) scaled by rstd, and rstd's relative error.
  * grad_x of the LayerNorm backward, dx = rstd (a - mean(a) - xhat mean(a xhat)), a = gamma gy, m = row mean:
      floor = eps rstd (2 |a| + 2 m|a| + xe m|a xhat| + |xhat| (m|a xhat| + m(|a| xe))).
  * grad_gamma / grad_beta: eps sum_rows |gy| xe and eps sum_rows |gy|.
  * grad_h of the GELU backward, GELU'(h) gy with GELU' = Phi + h phi: roundings of the two terms, plus the
    absolute error of the forward's erf (Abramowitz-Stegun 7.1.26: 1.5e-7, halved in Phi) and of 1 + erf (2^-24):
      floor = |gy| (eps (Phi + 3 |h phi|) + 1.4e-7).
  * the three scalar sums: quant_backward_ref.sum_floor (one rounding in q, one in the product, exp / log for the
    nonlinear quantizer), plus what the pre-op's own error delta in the quantizer's input a does to each term
    through its derivative (interior elements only; the saturated and zero regions are constants):
      d term  |dq/da| = t a^(t-1) / d,   t term  |d(p ln a)/da| = a^(t-1) |1 + t ln a|,   q_m term 0,
    evaluated at max(a, delta) and doubled (an element within delta of zero can change sign).
    delta = eps (xe |gamma| + |y| + |beta|) for LayerNorm; (0.75e-7 + 2^-24) |h| + eps |a| for GELU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import quant_backward_ref as R
from quant_backward_ref import LINEAR, NONLINEAR  # noqa: F401

EPS32 = 2.0 ** -23
MARGIN = 64.0 * 2.0 ** -24      # of max(1, |q|): distance a float64 value keeps from every branch point
LN_EPS = 1e-6                   # Block.norm1 / norm2


# ---- forward pieces ------------------------------------------------------------------------------------------
def layernorm_ref(x, gamma, beta, eps=LN_EPS, dtype=torch.float64):
    """(y, xhat, mean, rstd) of LayerNorm over the last dimension."""
    x, gamma, beta = x.to(dtype), gamma.to(dtype), beta.to(dtype)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    return xhat * gamma + beta, xhat, mean, rstd


def gelu_ref(h, dtype=torch.float64):
    """(GELU(h), GELU'(h)) for the exact GELU: h Phi(h) and Phi(h) + h phi(h)."""
    h = h.to(dtype)
    cdf = 0.5 * (1.0 + torch.erf(h * math.sqrt(0.5)))
    pdf = torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)
    return h * cdf, cdf + h * pdf


# ---- backward restatements -----------------------------------------------------------------------------------
def ln_quant_backward_ref(x, gamma, beta, g, kind, d, q_m, t=None, clip=(-2.0, 2.0), eps=LN_EPS,
                          dtype=torch.float64):
    """Backward of quantize(LayerNorm(x)) given g = d loss / d quantizer output, x and g [rows, cols]. Returns a
    dict: grad_x, grad_gamma, grad_beta, sums (d, q_m, t), masked (gy == 0 by the clip mask), and the pieces the
    floors need (q: the quantizer restatement's dict at y; y, xhat, mean, rstd, gy)."""
    y, xhat, mean, rstd = layernorm_ref(x, gamma, beta, eps, dtype)
    q = R.quant_backward_ref(y, g, kind, d, q_m, t, clip, dtype=dtype)
    gy = q["grad_x"].view_as(y)
    a = gamma.to(dtype) * gy
    dx = rstd * (a - a.mean(-1, keepdim=True) - xhat * (a * xhat).mean(-1, keepdim=True))
    return {"grad_x": dx, "grad_gamma": (gy * xhat).sum(0), "grad_beta": gy.sum(0), "sums": q["sums"],
            "masked": (y >= clip[1]) | (y <= clip[0]), "q": q, "y": y, "xhat": xhat, "mean": mean, "rstd": rstd,
            "gy": gy}


def gelu_quant_backward_ref(h, g, kind, d, q_m, t=None, clip=(-2.0, 2.0), dtype=torch.float64):
    """Backward of quantize(GELU(h)) over flat h, g. Returns grad_h, sums, masked and the floors' pieces."""
    h = h.reshape(-1)
    a, slope = gelu_ref(h, dtype)
    q = R.quant_backward_ref(a, g, kind, d, q_m, t, clip, dtype=dtype)
    gy = q["grad_x"]
    return {"grad_h": slope * gy, "sums": q["sums"], "masked": (a >= clip[1]) | (a <= clip[0]), "q": q, "a": a,
            "slope": slope, "gy": gy}


# ---- floors --------------------------------------------------------------------------------------------------
def _xhat_err(r64):
    """|error of xhat| / eps: two roundings of its own, the row mean's error eps mean|x| <= eps (|mean| + spread)
    scaled by rstd, and rstd's relative error on a value of order one."""
    return 2.0 * r64["xhat"].abs() + r64["mean"].abs() * r64["rstd"] + 1.0


def ln_grad_x_floor(r64, gamma):
    a = (gamma.double() * r64["gy"]).abs()
    xh, xe = r64["xhat"].abs(), _xhat_err(r64)
    m = lambda v: v.mean(-1, keepdim=True)
    return EPS32 * r64["rstd"] * (2.0 * a + 2.0 * m(a) + xe * m(a * xh) + xh * (m(a * xh) + m(a * xe)))


def ln_col_floors(r64):
    gy = r64["gy"].abs()
    return EPS32 * (gy * _xhat_err(r64)).sum(0), EPS32 * gy.sum(0)


def gelu_grad_h_floor(r64, h):
    h = h.double().reshape(-1)
    cdf = 0.5 * (1.0 + torch.erf(h * math.sqrt(0.5)))
    hpdf = (h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)).abs()
    return r64["gy"].abs() * (EPS32 * (cdf + 3.0 * hpdf) + 1.4e-7)


def ln_input_delta(r64, gamma, beta):
    return EPS32 * (_xhat_err(r64) * gamma.double().abs() + r64["y"].abs() + beta.double().abs())


def gelu_input_delta(r64, h):
    return (0.75e-7 + 2.0 ** -24) * h.double().reshape(-1).abs() + EPS32 * r64["a"].abs()


def sum_floors(r64, g, kind, d, q_m, t, delta):
    """[floor of the d, q_m, t sums]: quant_backward_ref.sum_floor plus the propagated input error (see the module
    docstring). `r64` is a restatement dict (its "q" entry is the quantizer's), `delta` the input's error bound."""
    base = R.sum_floor(r64["q"], g, kind)
    g = g.double().reshape(-1).abs()
    a = (r64["y"] if "y" in r64 else r64["a"]).double().reshape(-1).abs()
    delta = delta.double().reshape(-1)
    interior = a < abs(float(np.float32(q_m)))
    ae = torch.maximum(a, delta).clamp(min=1e-300)   # (an exact zero has delta = 0 and adds nothing)
    dd = float(np.float32(d))
    if kind == LINEAR:
        dq, dt = torch.full_like(a, 1.0 / dd), torch.zeros_like(a)
    else:
        tt = float(np.float32(t))
        dq = tt * ae ** (tt - 1.0) / dd
        dt = ae ** (tt - 1.0) * (1.0 + tt * torch.log(ae)).abs()
    w = 2.0 * g * delta * interior
    return [base + float((w * dq).sum()), base, base + float((w * dt).sum())]


# ---- inputs --------------------------------------------------------------------------------------------------
def branch_distance_ok(a64, kind, d, q_m, t, clip):
    """Elementwise: the float64 quantizer input a64 keeps MARGIN max(1, |q|) from every branch point, measured on
    the scale of the quotient q = p(|a|) / d: from every rounding tie of q (where the element is not saturated),
    from q_m (as |p(|a|) - p(|q_m|)| / d) and from both clip bounds (as |a - clip| / d)."""
    a = a64.double().abs()
    dd, qm = float(np.float32(d)), abs(float(np.float32(q_m)))
    tt = 1.0 if kind == LINEAR else float(np.float32(t))
    q = a ** tt / dd
    m = MARGIN * torch.clamp(q, min=1.0)
    tie = ((q - (torch.floor(q) + 0.5)).abs() > m) | (a >= qm)   # a saturated element rounds no quotient
    return (tie & ((q - qm ** tt / dd).abs() > m) & ((a64.double() - clip[0]).abs() / dd > m)
            & ((a64.double() - clip[1]).abs() / dd > m))


def ln_inputs(rows, cols, kind, d, q_m, t, clip, seed=0):
    """(x, gamma, beta, g, kept fraction): float32 rows drawn at random; a row is dropped when any element of its
    float64 y fails branch_distance_ok. The caller asserts the kept fraction. y spreads over about +-3 q_m, so
    every region (interior, saturated, clipped by the narrow clip) occurs."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * rows + cols)
    draw = rows + max(rows // 4, 64)
    x = torch.randn(draw, cols, generator=gen) * 1.7 + 0.3 * torch.randn(draw, 1, generator=gen)
    s = 1.2 * abs(q_m)
    gamma = (s * (1.0 + 0.2 * torch.randn(cols, generator=gen))).float()
    beta = (0.1 * s * torch.randn(cols, generator=gen)).float()
    y = layernorm_ref(x, gamma, beta)[0]
    keep = branch_distance_ok(y, kind, d, q_m, t, clip).all(-1)
    frac = float(keep.double().mean())
    x = x[keep][:rows].contiguous()
    assert x.shape[0] == rows, f"only {x.shape[0]} of {rows} rows survive the filter"
    g = torch.randn(rows, cols, generator=gen)
    return x, gamma, beta, g, frac


def gelu_inputs(n, kind, d, q_m, t, clip, seed=0):
    """(h, g, kept fraction): h uniform over +-6 (both tails, the slope maximum near 1.41) with the elements
    whose float64 GELU fails branch_distance_ok dropped."""
    gen = torch.Generator().manual_seed(1000 * seed + n)
    draw = n + n // 4 + 64
    h = (torch.rand(draw, generator=gen) * 12.0 - 6.0).float()
    keep = branch_distance_ok(gelu_ref(h)[0], kind, d, q_m, t, clip)
    frac = float(keep.double().mean())
    h = h[keep][:n].contiguous()
    assert h.numel() == n, f"only {h.numel()} of {n} elements survive the filter"
    g = torch.randn(n, generator=gen)
    return h, g, frac


# ---- the cases the CPU and GPU tests share -----------------------------------------------------------------------
# train_fuse.hip: one wave per row, kWaves = 4 rows per workgroup, at most kGridCap = 1024 workgroups
LN_WAVES, LN_GRID_CAP = 4, 1024
LN_SHAPES = [(1, 4), (5, 64), (3, 260), (333, 192), (7, 768), (5, 1024), (3, 1280), (2, 2048),
             # cols = 8: every wave of a full grid takes a second row, and 37 rows more start a third trip
             (2 * LN_WAVES * LN_GRID_CAP + 37, 8)]
QUANTIZERS = [R.PARAM_SETS[0], R.PARAM_SETS[2]]          # linear; nonlinear, t = 0.9
GELU_GRID_CAP = 1024                                     # workgroups of 256 threads x 4 floats
GELU_SIZES = R.SIZES + [2 * GELU_GRID_CAP * 256 * 4 + 4099]
