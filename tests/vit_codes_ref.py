"""The device quantizer of the ViT int8 kernels (csrc/qvit_common.h: quant_code + to_i8_sat) restated on the CPU, the
inputs that walk it one ulp at a time across every code boundary, and the tie-proven comparison for values that a
test cannot set exactly. Nothing here imports the package.

Bit equality. A kernel whose pre-quantization value is known exactly (the value itself, a GEMM's bias under zero
activation codes, a constant LayerNorm row's beta, attention over one key) must return `device_codes` of that value.
The only freedom is the double rounding of the nonlinear quantizer's log and exp: the device rounds ocml's fp64
result to fp32, the CPU rounds libm's, both fp64 results are within 1 fp64 ulp (2^-29 of an fp32 ulp) of the true
value, so the fp32 results can differ only where the fp64 value lies that close to an fp32 rounding midpoint.
`double_rounding_mask` marks a 2^-20 ulp neighbourhood of the midpoints (512 times the possible disagreement);
outside it equality is required. The linear and ULTRA_ACT quantizers use IEEE fp32 operations only: empty mask.

Possible ties. Where the kernel's fp32 value v is known only to within delta of an fp64 reference v64 (random GEMM,
LayerNorm and attention data), `bracket_ties` marks the elements whose code changes anywhere in [v64 - delta,
v64 + delta]; every other code must equal the reference's (ultra_ref.assert_codes_tie_proven). The deltas:
  GEMM epilogue   4 eps32 (|alpha acc| + |bias|): the integer accumulator is exact; one product and one sum, fused or
                  not, are at most 2 roundings of a magnitude below that sum (derived, not measured).
  LayerNorm       C_LN e32(row), e32(row) = max |F.layer_norm fp32 - fp64| over the row on the CPU, floored at
                  eps32 max |y64|; C_LN from the measured per-arm figures.
  attention       2e-6 max |out64|: the bar of the fp32 output (test_gpu_attention.py::test_attention_fp32_vs_fp64).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import quant_oracle as O
from oracle.ties import cr_codes

ULTRA_ACT = "ultra_act"
EPS32 = 2.0 ** -24                 # half an fp32 ulp, relative: the bound of one rounding
CAP_GEMM = CAP_LN = 1e-3           # possible-tie shares allowed (conditions, checked on the reference alone)
CAP_ATTN = 2e-3
CAP_DOUBLE_ROUNDING = 1e-5
C_LN = 2.0                         # the next power of two >= 2 x the worst measured figure (0.63)
ATTN_REL_DELTA = 2e-6


def _f32(v) -> torch.Tensor:
    return torch.tensor([float(v)], dtype=torch.float32)


def _log_cr(a: torch.Tensor) -> torch.Tensor:
    return torch.log(a.double()).float()


def _exp_cr(a: torch.Tensor) -> torch.Tensor:
    return torch.exp(a.double()).float()


def saturation_code(qt: str, d: float, qm: float, t: float = 1.0) -> float:
    """load_qparams' L: rint(|q_m| / d), or rint(exp_cr(t log_cr(|q_m| + 1e-6)) / d), every step in fp32."""
    aq = _f32(qm).abs()
    if qt == O.NONLINEAR:
        aq = _exp_cr(_f32(t) * _log_cr(aq + _f32(1e-6)))
    return float(torch.round(aq / _f32(d)))


def device_codes(x: torch.Tensor, qt: str, d: float, qm: float, t: float = 1.0, levels: int = 0) -> torch.Tensor:
    """to_i8_sat(quant_code(x)) on an fp32 tensor -> int8."""
    assert x.dtype == torch.float32
    if qt == ULTRA_ACT:
        c = torch.where(torch.isnan(x), torch.zeros_like(x), x).clamp(0.0, 1.0)      # fmaxf(NaN, 0) = 0
        return torch.round(c * _f32(levels)).clamp(-127, 127).to(torch.int8)
    a = x.abs()
    mag = cr_codes(x, qt, d, qm, t).abs()                     # rne(p(a) / d), correctly rounded log / exp
    mag = torch.where(a >= _f32(qm), torch.full_like(a, saturation_code(qt, d, qm, t)), mag)
    mag = torch.where(a > 0, mag, torch.zeros_like(a))        # 0 and NaN
    return torch.copysign(mag.clamp(max=127.0), x).to(torch.int8)


def _near_midpoint(v64: torch.Tensor) -> torch.Tensor:
    """v64 within 2^-20 fp32 ulp of the midpoint between two adjacent fp32 values."""
    f = v64.float()
    up = v64 >= f.double()
    nb = torch.where(up, torch.nextafter(f, torch.full_like(f, math.inf)),
                     torch.nextafter(f, torch.full_like(f, -math.inf))).double()
    ulp = (nb - f.double()).abs()
    near = ((v64 - f.double()).abs() - 0.5 * ulp).abs() <= 2.0 ** -20 * ulp
    return near & torch.isfinite(v64) & torch.isfinite(ulp)


def double_rounding_mask(x: torch.Tensor, qt: str, d: float, qm: float, t: float = 1.0, levels: int = 0) -> torch.Tensor:
    """Elements whose fp64 log or exp is too close to an fp32 rounding midpoint for two fp64 libraries to be sure
    to round alike (module docstring). Only elements on the nonlinear quantizer's log / exp path."""
    if qt != O.NONLINEAR:
        return torch.zeros(x.shape, dtype=torch.bool)
    a = x.float().abs()
    in_range = (a > 0) & (a < _f32(qm))
    a = torch.where(in_range, a, torch.ones_like(a))
    l64 = torch.log(a.double())
    e64 = torch.exp((_f32(t) * l64.float()).double())
    return in_range & (_near_midpoint(l64) | _near_midpoint(e64))


def num_boundaries(qt: str, d: float, qm: float, t: float = 1.0, levels: int = 0) -> int:
    return int(levels) if qt == ULTRA_ACT else int(min(saturation_code(qt, d, qm, t), 127))


def boundary_preimages(qt: str, d: float, qm: float, t: float = 1.0, levels: int = 0) -> torch.Tensor:
    """fp32 roundings of the values whose quotient is k + 1/2, k = 0 .. L - 1: ((k + 1/2) d)^(1/t), evaluated in fp64."""
    k = torch.arange(num_boundaries(qt, d, qm, t, levels), dtype=torch.float64) + 0.5
    if qt == ULTRA_ACT:
        return (k / levels).float()
    p = k * float(_f32(d))
    if qt == O.NONLINEAR:
        p = p ** (1.0 / float(_f32(t)))
    return p.float()


def _neighbours(c: torch.Tensor, ulps: int) -> torch.Tensor:
    """[len(c)][2 ulps + 1]: the fp32 values within +-ulps ulp of each (positive) c, ascending."""
    up, dn = [c], []
    hi, lo = c, c
    pinf, ninf = torch.full_like(c, math.inf), torch.full_like(c, -math.inf)
    for _ in range(ulps):
        hi, lo = torch.nextafter(hi, pinf), torch.nextafter(lo, ninf)
        up.append(hi)
        dn.append(lo)
    return torch.stack(dn[::-1] + up, dim=1)


TINY_SWITCH = 1e-30                # quant_fast: the hardware log2 flushes denormals, so a <= 1e-30 goes the careful way
DENORM_MIN, DENORM_MAX = 2.0 ** -149, 2.0 ** -126 - 2.0 ** -149


def special_inputs(qm: float) -> torch.Tensor:
    pos = torch.cat([torch.tensor([0.0, DENORM_MIN, DENORM_MAX], dtype=torch.float32),
                     _neighbours(_f32(TINY_SWITCH), 4).reshape(-1), _neighbours(_f32(qm).abs(), 4).reshape(-1),
                     torch.tensor([math.inf], dtype=torch.float32)])
    return torch.cat([pos, -pos, torch.tensor([math.nan], dtype=torch.float32)])


def boundary_inputs(qt: str, d: float, qm: float, t: float = 1.0, levels: int = 0, ulps: int = 64) -> torch.Tensor:
    """Every fp32 value within +-ulps ulp of a code boundary's preimage, both signs, and the specials (+-0, the
    smallest and largest denormal, +-4 ulp around the tiny switch and around |q_m|, +-inf, NaN). 1-D, fp32."""
    nb = _neighbours(boundary_preimages(qt, d, qm, t, levels), ulps).reshape(-1)
    return torch.cat([nb, -nb, special_inputs(qm if qt != ULTRA_ACT else 1.0)])


class PSet:
    def __init__(self, name, qt, d, qm, t=1.0, levels=0):
        self.name, self.qt, self.d, self.qm, self.t, self.levels = name, qt, float(d), float(qm), float(t), int(levels)

    @property
    def args(self):
        return self.qt, self.d, self.qm, self.t, self.levels

    def __repr__(self):
        return self.name


def _nl(qm, t):
    return PSet(f"nonlinear-qm{qm:g}-t{t:g}", O.NONLINEAR, qm ** t / 127, qm, t)


# q_m^t / d = 126.45 but (q_m + 1e-6)^t / d = 126.65: the saturation code (127, from q_m + 1e-6 as the reference forms
# it) is not the code of the value q_m itself (126), so |x| == q_m tells `>=` from `>` in the saturation mask. In the
# other sets the two agree and that comparison cannot be observed. The boundary 126.5 lies past q_m (all saturated).
SAT_OFFSET = PSet("nonlinear-qm0.001-t1.25-sat-offset", O.NONLINEAR, 1e-3 ** 1.25 / 126.45, 1e-3, 1.25)
POW2 = PSet("linear-d2^-6", O.LINEAR, 2.0 ** -6, 127 * 2.0 ** -6)      # every (k + 1/2) d is an fp32 (and fp16) value
PARAM_SETS = ([PSet("linear-d1/127", O.LINEAR, 1 / 127, 1.0), PSet("linear-d0.01", O.LINEAR, 0.01, 1.0), POW2,
               PSet("linear-negative-qm", O.LINEAR, 0.05, -0.5)] +
              [_nl(qm, t) for t in (1.0, 0.7, 0.85, 1.25) for qm in (0.6, 1.5)] +
              [_nl(1e4, 1.25), _nl(1e-3, 1.25), SAT_OFFSET] +           # |t ln a| up to 11.5 and 8.6 (+ boundary 0: 20)
              [PSet(f"ultra-levels{n}", ULTRA_ACT, 1.0, 0.0, 1.0, n) for n in (1, 15, 127)])
VIT_SETS = [p for p in PARAM_SETS if p.qt != ULTRA_ACT]
PSET = {p.name: p for p in PARAM_SETS}


def gelu_boundary_inputs(ps: PSet, ulps: int = 8, scan: int = 64) -> torch.Tensor:
    """The fp32 h > 0 whose O.gelu(h) lies within `ulps` ulp of a boundary preimage of `ps`: the +-scan nextafter
    neighbours of the fp64 solution of gelu(h) = preimage, filtered (GELU's slope on h > 0 is 0.5 .. 1.13 and an ulp
    of h is at most 4 ulp of gelu(h), so +-64 neighbours of h cover +-16 ulp of the value and more)."""
    c = boundary_preimages(*ps.args)
    gelu64 = lambda h: 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
    lo, hi = torch.zeros(len(c), dtype=torch.float64), torch.full((len(c),), 1.0, dtype=torch.float64)
    while bool((gelu64(hi) < c.double()).any()):
        hi = hi * 2
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        below = gelu64(mid) < c.double()
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    h = _neighbours(hi.float(), scan)
    g = O.gelu(h.reshape(-1)).reshape(h.shape)
    near = (g >= _neighbours(c, ulps)[:, :1]) & (g <= _neighbours(c, ulps)[:, -1:])
    return h[near]


def tile_columns(vals: torch.Tensor, rows: int, cols: int, offset: int = 0) -> torch.Tensor:
    """[rows][cols] whose element (r, c) is vals[(offset + r * cols + c) % len(vals)]: with rows * cols >= len(vals)
    every value occurs, in every column residue that the shapes' greatest common divisor allows."""
    idx = (offset + torch.arange(rows * cols)) % vals.numel()
    return vals[idx].reshape(rows, cols)


def bracket_ties(v64: torch.Tensor, delta, f):
    """(f(v64), possible_tie): possible_tie marks the elements whose code is not the same at v64 - delta, v64 and
    v64 + delta. f maps an fp64 tensor to codes (it rounds to fp32 itself); it is monotone up to GELU's dip on
    v < 0, which is why the middle value is compared too."""
    v64 = v64.double()
    ref, lo, hi = f(v64), f(v64 - delta), f(v64 + delta)
    return ref, (lo != hi) | (lo != ref) | (hi != ref)


def codes_fn(ps: PSet, gelu: bool = False):
    if gelu:
        return lambda v: device_codes(O.gelu(v.float()).reshape(v.shape), *ps.args)
    return lambda v: device_codes(v.float(), *ps.args)


# ---- the random-data cases of the kernel-level tests (inputs as those tests generate them) and their references -----
class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _qset(qt: str, d: float, qm: float, t: float) -> PSet:
    return PSet("case", qt, d, qm, t if qt == O.NONLINEAR else 1.0)


def gemm_epilogue_ties(a, w, bias, d_a: float, d_w: float, gelu: bool, ps: PSet):
    """Codes of quantize([gelu](alpha acc + bias)) from the fp64 value and its possible ties."""
    acc = O.int_accumulators(a.float(), w.float()).double()
    alpha = float(_f32(d_a) * _f32(d_w))
    v64 = alpha * acc + bias.double()
    delta = 4 * EPS32 * ((alpha * acc).abs() + bias.double().abs())
    return bracket_ties(v64, delta, codes_fn(ps, gelu))


GEMM_CODE_CASES = [(gelu, qt, t) for gelu in (False, True) for qt, t in ((O.LINEAR, 1.0), (O.NONLINEAR, 1.0),
                                                                         (O.NONLINEAR, 0.85))]


def gemm_code_case(gelu: bool, qt: str, t: float) -> Case:
    """test_gpu_kernels.py::test_gemm_int8_code_epilogue."""
    M, N, K = 300, 640, 768
    g = torch.Generator().manual_seed(11)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    bias = torch.randn(N, generator=g) * 0.1
    ps = _qset(qt, 0.9 / 127, 0.9, t)
    ref, tie = gemm_epilogue_ties(a, w, bias, 0.002, 0.0011, gelu, ps)
    return Case(a=a, w=w, bias=bias, ref=ref, tie=tie, cap=CAP_GEMM)


EPI_GEMM_CASES = [(gelu, qt, t) for gelu in (False, True) for qt, t in ((O.LINEAR, 1.0), (O.NONLINEAR, 1.0),
                                                                        (O.NONLINEAR, 0.8), (O.NONLINEAR, 1.25))]


def epi_gemm_case(gelu: bool, qt: str, t: float, M=4096, N=768, K=256, seed=5, dn=1.4 / 127, qmn=1.4) -> Case:
    """test_gpu_kernels.py::_epi_gemm's direct run (test_epilogue_code_table_equals_direct)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    bias = torch.randn(N, generator=g) * 0.5
    if qt == O.NONLINEAR:
        dn = qmn ** t / 127
    ref, tie = gemm_epilogue_ties(a, w, bias, 0.004, 0.0011, gelu, _qset(qt, dn, qmn, t))
    return Case(a=a, w=w, bias=bias, ref=ref, tie=tie, cap=CAP_GEMM)


def ln_row_error(x: torch.Tensor, gamma, beta, eps: float = 1e-6):
    """(y64, e32 [rows][1]): F.layer_norm in fp64 and the largest fp32-against-fp64 difference per row on the CPU,
    floored at eps32 max |y64| of the row."""
    cols = x.shape[1]
    y64 = F.layer_norm(x.double(), (cols,), None if gamma is None else gamma.double(),
                       None if beta is None else beta.double(), eps)
    y32 = F.layer_norm(x.float(), (cols,), gamma, beta, eps)
    e32 = (y32.double() - y64).abs().amax(dim=1, keepdim=True)
    return y64, torch.maximum(e32, EPS32 * y64.abs().amax(dim=1, keepdim=True))


def ln_ties(x, gamma, beta, ps: PSet, c_ln: float = C_LN):
    y64, e32 = ln_row_error(x, gamma, beta)
    return bracket_ties(y64, c_ln * e32, codes_fn(ps))


def ln_needed_c(x, gamma, beta, ps: PSet, got: torch.Tensor) -> float:
    """The smallest C for which every differing code of `got` is a possible tie: for each flip, the distance of y64
    from the nearest value whose code is got's, in units of the row's e32 (found by bisection on C)."""
    y64, e32 = ln_row_error(x, gamma, beta)
    f = codes_fn(ps)
    flip = f(y64) != got
    if not bool(flip.any()):
        return 0.0
    yv, ev, gv = y64[flip], e32.expand_as(y64)[flip], got[flip]
    lo, hi = torch.zeros_like(yv), torch.full_like(yv, 2.0 ** 20)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        hit = (f(yv - mid * ev) <= gv) & (gv <= f(yv + mid * ev))       # f is monotone
        lo, hi = torch.where(hit, lo, mid), torch.where(hit, mid, hi)
    return float(hi.max())


LN_ROWS = [1, 5, 333]
LN_COLS = [1, 192, 384, 768, 770, 1000, 1280, 2048, 2052]      # the widths of test_gpu_kernels.LN_ARMS
LN_D, LN_QM = 4.0 / 127, 4.0


def ln_case_inputs(cols: int, affine: bool):
    """test_gpu_kernels.py::test_layernorm_quant_vs_oracle: (gamma, beta, [x per row count])."""
    g = torch.Generator().manual_seed(8 + cols)
    gamma = (torch.rand(cols, generator=g) + 0.5) if affine else None
    beta = (torch.randn(cols, generator=g) * 0.1) if affine else None
    return gamma, beta, [torch.randn(rows, cols, generator=g) * 2 + 0.3 for rows in LN_ROWS]


def ref_attention(qkv: torch.Tensor, B: int, N: int, H: int, hd: int, scale: float) -> torch.Tensor:
    """softmax(q k^T scale) v in fp64 from [B N][3 H hd] (as test_gpu_attention.ref_attention)."""
    x = qkv[:, :3 * H * hd].double().reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    a = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    return (a @ v).transpose(1, 2).reshape(B * N, H * hd)


def attention_ties(out64: torch.Tensor, ps: PSet):
    return bracket_ties(out64, ATTN_REL_DELTA * float(out64.abs().max()), codes_fn(ps))


ATTN_CODE_CASES = [(O.LINEAR, 1.0), (O.NONLINEAR, 1.0), (O.NONLINEAR, 0.8)]


def attention_code_case(qt: str, t: float) -> Case:
    """test_gpu_attention.py::test_attention_int8_codes_vs_oracle."""
    B, N, H = 2, 197, 12
    qkv = torch.randn(B * N, 3 * H * 64, generator=torch.Generator().manual_seed(11))
    qm = 1.2
    ps = _qset(qt, qm ** t / 127 if qt == O.NONLINEAR else qm / 127, qm, t)
    ref, tie = attention_ties(ref_attention(qkv, B, N, H, 64, 0.125), ps)
    return Case(qkv=qkv, ref=ref, tie=tie, cap=CAP_ATTN)


def attention_split_case() -> Case:
    """test_gpu_attention.py::test_attention_split_int8_and_in_scale."""
    B, N, H = 2, 197, 12
    qkv = torch.randn(B * N, 3 * H * 64, generator=torch.Generator().manual_seed(13))
    qkv[:, 2 * H * 64:] *= 3.0e4
    ref, tie = attention_ties(ref_attention(qkv, B, N, H, 64, 0.125), _qset(O.NONLINEAR, 4e4 ** 0.9 / 127, 4e4, 0.9))
    return Case(qkv=qkv, ref=ref, tie=tie, cap=CAP_ATTN)


FUSED_CODE_CASES = [(4, 197, 12, 7 + 197), (3, 64, 6, 7 + 64), (2, 208, 4, 7 + 208), (3, 17, 5, 7 + 17)]
FUSED_STORE_CASES = [(3, 197, 4, 11), (3, 197, 4, 15)]      # seeds 11 + pad, pad in {0, 4}


def fused_attention_case(B: int, N: int, H: int, seed: int, K: int = 768) -> Case:
    """test_gpu_attention.py::_fused_case's data (test_qkv_attention_fused_int8_codes, _store_paths): fp64 attention
    of the fp64-evaluated projection alpha acc + bias."""
    g = torch.Generator().manual_seed(seed)
    C = 64 * H
    a = torch.randint(-60, 61, (B * N, K), generator=g)
    w = torch.randint(-7, 8, (3 * C, K), generator=g)
    bias = torch.randn(3 * C, generator=g) * 0.3
    alpha = float(_f32(0.004) * _f32(0.003))
    qkv64 = alpha * O.int_accumulators(a.float(), w.float()).double() + bias.double()
    qm, t = 0.5, 0.9
    ref, tie = attention_ties(ref_attention(qkv64, B, N, H, 64, 0.125), _qset(O.NONLINEAR, qm ** t / 127, qm, t))
    return Case(a=a, w=w, bias=bias, ref=ref, tie=tie, cap=CAP_ATTN)


def identical_rows_case(B: int = 3, N: int = 33, H: int = 2) -> Case:
    """test_gpu_quant_boundaries.py::test_attention_identical_value_rows: random q and k, one v row per image
    repeated over the N keys, so out = v in exact arithmetic. v spans +-1.05 q_m of the power-of-two set. One possible
    tie among the 384 distinct values recurs in all 33 rows and alone exceeds the cap (1 / 384), so the seed is one
    whose values have none (seeds 33 and 35 have one; test_vit_codes_ref_cpu.py holds the condition)."""
    C = 64 * H
    g = torch.Generator().manual_seed(34)
    qkv = torch.randn(B, N, 3 * C, generator=g)
    v = (torch.rand(B, 1, C, generator=g) * 2 - 1) * POW2.qm * 1.05
    qkv[:, :, 2 * C:] = v
    ref, tie = attention_ties(v.expand(B, N, C).reshape(B * N, C).double(), POW2)
    return Case(qkv=qkv.reshape(B * N, 3 * C), ref=ref, tie=tie, cap=CAP_ATTN)
