"""NaN, Inf, zero and tiny inputs of the forward quantizer paths: the planted values, the expected codes and fake-quant
values, and the two checkers (containment, path equality) of tests/test_gpu_special_values.py. Nothing here imports
the package; tests/test_special_values_ref_cpu.py pins the tables as literals and holds the negative controls.

Expected codes are oracle.quant_oracle.quant_codes with one stated mapping, NaN -> 0, saturated to int8 (+-127): the
contract of include/qvit_hip.h ("special values"). Expected fake-quant values are O.fake_quant unchanged (a NaN stays a
NaN). ULTRA_ACT has no entry in quant_oracle: its codes are rne(clamp(x, 0, 1) levels), quant_ultra.py:18-19,71, with
the same NaN -> 0.
"""
from __future__ import annotations

import math

import torch

import vit_codes_ref as V
from oracle import quant_oracle as O

FLT_MAX = 3.4028234663852886e38
FLT_MIN = 1.1754943508222875e-38
DENORMAL = 1e-40


def _bits(u: int) -> torch.Tensor:
    return torch.tensor([u - (1 << 32) if u >= (1 << 31) else u], dtype=torch.int32).view(torch.float32)


def _next(v: float, to: float) -> float:
    return float(torch.nextafter(V._f32(v), V._f32(to)))


def special_names(qm: float):
    """(name, fp32 value) of every planted input for a quantizer whose saturation threshold is qm."""
    aq = float(V._f32(abs(qm)))
    return [("+nan", float("nan")), ("-nan", None), ("+inf", math.inf), ("-inf", -math.inf), ("+0", 0.0), ("-0", -0.0),
            ("+flt_max", FLT_MAX), ("-flt_max", -FLT_MAX), ("+flt_min", FLT_MIN), ("-flt_min", -FLT_MIN),
            ("+denormal", DENORMAL), ("-denormal", -DENORMAL), ("1e-31", 1e-31), ("1e-38", 1e-38),
            ("+qm", aq), ("-qm", -aq), ("below-qm", _next(aq, 0.0)), ("above-qm", _next(aq, math.inf))]


def special_inputs(qm: float) -> torch.Tensor:
    """The planted list as fp32 [18]; the two quiet NaNs are 0x7fc00000 and 0xffc00000."""
    vals = [_bits(0xFFC00000) if n == "-nan" else (_bits(0x7FC00000) if n == "+nan" else V._f32(v))
            for n, v in special_names(qm)]
    return torch.cat(vals)


# The quantizers of the special-value tests. "linear-L7" is a 4-bit activation quantizer: the bucket width of its code
# table (0.8 d) is wider than the margin below -q_m, which is what put a change point into bucket 0 of the table.
SETS = [V.PSet("linear-L127", O.LINEAR, 1.0 / 127, 1.0), V.PSet("linear-L7", O.LINEAR, 0.5 / 7, 0.5),
        V.PSet("nonlinear-t1", O.NONLINEAR, 1.5 / 127, 1.5, 1.0),
        V.PSet("nonlinear-t0.8", O.NONLINEAR, 1.5 ** 0.8 / 127, 1.5, 0.8),
        V.PSet("linear-negative-qm", O.LINEAR, 0.05, -0.5),
        V.PSet("ultra-levels15", V.ULTRA_ACT, 1.0, 0.0, 1.0, 15)]
# The tiny arm (quant_fast: |x| <= 1e-30 takes the careful path on the nonlinear quantizer): steps small enough for
# such values to get a non-zero code. t = 0.5: (1e-38)^0.5 = 1e-19, code 10; the denormal 1e-40 has code 1, 1e-31
# saturates at 127. t = 1.25: (1e-31)^1.25 = 1.78e-39, code 18 at d = 1e-40; (1e-38)^1.25 = 3e-48 and the denormal's
# power are below the smallest fp32 denormal, so their code is 0 at every fp32 step (nothing to choose there).
TINY_SETS = [V.PSet("tiny-t0.5", O.NONLINEAR, 1e-20, 1.5, 0.5), V.PSet("tiny-t1.25", O.NONLINEAR, 1e-40, 1.5, 1.25)]
TINY_INPUTS = torch.tensor([1e-31, 1e-38, DENORMAL, FLT_MIN, 3e-35, -1e-31, -1e-38, -DENORMAL, -FLT_MIN, -3e-35],
                           dtype=torch.float32)
PSET = {p.name: p for p in SETS + TINY_SETS}


def expected_codes(x: torch.Tensor, ps: V.PSet) -> torch.Tensor:
    """int8 codes of fp32 x: O.quant_codes, NaN -> 0, saturated at +-127."""
    x = x.float()
    if ps.qt == V.ULTRA_ACT:
        k = torch.round(x.clamp(0.0, 1.0) * float(ps.levels))
    else:
        k = O.quant_codes(x, ps.qt, ps.d, ps.qm, ps.t)
    k = torch.where(torch.isnan(k), torch.zeros_like(k), k)
    return k.clamp(-127.0, 127.0).to(torch.int8)


def expected_fake_quant(x: torch.Tensor, ps: V.PSet) -> torch.Tensor:
    """O.fake_quant unchanged: NaN in, NaN out."""
    return O.fake_quant(x.float(), ps.qt, ps.d, ps.qm, ps.t)


def expected_gelu_codes(h: torch.Tensor, ps: V.PSet) -> torch.Tensor:
    """O.gelu, then the oracle quantizer: gelu(-inf) = -inf * 0 is NaN (code 0), gelu(+inf) = +inf (saturated)."""
    return expected_codes(O.gelu(h.float()).reshape(h.shape), ps)


def same_values(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal semantics plus equal NaN positions: +0 == -0, a NaN equals a NaN of any sign or payload."""
    a, b = a.cpu(), b.cpu()
    if a.shape != b.shape:
        return False
    if not a.is_floating_point():
        return bool(torch.equal(a, b))
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na], b[~nb]))


def same_bits(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Elementwise bit identity (fp32 compared as int32: the sign of zero and a NaN's payload count)."""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.is_floating_point():
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a == b


def assert_planted(got: torch.Tensor, want: torch.Tensor, what: str = "") -> None:
    """(a): the outputs at the planted positions equal the expected table."""
    got, want = got.cpu(), want.cpu()
    if not same_values(got, want):
        raise AssertionError(f"{what}: planted outputs {got.reshape(-1).tolist()} != expected {want.reshape(-1).tolist()}")


def assert_paths_equal(outs: dict, what: str = "") -> None:
    """(b): every path of an entry point returned the same bytes. outs: {path name: tensor}."""
    names = list(outs)
    assert len(names) >= 2, "path equality needs two paths"
    first = outs[names[0]]
    for n in names[1:]:
        same = same_bits(first, outs[n]) if first.shape == outs[n].shape else None
        if same is None or not bool(same.all()):
            where = [] if same is None else (~same).nonzero()[:4].tolist()
            raise AssertionError(f"{what}: path {n!r} differs from {names[0]!r} at {where}")


def assert_contained(clean: torch.Tensor, poisoned: torch.Tensor, allowed: torch.Tensor, what: str = "") -> None:
    """(c): outside the boolean mask `allowed` (the outputs that depend on a planted input) the poisoned run is bit
    identical to the clean one. Inside it anything goes: what is expected there is assert_planted's business."""
    assert clean.shape == poisoned.shape == allowed.shape, (clean.shape, poisoned.shape, allowed.shape)
    leak = ~same_bits(clean, poisoned) & ~allowed.cpu()
    if bool(leak.any()):
        raise AssertionError(f"{what}: {int(leak.sum())} outputs outside the allowed set changed; first at "
                             f"{leak.nonzero()[0].tolist()}")


def rows_mask(shape, rows) -> torch.Tensor:
    m = torch.zeros(shape, dtype=torch.bool)
    m[list(rows)] = True
    return m


def cols_mask(shape, cols) -> torch.Tensor:
    m = torch.zeros(shape, dtype=torch.bool)
    m[:, list(cols)] = True
    return m


def im2col_taps(B: int, C: int, H: int, W: int, k: int, s: int, p: int, pixels) -> torch.Tensor:
    """Boolean [B OH OW][C k k]: the im2col entries that read one of `pixels` [(b, c, y, x)] (dilation 1)."""
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    m = torch.zeros((B * OH * OW, C * k * k), dtype=torch.bool)
    for (b, c, y, x) in pixels:
        for oh in range(OH):
            for ow in range(OW):
                ih, iw = y - (oh * s - p), x - (ow * s - p)
                if 0 <= ih < k and 0 <= iw < k:
                    m[(b * OH + oh) * OW + ow, (c * k + ih) * k + iw] = True
    return m


def attention_blocks_mask(B: int, N: int, H: int, hd: int, blocks) -> torch.Tensor:
    """Boolean [B N][H hd]: the outputs of the (image, head) pairs in `blocks`."""
    m = torch.zeros((B, N, H, hd), dtype=torch.bool)
    for (b, h) in blocks:
        m[b, :, h] = True
    return m.reshape(B * N, H * hd)
