"""qvit_quantize_act_i16 and qvit_gemm_a16 at the kernel level: the digit planes decode to the quantizer's codes, and
the GEMM is one fp32 rounding away from the fp64 value of the exact int64 contraction, on all four weight formats."""
import pytest
import torch

from quantized_vit_amd import _lib

pytestmark = pytest.mark.gpu

D_ACT, D_WT = 1.23e-3, 3.1e-5
# the codes a format holds (W16 / W24: what pack_weight_wide's balanced digits reach)
W_RANGE = {_lib.W4: (-8, 7), _lib.W8: (-128, 127), _lib.W16: (-32639, 32639), _lib.W24: (-(2 ** 23 - 1), 8355711)}


def _planes(ka: torch.Tensor, dev) -> torch.Tensor:
    """int64 codes [M, K] in [-32768, 32767] -> the digit planes int8 [2, M, K]."""
    return torch.stack([ka >> 8, (ka & 255) - 128]).to(torch.int8).to(dev).contiguous()


def _check_gemm(planes, image, wfmt, ka, kw, bias, dev):
    """Runs qvit_gemm_a16 and holds it to |y - y64| <= 2^-23 |y64| + 2^-50 (|d_a d_w S| + |bias|)."""
    (M, K), N = ka.shape, kw.shape[0]
    npad = _lib.round_up(N, _lib.TILE_N)
    d_act, d_wt = torch.tensor([D_ACT], device=dev), torch.tensor([D_WT], device=dev)
    wsum = _lib.weight_code_sums(image, wfmt, npad, K)
    scale = 16 if wfmt == _lib.W4 else 1   # the W4 image is contracted as the bytes 16 k
    assert torch.equal(wsum[:N].cpu(), scale * kw.sum(1)) and not bool(wsum[N:].any())
    y = torch.full((M, _lib.round_up(N, 4)), float("nan"), device=dev)
    _lib.gemm_a16(planes, M, K, image, wfmt, N, npad, d_act, d_wt, _lib.pad_bias(bias.to(dev), N, npad, dev), wsum, y)
    S = (ka @ kw.t()).double()   # int64 matmul on the CPU: exact
    prod = float(d_act.double() * d_wt.double()) * S
    y64 = prod + bias.double()
    err = (y[:, :N].double().cpu() - y64).abs()
    bound = 2.0 ** -23 * y64.abs() + 2.0 ** -50 * (prod.abs() + bias.double().abs())
    print(f"wfmt {wfmt} M {M} N {N} K {K}: worst err / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    assert bool(y[:, N:].isnan().all())   # columns past N are not written


@pytest.mark.parametrize("wfmt", [_lib.W4, _lib.W8, _lib.W16, _lib.W24])
@pytest.mark.parametrize("M, N, K", [(1, 48, 128), (70, 300, 384), (197, 256, 128)])
def test_gemm_against_int64(dev, wfmt, M, N, K):
    g = torch.Generator().manual_seed(1000 * wfmt + M)
    ka = torch.randint(-32768, 32768, (M, K), generator=g)
    ka[0, 0], ka[-1, -1] = -32768, 32767
    lo, hi = W_RANGE[wfmt]
    kw = torch.randint(lo, hi + 1, (N, K), generator=g)
    kw[0, 0], kw[-1, -1], kw[N // 2, 1] = lo, hi, lo
    bias = torch.randn(N, generator=g)
    npad = _lib.round_up(N, _lib.TILE_N)
    if wfmt in (_lib.W4, _lib.W8):
        image = _lib.pack_codes(kw.float().to(dev), wfmt, npad, K)
    else:
        image, fmt = _lib.pack_weight_wide(kw.float().to(dev), npad, K)
        assert fmt == wfmt
    _check_gemm(_planes(ka, dev), image, wfmt, ka, kw, bias, dev)


def test_gemm_largest_k_extreme_classes(dev):
    """Largest K, every digit -128 or 127: row 0 drives both middle classes to 2^30, row 1 alternates the sign."""
    K, N = _lib.A16_MAX_K, 256
    assert K >= 16384
    ka = torch.full((2, K), -32768, dtype=torch.int64)         # hi = lo = -128
    ka[1, 1::2] = 32767                                         # hi = lo = 127
    digit = torch.full((N, K), -128.0, device=dev)
    digit[1::2, 1::2] = 127.0                                   # odd weight rows alternate too: aligned with row 1
    image = torch.cat([_lib.pack_codes(digit, _lib.W8, N, K)] * 3)
    kw = (digit.cpu().long() * (65536 + 256 + 1))
    _check_gemm(_planes(ka, dev), image, _lib.W24, ka, kw, torch.linspace(-3.0, 3.0, N), dev)


@pytest.mark.parametrize("L", [255, 2047, 32767])
@pytest.mark.parametrize("cols", [100, 128])
def test_quantizer_linear_digits(dev, L, cols):
    """x = d (k + delta), |delta| <= 0.3: the planes decode to k clamped to +-L, exactly; NaN -> 0, +-Inf -> +-L."""
    g = torch.Generator().manual_seed(L + cols)
    rows, kpad, d = 37, 128, 0.0123
    k = torch.randint(-L, L + 1, (rows, cols), generator=g)
    edge = [0, 1, 127, 128, 255, 256, L, L + 1, L + 300, 2 * L]
    k[0, :2 * len(edge)] = torch.tensor([s * v for v in edge for s in (1, -1)])
    x = (d * (k.double() + 0.6 * torch.rand(rows, cols, generator=g, dtype=torch.float64) - 0.3)).float()
    x[1, :3] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    want = k.clamp(-L, L)
    want[1, :3] = torch.tensor([0, L, -L])
    planes = torch.empty((2, rows, kpad), dtype=torch.int8, device=dev)
    qd = torch.tensor([d], device=dev)
    _lib.quantize_act_i16(x.to(dev), _lib.QT_LINEAR, qd, qd * L, None, 0, planes, kpad)
    assert torch.equal(_lib.digits_to_codes(planes)[:, :cols].cpu().long(), want)
    assert bool((planes[0, :, cols:] == 0).all()) and bool((planes[1, :, cols:] == -128).all())   # padding: code 0


def test_quantizer_nonlinear_digits(dev):
    """The nonlinear quantizer: the same quant_code as qvit_fake_quant_f32, so the codes are round(value / d)."""
    g = torch.Generator().manual_seed(5)
    x = (2.0 * torch.randn(37, 100, generator=g)).to(dev)
    d, qm, t = (torch.tensor([v], device=dev) for v in (3.03 / 2000, 4.0, 0.8))
    planes = torch.empty((2, 37, 128), dtype=torch.int8, device=dev)
    _lib.quantize_act_i16(x, _lib.QT_NONLINEAR, d, qm, t, 0, planes, 128)
    want = (_lib.fake_quant_f32(x, _lib.QT_NONLINEAR, d, qm, t) / d).round().to(torch.int32)
    assert int(want.abs().max()) > 1500 and torch.equal(_lib.digits_to_codes(planes)[:, :100], want)
