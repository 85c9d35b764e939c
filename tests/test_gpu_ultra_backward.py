"""UltraNet's training kernels through the C ABI (ultra_backward.hip) against tests/ultra_backward_ref.py:
qvit_ultra_weight_quant_backward, qvit_ultra_act_quant_backward, qvit_conv_wgrad, and the input gradient as
qvit_conv_wonly on the transposed, flipped codes. Accuracy of the two contractions:
err = max|g - g64| / max|g64| against the float64 restatement, bound c * max(err of the float32 CPU restatement,
eps), c the next power of two at or above twice the worst ratio measured on an MI355X over these shapes
(DESIGN.md section 17 holds the table)."""
import pytest
import torch

import ultra_backward_ref as R
from quantized_vit_amd import _lib
from quantized_vit_amd.quant_ultra import conv2d_Q_fn

pytestmark = pytest.mark.gpu

EPS = float(torch.finfo(torch.float32).eps)
C_WGRAD, C_DGRAD = R.C_WGRAD, R.C_DGRAD

# (B, C, H, W, N, k, stride, pad, dilation, levels)
WGRAD_SHAPES = [(1, 1, 1, 1, 1, 1, 1, 0, 1, 1), (2, 3, 5, 7, 5, 3, 1, 1, 1, 15), (1, 16, 9, 9, 32, 3, 1, 1, 1, 15),
                (2, 64, 6, 6, 64, 3, 1, 1, 1, 15), (3, 64, 4, 4, 36, 1, 1, 0, 1, 15),
                (2, 16, 40, 40, 16, 3, 1, 1, 1, 15), (1, 4, 11, 13, 8, 3, 2, 1, 1, 7),
                (1, 4, 11, 13, 8, 3, 1, 2, 2, 127)]


def _args(shape):
    k, s, p, d = shape[5:9]
    return (k, k), (s, s), (p, p), (d, d)


def _out_hw(shape):
    _, _, H, W, _, k, s, p, d, _ = shape
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


def _operands(shape, seed=0):
    B, C, H, W, N = shape[:5]
    levels = shape[9]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(0, levels + 1, (B, C, H, W), generator=gen).float() / levels   # k / levels as fp32
    G = torch.randn(B, N, *_out_hw(shape), generator=gen)
    return G, x


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


_WGRAD_REF = {}


def _wgrad_ref(shape):
    """(G, x, float64 restatement, err of the float32 restatement): computed once per shape, never modified."""
    if shape not in _WGRAD_REF:
        G, x = _operands(shape)
        ref = R.conv_wgrad(G, x, *_args(shape))
        _WGRAD_REF[shape] = (G, x, ref, _rel(R.conv_wgrad(G, x, *_args(shape), dtype=torch.float32), ref))
    return _WGRAD_REF[shape]


def _wgrad(dev, G, x, shape, **kw):
    return _lib.conv_wgrad(G.to(dev), x.to(dev), *_args(shape), shape[9], **kw)


def wgrad_ratio(dev, shape):
    G, x, ref, err32 = _wgrad_ref(shape)
    err = _rel(_wgrad(dev, G, x, shape).cpu(), ref)
    return err, err32, err / max(err32, EPS)


def dgrad_ratio(dev, shape):
    """Input gradient of a 4-bit Conv2d_Q at `shape` through autograd (qvit_conv_wonly on the flipped image)."""
    B, C, H, W, N, k, s, p, d, _ = shape
    G, x = _operands(shape, seed=1)
    torch.manual_seed(2)
    conv = conv2d_Q_fn(4)(C, N, k, s, p, d, bias=False).to(dev)
    xg = x.to(dev).requires_grad_(True)
    (conv(xg) * G.to(dev)).sum().backward()
    with torch.no_grad():
        wq = conv.quantize_fn(conv.weight).cpu()
    ref = R.conv_dgrad(G, wq, (H, W), *_args(shape)[1:])
    err32 = _rel(R.conv_dgrad(G, wq, (H, W), *_args(shape)[1:], dtype=torch.float32), ref)
    err = _rel(xg.grad.cpu(), ref)
    return err, err32, err / max(err32, EPS)


# ---- qvit_ultra_weight_quant_backward ------------------------------------------------------------------------
def _weights(n, case, seed=0):
    gen = torch.Generator().manual_seed(seed)
    if case == "equal":
        w = torch.full((n,), 0.7)
        w[1::2] = -0.7
        return w
    w = torch.rand(n, generator=gen) * 4 - 2          # |tanh| <= tanh(2) < tanh(2.5)
    w[n // 2] = 2.5                                    # the unique maximum
    if case == "tie" and n > 1:
        w[0] = -2.5                                    # a second element attains it, with the other sign
    return w


@pytest.mark.parametrize("w_bit", [2, 4, 8])
@pytest.mark.parametrize("case", ["unique", "tie", "equal"])
@pytest.mark.parametrize("n", [1, 3, 255, 1025, 64 * 576])
def test_weight_quant_backward(dev, n, case, w_bit):
    w = _weights(n, case)
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen)
    for scale in (1.0, 2.0 ** -30, 2.0 ** 20):
        gs = g * scale
        got = _lib.ultra_weight_quant_backward(w.to(dev), gs.to(dev), w_bit).cpu().double()
        ref = R.weight_quant_backward(w, gs)
        bound = R.weight_quant_bound(w, gs)
        err = (got - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"wq backward n {n} {case} w_bit {w_bit} scale {scale:g}: worst err / bound {worst:.4f}")
        assert bool((err <= bound).all()), (scale, worst)


def test_weight_quant_backward_nan_and_determinism(dev):
    n = 1025
    w = _weights(n, "tie")
    gen = torch.Generator().manual_seed(9)
    g = torch.randn(n, generator=gen)
    a = _lib.ultra_weight_quant_backward(w.to(dev), g.to(dev), 4)
    b = _lib.ultra_weight_quant_backward(w.to(dev), g.to(dev), 4)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    gn = g.clone()
    gn[7] = float("nan")
    got = _lib.ultra_weight_quant_backward(w.to(dev), gn.to(dev), 4).cpu()
    nan = torch.isnan(got)
    # at that element, and through the sum at every element of the tie set (masks select: nowhere else, as torch)
    assert nan.nonzero().flatten().tolist() == [0, 7, n // 2]
    assert torch.equal(nan, torch.isnan(R.weight_quant_backward(w, gn)))
    keep = ~nan
    assert torch.equal(got[keep], a.cpu()[keep])
    # every element tied: the NaN is everywhere
    we = _weights(n, "equal")
    assert bool(torch.isnan(_lib.ultra_weight_quant_backward(we.to(dev), gn.to(dev), 4)).all())
    # a NaN weight reaches its own element; in place (grad_w is grad_out)
    wn = w.clone()
    wn[11] = float("nan")
    assert bool(torch.isnan(_lib.ultra_weight_quant_backward(wn.to(dev), g.to(dev), 4)[11]))
    gd = g.to(dev)
    assert torch.equal(_lib.ultra_weight_quant_backward(w.to(dev), gd, 4, grad_w=gd), a)


# ---- qvit_ultra_act_quant_backward ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_act_quant_backward(dev, n):
    edge = torch.tensor([0.0, 1.0, -0.1, 1.1, float("nan")])
    gen = torch.Generator().manual_seed(n)
    x = torch.rand(n, generator=gen) * 1.4 - 0.2
    x[:min(n, 5)] = edge[:min(n, 5)]
    if n > 5:
        x[-5:] = edge                                  # the scalar tail sees them too
    g = torch.randn(n, generator=gen)
    want = R.act_quant_backward(x, g)
    got = _lib.ultra_act_quant_backward(x.to(dev), g.to(dev))
    assert torch.equal(got.cpu(), want)
    gd = g.to(dev)
    out = _lib.ultra_act_quant_backward(x.to(dev), gd, grad_x=gd)   # in place
    assert out.data_ptr() == gd.data_ptr() and torch.equal(gd.cpu(), want)


# ---- qvit_conv_wgrad -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_conv_wgrad_accuracy(dev, shape):
    err, err32, ratio = wgrad_ratio(dev, shape)
    print(f"conv wgrad {shape}: err {err:.3e}, fp32 CPU err {err32:.3e}, ratio {ratio:.3f}")
    assert err <= C_WGRAD * max(err32, EPS), (err, err32, ratio)


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_conv_wgrad_properties(dev, shape):
    B, C, H, W, N, k = shape[:6]
    G, x, ref, _ = _wgrad_ref(shape)
    a = _wgrad(dev, G, x, shape)
    assert a.shape == (N, C, k, k)
    # two calls, a dirty workspace: the same bits
    nbytes = int(_lib.load().qvit_conv_wgrad_workspace_bytes(B, C, H, W, N, k, k, *[v for p in _args(shape)[1:] for v in p]))
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    assert torch.equal(_wgrad(dev, G, x, shape, workspace=ws), a)
    # G = 0: exact zeros
    assert bool((_wgrad(dev, torch.zeros_like(G), x, shape) == 0).all())
    # integer G: every partial sum is an integer below 2^24, the result is the float64 one rounded once
    Gi = torch.randint(-8, 9, G.shape, generator=torch.Generator().manual_seed(5)).float()
    want = (R.conv_wgrad(Gi, x * shape[9], *_args(shape)) * float(torch.tensor(1.0 / shape[9]))).float()
    assert torch.equal(_wgrad(dev, Gi, x, shape).cpu(), want)
    # a NaN at one G[b][n] poisons output channel n only
    Gn = G.clone()
    n0 = N // 2
    Gn[B - 1, n0, -1, -1] = float("nan")
    got = _wgrad(dev, Gn, x, shape)
    keep = torch.arange(N, device=dev) != n0
    assert bool(torch.isnan(got[n0]).all()) and torch.equal(got[keep], a[keep])
    # a guard band around dW is untouched
    band = 64
    buf = torch.full((band + a.numel() + band,), -7.5, dtype=torch.float32, device=dev)
    out = buf[band:band + a.numel()].view(N, C, k, k)
    _wgrad(dev, G, x, shape, out=out)
    assert torch.equal(out, a) and bool((buf[:band] == -7.5).all()) and bool((buf[-band:] == -7.5).all())


def test_conv_wgrad_crosses_the_split_boundaries(dev):
    def splits(shape):   # from the workspace query: s partial sets of the padded output
        B, C, H, W, N, k, s, p, d, _ = shape
        r = lambda v: (v + 63) // 64 * 64
        nbytes = int(_lib.load().qvit_conv_wgrad_workspace_bytes(B, C, H, W, N, k, k, s, s, p, p, d, d))
        return nbytes // (r(N) * r(C * k * k) * 4)
    assert splits((2, 16, 40, 40, 16, 3, 1, 1, 1, 15)) == 100     # 3200 rows: one 32-row stage per split
    assert splits((1, 1, 1, 1, 1, 1, 1, 0, 1, 1)) == 1


@pytest.mark.parametrize("shape", [s for s in WGRAD_SHAPES if s[6] == 1])
def test_conv_dgrad_accuracy(dev, shape):
    err, err32, ratio = dgrad_ratio(dev, shape)
    print(f"conv dgrad {shape}: err {err:.3e}, fp32 CPU err {err32:.3e}, ratio {ratio:.3f}")
    assert err <= C_DGRAD * max(err32, EPS), (err, err32, ratio)
