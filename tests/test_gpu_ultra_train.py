"""UltraNet under autograd: Conv2d_Q, the quantizers and UltraNetQua.train() give the reference's straight-through
gradients (tests/ultra_backward_ref.py) with the forward bit-identical to the no_grad HIP forward. Without the
training backward weight.grad is None and only the head's bias receives a gradient."""
import pytest
import torch
import torch.nn as nn

import ultra_backward_ref as R
from quantized_vit_amd import quant_ultra as Q
from quantized_vit_amd.ultranet import UltraNetQua

pytestmark = pytest.mark.gpu

EPS = float(torch.finfo(torch.float32).eps)
TIE_BAND = 1e-4


def _rel(got, ref):
    return float((got.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


def conv_module_figures(dev, monkeypatch=None):
    """Conv2d_Q(4-bit) 16 -> 32, 3 x 3 on codes input, per route: (route, in_levels, err of weight.grad against
    the float64 restatement, err of the float32 CPU restatement, HIP weight-gradient calls so far)."""
    torch.manual_seed(0)
    conv = Q.conv2d_Q_fn(4)(16, 32, 3, 1, 1).to(dev)
    gen = torch.Generator().manual_seed(1)
    x = (torch.randint(0, 16, (2, 16, 9, 9), generator=gen).float() / 15).to(dev)
    G = torch.randn(2, 32, 9, 9, generator=gen)
    with torch.no_grad():
        y0 = conv(x)
        wq = conv.quantize_fn(conv.weight).cpu()
    calls = []
    real = Q._lib.conv_wgrad
    prev = Q.ULTRA_BWD
    Q._lib.conv_wgrad = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    out = []
    try:
        # qvit_conv_wgrad (selected by name: the default keeps wgrad on the library), the
        # default route, and the library route of a stand-alone call on unknown input
        for route, in_levels in (("wgrad", 15), ("hip", 15), ("wgrad", None)):
            Q.ULTRA_BWD = route
            conv.zero_grad()
            y = conv(x, _in_levels=in_levels)
            assert y.grad_fn is not None and torch.equal(y, y0)   # the no_grad forward, bit for bit
            (y * G.to(dev)).sum().backward()
            assert conv.weight.grad is not None and conv.bias.grad is not None
            # float64 restatement: the conv's weight gradient, then the weight quantizer's backward; the float32
            # one runs both steps in float32, so its error holds the quantizer backward's too
            w = conv.weight.detach().cpu().flatten()
            g_wq = R.conv_wgrad(G, x.cpu(), (3, 3), (1, 1), (1, 1), (1, 1))
            ref = R.weight_quant_backward(w, g_wq.flatten()).reshape(conv.weight.shape)
            g_wq32 = R.conv_wgrad(G, x.cpu(), (3, 3), (1, 1), (1, 1), (1, 1), dtype=torch.float32)
            ref32 = R.weight_quant_backward(w, g_wq32.flatten(), dtype=torch.float32).reshape(conv.weight.shape)
            out.append((route, in_levels, _rel(conv.weight.grad, ref), _rel(ref32, ref), len(calls),
                        _rel(conv.bias.grad, G.sum((0, 2, 3))), _rel(G.sum((0, 2, 3)), G.double().sum((0, 2, 3)))))
    finally:
        Q.ULTRA_BWD = prev
        Q._lib.conv_wgrad = real
    assert torch.equal(wq, conv.quantize_fn(conv.weight).detach().cpu())
    return out


def test_conv2d_q_weight_grad_and_bit_equal_forward(dev):
    for route, in_levels, err, err32, calls, berr, berr32 in conv_module_figures(dev):
        print(f"Conv2d_Q weight.grad ({route}, in_levels {in_levels}): err {err:.3e}, fp32 CPU err {err32:.3e}, "
              f"ratio {err / max(err32, EPS):.3f}; bias.grad err {berr:.3e}, fp32 CPU {berr32:.3e}")
        assert calls == 1                             # the first route alone ran the HIP weight gradient
        assert err <= R.C_WGRAD * max(err32, EPS), (route, in_levels, err, err32)
        assert berr <= R.C_WGRAD * max(berr32, EPS), (berr, berr32)


@pytest.mark.parametrize("a_bit", [4, 8])
def test_activation_quantizer_passes_the_clamp_mask(dev, a_bit):
    act = Q.activation_quantize_fn(a_bit)
    gen = torch.Generator().manual_seed(a_bit)
    x = torch.rand(3, 5, 7, generator=gen) * 1.4 - 0.2
    x.view(-1)[:4] = torch.tensor([0.0, 1.0, -0.1, 1.1])
    g = torch.randn(x.shape, generator=gen)
    xg = x.to(dev).requires_grad_(True)
    with torch.no_grad():
        y0 = act(xg)
    y = act(xg)
    assert torch.equal(y, y0)
    y.backward(g.to(dev))
    assert xg.grad is not None and bool((xg.grad != 0).any())
    assert torch.equal(xg.grad.cpu(), R.act_quant_backward(x, g))


def test_one_bit_conv_and_uniform_quantize_get_gradients(dev):
    torch.manual_seed(3)
    conv = Q.conv2d_Q_fn(1)(3, 4, 3, 1, 1).to(dev)
    x = torch.rand(2, 3, 6, 6, device=dev)
    conv(x).square().mean().backward()
    assert conv.weight.grad is not None and bool((conv.weight.grad != 0).any())
    # BatchNorm2d_Q's quantizer (uniform_quantize(k), quant_ultra.py:8-27): the rounding and the sign pass the
    # gradient straight through, forward values unchanged
    for k in (1, 4, 32):
        v = (torch.rand(37, device=dev) * 2 - 1).requires_grad_(True)
        g = torch.randn(37, device=dev)
        y = Q.uniform_quantize(k)(v)
        n = float(2 ** k - 1)
        want = v.detach() if k == 32 else (torch.sign(v.detach()) if k == 1 else torch.round(v.detach() * n) / n)
        assert torch.equal(y.detach(), want)
        y.backward(g)
        assert torch.equal(v.grad, g)


def linear_figures(dev):
    """Linear_Q(4-bit) 40 -> 24 on 6 rows: {name: (err against float64, err of the float32 CPU restatement)} for
    the input, weight and bias gradients."""
    torch.manual_seed(4)
    lin = Q.linear_Q_fn(4)(40, 24).to(dev)
    x = torch.randn(6, 40, device=dev, requires_grad=True)
    G = torch.randn(6, 24, device=dev)
    with torch.no_grad():
        y0 = lin(x)
    y = lin(x)
    assert torch.equal(y, y0)
    (y * G).sum().backward()
    wq = lin.quantize_fn(lin.weight).detach().cpu()
    Gc, xc, w = G.cpu(), x.detach().cpu(), lin.weight.detach().cpu().flatten()
    ref_x = Gc.double() @ wq.double()
    ref_w = R.weight_quant_backward(w, (Gc.double().t() @ xc.double()).flatten())
    ref_w32 = R.weight_quant_backward(w, (Gc.t() @ xc).flatten(), dtype=torch.float32)
    ref_b = Gc.double().sum(0)
    return {"input": (_rel(x.grad, ref_x), _rel(Gc @ wq, ref_x)),
            "weight": (_rel(lin.weight.grad.flatten(), ref_w), _rel(ref_w32, ref_w)),
            "bias": (_rel(lin.bias.grad, ref_b), _rel(Gc.sum(0), ref_b))}


def test_linear_q_gradients(dev):
    for name, (err, err32) in linear_figures(dev).items():
        print(f"Linear_Q {name}.grad: err {err:.3e}, fp32 CPU err {err32:.3e}, ratio {err / max(err32, EPS):.3f}")
        assert err <= R.C_LINEAR * max(err32, EPS), (name, err, err32)


# ---- the network ---------------------------------------------------------------------------------------------
def _clear_of_ties(model, x):
    """Makes the input (image, parameters) one on which the two forwards cannot round differently: walks the CPU
    restatement block by block and moves each BatchNorm bias, channel by channel, by the smallest multiple of 1e-4
    that leaves no pre-quantizer value of that channel within 1.25 TIE_BAND of a rounding tie or of the clamp's
    edges; weights whose normalised value lies within 1e-5 of a tie of the weight quantizer are nudged by 2e-3.
    Returns the pre-quantizer values."""
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.Conv2d):
                for _ in range(8):
                    t = torch.tanh(m.weight.double())
                    near = R.round_tie_distance((t / t.abs().max()).abs(), 7.0) < 1e-5
                    if not bool(near.any()):
                        break
                    m.weight[near] += 2e-3
        params = R.ultranet_params(model.state_dict())
        pre = []
        R.ultranet_forward(params, x, pre_quant=pre)
        for li in range(len(pre)):
            bias = model.layers[[1, 5, 9, 13, 17, 20, 23, 26][li]].bias
            v = pre[li]
            steps = torch.arange(2000, dtype=torch.float64) * 1e-4
            for c in range(v.shape[1]):
                d = R.tie_distance(v[:, c].reshape(1, -1).double() + steps[:, None], 15.0).min(dim=1).values
                ok = (d >= 1.25 * TIE_BAND).nonzero()
                assert ok.numel(), "no tie-free bias found"
                bias[c] += float(steps[int(ok[0])])
            params = R.ultranet_params(model.state_dict())
            pre = []
            R.ultranet_forward(params, x, pre_quant=pre)
    return pre


def _grads(model, x, route):
    prev, Q.ULTRA_BWD = Q.ULTRA_BWD, route
    try:
        model.zero_grad()
        out = model(x)
        assert isinstance(out, list) and out[0].grad_fn is not None
        out[0].square().mean().backward()
        return {k: p.grad.detach().clone() for k, p in model.named_parameters()}, out[0].detach()
    finally:
        Q.ULTRA_BWD = prev


def _restatement(state, x, dev, dtype):
    params = {k: v.to(dev, dtype).requires_grad_(True) for k, v in R.ultranet_params(state).items()}
    p = R.ultranet_forward(params, x.to(dev, dtype))
    p.square().mean().backward()
    return {k: v.grad for k, v in params.items()}, p.detach()


def network_figures(dev):
    """UltraNetQua().train() at 2 x 3 x 32 x 32, loss = p.square().mean(). Returns (grads per route, p per route,
    the torch-only restatement on the same device in float32, the same restatement on the CPU in float64 (the
    truth both are measured against), HIP weight-gradient calls under route "wgrad")."""
    torch.manual_seed(0)
    model = UltraNetQua().train()
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    pre = _clear_of_ties(model, x)
    # the condition on the input: no pre-quantizer value of the CPU restatement within TIE_BAND of a tie
    assert min(float(R.tie_distance(v, 15.0).min()) for v in pre) >= TIE_BAND
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            t = torch.tanh(m.weight.detach().double())
            assert float(R.round_tie_distance((t / t.abs().max()).abs(), 7.0).min()) >= 1e-5
    state = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev)
    xd = x.to(dev)
    calls = []
    real = Q._lib.conv_wgrad
    Q._lib.conv_wgrad = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        routes = {}
        for r in ("hip", "wgrad", "dgrad", "torch"):   # the default mix, each op on HIP at every layer, the library
            n0 = len(calls)
            routes[r] = _grads(model, xd, r)
            if r == "wgrad":
                wgrad_calls = len(calls) - n0
    finally:
        Q._lib.conv_wgrad = real
    return routes, _restatement(state, x, dev, torch.float32), _restatement(state, x, "cpu", torch.float64), \
        wgrad_calls


def test_ultranet_trains(dev):
    routes, (g32, p32), (g64, p64), wgrad_calls = network_figures(dev)
    # forward_modules tells every conv but layer 0 (float image) that its input holds codes: with wgrad selected
    # each of those 8 convs runs qvit_conv_wgrad
    assert wgrad_calls == 8
    for k, g in routes["hip"][0].items():
        assert bool(torch.isfinite(g).all()) and bool((g != 0).any()), k
    perr32 = _rel(p32, p64)
    for r, (grads, p) in routes.items():
        print(f"p ({r}): err {_rel(p, p64):.3e}, fp32 restatement err {perr32:.3e}")
        assert _rel(p, p64) <= R.C_NET * max(perr32, EPS), r
    worst = 0.0
    for k in g64:
        err32 = _rel(g32[k], g64[k])
        for r in ("hip", "wgrad", "dgrad", "torch"):
            err = _rel(routes[r][0][k], g64[k])
            print(f"{k} ({r}): err {err:.3e}, fp32 restatement err {err32:.3e}, ratio {err / max(err32, EPS):.3f}")
            # against the float64 truth, in units of the same-device float32 restatement's own error
            assert err <= R.C_NET * max(err32, EPS), (k, r, err, err32)
            # and so against that restatement itself (triangle inequality)
            assert _rel(routes[r][0][k], g32[k]) <= (R.C_NET + 1) * max(err32, EPS), (k, r)
        d = _rel(routes["torch"][0][k], routes["hip"][0][k])
        worst = max(worst, d)
        print(f"{k}: torch route vs default {d:.3e}")
        assert d <= R.NET_TORCH_VS_DEFAULT, (k, d)
    print(f"worst torch route vs default {worst:.3e}")
