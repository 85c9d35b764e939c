"""QuantizeLinear with quant_layers.A16_GEMM on: W+A layers with 9- to 16-bit activations run qvit_quantize_act_i16 +
qvit_gemm_a16 and never reach qvit_fake_quant_f32 or qvit_gemm_wonly in the forward; the default keeps the old route."""
import pytest
import torch

from quantized_vit_amd import _lib, quant_layers as ql

pytestmark = pytest.mark.gpu

WA = ql.QuantizationMode.WEIGHT_AND_ACTIVATION
# (weight bits, activation bits, the plan's weight format); equal bits: initialize_quant_layer alone
CONFIGS = [(9, 9, _lib.W16), (12, 12, _lib.W16), (16, 16, _lib.W24), (8, 12, _lib.W8), (4, 12, _lib.W4)]


def _old_route(*a, **k):
    raise RuntimeError("old route reached")


def _layer(dev, fin, fout, wbits, abits):
    torch.manual_seed(fin + wbits)
    layer = ql.QuantizeLinear(fin, fout, quant_mode=WA).to(dev)
    ql.initialize_quant_layer(layer, num_bits=wbits, quant_mode=WA)
    if abits != wbits:   # activation scalars by hand: the same range at abits
        with torch.no_grad():
            layer.d_quant_act.copy_(layer.q_m_act / (2 ** (abits - 1) - 1))
        layer.invalidate()
    return layer.eval()   # the plan is kept between calls: nothing but the forward itself can reach the old kernels


def _step(layer, x, G, monkeypatch, on, patched):
    """One forward + backward with the switch `on`; the old route's kernels raise during the forward if `patched`."""
    layer.zero_grad()
    xg = x.clone().requires_grad_(True)
    with monkeypatch.context() as mp:
        mp.setattr(ql, "A16_GEMM", on)
        if patched:
            mp.setattr(_lib, "gemm_wonly", _old_route)
            mp.setattr(_lib, "fake_quant_f32", _old_route)
        y = layer(xg)
        with torch.no_grad():
            y_ng = layer(x)
    (y * G).sum().backward()
    grads = {"input": xg.grad}
    grads.update({n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None})
    return y.detach(), y_ng, grads


@pytest.mark.parametrize("fin, fout", [(100, 48), (200, 300)])
@pytest.mark.parametrize("wbits, abits, wfmt", CONFIGS)
def test_layer_on_the_a16_kernels(dev, monkeypatch, fin, fout, wbits, abits, wfmt):
    layer = _layer(dev, fin, fout, wbits, abits)
    plan = layer.quant_plan()
    assert plan.extra.get("wonly") and plan.wfmt == wfmt and 128 <= plan.level_act <= 32767
    g = torch.Generator().manual_seed(fout)
    x = (1.2 * float(layer.q_m_act.detach()) * (2 * torch.rand(2, 35, fin, generator=g) - 1)).to(dev)   # some saturate
    G = torch.randn(2, 35, fout, generator=g).to(dev)
    ka = (layer.quantize_act(x).detach() / plan.d_act).round().reshape(-1, fin).double().cpu()
    kw = layer.weight_codes().double().cpu()
    assert ka.abs().max() == plan.level_act and ka.abs().min() < 128   # both digits in use

    y, y_ng, g_on = _step(layer, x, G, monkeypatch, True, patched=True)
    assert torch.equal(y, y_ng)                                        # autograd and no_grad: the same bits
    prod = float(plan.d_act.double() * plan.d_wt.double()) * (ka @ kw.t())   # |S| < 2^53: exact in fp64
    bias = layer.bias.detach().double().cpu()
    err = (y.reshape(-1, fout).double().cpu() - (prod + bias)).abs()
    bound = 2.0 ** -23 * (prod + bias).abs() + 2.0 ** -50 * (prod.abs() + bias.abs())
    print(f"W{wbits}A{abits} {fin}x{fout}: forward worst err / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())

    _, _, g_off = _step(layer, x, G, monkeypatch, False, patched=False)
    assert set(g_on) == set(g_off) and {"input", "weight", "bias", "d_quant_wt", "d_quant_act"} <= set(g_on)
    for name, want in g_off.items():
        diff, top = float((g_on[name] - want).abs().max()), float(want.abs().max())
        print(f"  grad {name}: max diff {diff:.3e}, max |default| {top:.3e}")
        assert diff <= 2.0 ** -15 * top, name

    with pytest.raises(RuntimeError, match="old route reached"):      # off by default
        _step(layer, x, G, monkeypatch, ql.A16_GEMM, patched=True)
