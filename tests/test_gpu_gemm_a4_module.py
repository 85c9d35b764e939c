"""quant_layers.A4_GEMM: with the switch on, a 4-bit W+A QuantizeLinear runs qvit_quantize_act_i4 + qvit_gemm_a4 in its
forward, under no_grad and under autograd, and neither the output nor any gradient changes by a bit; a layer with more
than 7 activation levels stays on the int8 route."""
import pytest
import torch

from quantized_vit_amd import _lib, quant_layers as ql

pytestmark = pytest.mark.gpu

WA = ql.QuantizationMode.WEIGHT_AND_ACTIVATION


def _run(layer, x, G, monkeypatch, on):
    """(forward under no_grad, forward under autograd, gradients, rows seen by gemm_a4) with the switch `on`."""
    calls = []
    gemm_a4 = _lib.gemm_a4
    layer.zero_grad()
    xg = x.clone().requires_grad_(True)
    with monkeypatch.context() as mp:
        mp.setattr(ql, "A4_GEMM", on)
        mp.setattr(_lib, "gemm_a4", lambda *a, **k: (calls.append(a[1]), gemm_a4(*a, **k))[1])
        with torch.no_grad():
            y_ng = layer(x)
        y = layer(xg)
        (y * G).sum().backward()
    grads = {"input": xg.grad}
    grads.update({n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None})
    return y_ng, y.detach(), grads, calls


@pytest.mark.parametrize("bits, routed", [(4, True), (8, False)])
@pytest.mark.parametrize("fin, fout", [(768, 200), (200, 768)])   # npad above n; kpad above k
def test_layer_bit_identical_with_the_switch(dev, monkeypatch, fin, fout, bits, routed):
    torch.manual_seed(fin + bits)
    layer = ql.QuantizeLinear(fin, fout, quant_mode=WA).to(dev)
    ql.initialize_quant_layer(layer, num_bits=bits, quant_mode=WA)
    layer.eval()
    plan = layer.quant_plan()
    assert plan.int_path and (abs(plan.level_act) <= 7) == routed
    g = torch.Generator().manual_seed(fout)
    x = (1.2 * float(layer.q_m_act.detach()) * (2 * torch.rand(197, fin, generator=g) - 1)).to(dev)   # some saturate
    G = torch.randn(197, fout, generator=g).to(dev)
    ng_off, y_off, g_off, calls_off = _run(layer, x, G, monkeypatch, False)
    ng_on, y_on, g_on, calls_on = _run(layer, x, G, monkeypatch, True)
    assert calls_off == [] and calls_on == ([197, 197] if routed else [])
    assert torch.equal(ng_on, ng_off) and torch.equal(y_on, y_off) and torch.equal(y_on, ng_on)
    assert set(g_on) == set(g_off) and {"input", "weight", "d_quant_act"} <= set(g_on)
    for name, want in g_off.items():
        assert torch.equal(g_on[name], want), name
