"""quant_layers.F6_GEMM: with the switch on, a 4-bit W+A QuantizeLinear runs qvit_quantize_act_f6 + qvit_gemm_f6 in its
forward, under no_grad and under autograd, and neither the output nor any gradient changes by a bit; a layer at 8 bits
stays on the int8 route."""
import pytest
import torch

from quantized_vit_amd import _lib, quant_layers as ql

pytestmark = pytest.mark.gpu

WA = ql.QuantizationMode.WEIGHT_AND_ACTIVATION


def _run(layer, x, G, monkeypatch, on):
    """(forward under no_grad, forward under autograd, gradients, rows seen by gemm_f6) with the switch `on`."""
    calls = []
    gemm_f6 = _lib.gemm_f6
    layer.zero_grad()
    xg = x.clone().requires_grad_(True)
    with monkeypatch.context() as mp:
        mp.setattr(ql, "F6_GEMM", on)
        mp.setattr(_lib, "gemm_f6", lambda *a, **k: (calls.append(a[1]), gemm_f6(*a, **k))[1])
        with torch.no_grad():
            y_ng = layer(x)
        y = layer(xg)
        (y * G).sum().backward()
    grads = {"input": xg.grad}
    grads.update({n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None})
    return y_ng, y.detach(), grads, calls


@pytest.mark.parametrize("bits, routed", [(4, True), (8, False)])
@pytest.mark.parametrize("qtype", [ql.QuantizationType.SYMMETRIC_LINEAR, ql.QuantizationType.SYMMETRIC_NONLINEAR])
def test_layer_bit_identical_with_the_switch(dev, monkeypatch, qtype, bits, routed):
    torch.manual_seed(bits)
    layer = ql.QuantizeLinear(200, 136, quant_type=qtype, quant_mode=WA).to(dev)   # kpad above k, npad above n
    ql.initialize_quant_layer(layer, num_bits=bits, quant_type=qtype, quant_mode=WA)
    layer.eval()
    plan = layer.quant_plan()
    assert plan.int_path and (abs(plan.level_act) <= 7 and abs(plan.level_wt) <= 7) == routed
    g = torch.Generator().manual_seed(136)
    x = (1.2 * float(layer.q_m_act.detach()) * (2 * torch.rand(67, 200, generator=g) - 1)).to(dev)   # some saturate
    G = torch.randn(67, 136, generator=g).to(dev)
    ng_off, y_off, g_off, calls_off = _run(layer, x, G, monkeypatch, False)
    ng_on, y_on, g_on, calls_on = _run(layer, x, G, monkeypatch, True)
    assert calls_off == [] and calls_on == ([67, 67] if routed else [])
    assert torch.equal(ng_on, ng_off) and torch.equal(y_on, y_off) and torch.equal(y_on, ng_on)
    assert set(g_on) == set(g_off) and {"input", "weight", "d_quant_act"} <= set(g_on)
    for name, want in g_off.items():
        assert torch.equal(g_on[name], want), name
