"""QuantizeLinear with quant_layers.F32_GEMM = "hip": the contractions that have no code image to run on (forward and
dgrad beyond 65536 weight levels, wgrad wherever the layer is off the integer path) go through qvit_gemm_f32_nt /
qvit_gemm_f32_tn and never reach the library's GEMMs; the default keeps them there."""
import pytest
import torch

from quantized_vit_amd import quant_layers as ql

pytestmark = pytest.mark.gpu

WA, WO = ql.QuantizationMode.WEIGHT_AND_ACTIVATION, ql.QuantizationMode.WEIGHT_ONLY
LIN, NONLIN = ql.QuantizationType.SYMMETRIC_LINEAR, ql.QuantizationType.SYMMETRIC_NONLINEAR
# (bits, quantizer, mode, the plan holds packed weight codes): without codes all three ops are new, with them wgrad
CONFIGS = [(32, LIN, WA, False), (20, NONLIN, WA, False), (12, LIN, WA, True), (16, LIN, WO, True)]


def _library_gemm(*a, **k):
    raise RuntimeError("library GEMM reached")


def _step(layer, x, G, monkeypatch, route, patched):
    """One forward + backward on `route`; the library's GEMMs raise if `patched`. Returns (output, gradients)."""
    with monkeypatch.context() as mp:
        mp.setattr(ql, "F32_GEMM", route)
        if patched:
            mp.setattr(torch, "mm", _library_gemm)
            mp.setattr(torch.nn.functional, "linear", _library_gemm)
        layer.zero_grad()
        xg = x.clone().requires_grad_(True)
        y = layer(xg)
        (y * G).sum().backward()
    grads = {"input": xg.grad}
    grads.update({n: p.grad.clone() for n, p in layer.named_parameters() if p.grad is not None})
    return y.detach(), grads


@pytest.mark.parametrize("bits, qtype, mode, has_codes", CONFIGS)
def test_layer_on_the_f32_kernels(dev, monkeypatch, bits, qtype, mode, has_codes):
    torch.manual_seed(0)
    layer = ql.QuantizeLinear(100, 48, quant_type=qtype, quant_mode=mode).to(dev)
    ql.initialize_quant_layer(layer, num_bits=bits, quant_type=qtype, quant_mode=mode)
    x = (0.05 * torch.randn(2, 35, 100)).to(dev)
    G = torch.randn(2, 35, 48).to(dev)
    plan = layer.quant_plan()
    assert not plan.int_path and plan.has_codes == has_codes

    y, g_hip = _step(layer, x, G, monkeypatch, "hip", patched=True)
    xq = (layer.quantize_act(x) if mode == WA else x).detach().reshape(-1, 100).double()
    wq = layer.w_fakequant(layer.quant_plan()).detach().reshape(48, 100).double()
    ref = xq @ wq.t() + layer.bias.detach().double()
    bound = (4 * 100 + 9) * 2.0 ** -24 * (xq.abs() @ wq.abs().t())
    err = (y.reshape(-1, 48).double() - ref).abs()
    print(f"{bits}-bit {qtype.name} {mode.name}: forward worst err / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())

    _, g_torch = _step(layer, x, G, monkeypatch, "torch", patched=False)
    assert set(g_hip) == set(g_torch) and {"input", "weight", "bias", "d_quant_wt", "q_m_wt"} <= set(g_hip)
    for name, want in g_torch.items():
        diff, top = float((g_hip[name] - want).abs().max()), float(want.abs().max())
        print(f"  grad {name}: max diff {diff:.3e}, max |torch| {top:.3e}")
        assert diff <= 2.0 ** -15 * top, name

    with pytest.raises(RuntimeError, match="library GEMM reached"):   # off by default
        _step(layer, x, G, monkeypatch, ql.F32_GEMM, patched=True)
