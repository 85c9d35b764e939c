"""The backward GEMMs of QuantizeLinear on the HIP kernels (quant_layers.BACKWARD_GEMM): dgrad as qvit_gemm_wonly on
the transposed weight codes, wgrad as qvit_gemm_wgrad on the int8 activation codes. Checked against the float64 CPU
autograd graph of tests/test_gpu_layer_autograd.py with its bounds, route by route, plus the route selection itself
and a tiny ViT whose two routes must agree to summation-order rounding."""
import numpy as np
import pytest
import torch

import quant_backward_ref as R
import test_gpu_layer_autograd as T

pytestmark = pytest.mark.gpu

CLIP = T.CLIP
SHAPES = [(10, 64, 48), (70, 200, 1000)]   # (M, K, N): one tile; every dimension ragged, N the classifier head's


def _build(dev, kind, path, shape, seed=0, wq=None, aq=None):
    """A QuantizeLinear of the given shape in the quantizer state T._case(kind, path) (or wq / aq), tie-free
    weights and inputs. Returns what T._build returns."""
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeLinear
    M, K, N = shape
    mode, wq0, aq0 = T._case(kind, path)
    wq, aq = wq or wq0, (aq or aq0) if aq0 is not None else None
    qt = QuantizationType.SYMMETRIC_LINEAR if kind == R.LINEAR else QuantizationType.SYMMETRIC_NONLINEAR
    qm = QuantizationMode.WEIGHT_AND_ACTIVATION if mode == "wa" else QuantizationMode.WEIGHT_ONLY
    layer = QuantizeLinear(K, N, bias=True, quant_type=qt, quant_mode=qm).to(dev).eval()
    W = R.tie_free_values((N, K), kind, *wq, seed=seed + 10)
    gen = torch.Generator().manual_seed(seed + 20)
    b = 0.1 * torch.randn(N, generator=gen)
    layer.weight.data.copy_(W)
    layer.bias.data.copy_(b)
    for name, v in zip(("d_quant_wt", "q_m_wt", "t_quant_wt"), wq):
        T._set(getattr(layer, name, None), v)
    if aq is not None:
        for name, v in zip(("d_quant_act", "q_m_act", "t_quant_act"), aq):
            T._set(getattr(layer, name, None), v)
        x = R.tie_free_values((M, K), kind, *aq, seed=seed + 30)
    else:
        x = torch.randn((M, K), generator=gen)
    layer.invalidate()
    return layer, x, W, b, wq, aq


def _spy(monkeypatch, obj, name):
    calls = []
    orig = getattr(obj, name)

    def wrapped(*a, **k):
        calls.append(name)
        return orig(*a, **k)
    monkeypatch.setattr(obj, name, wrapped)
    return calls


def _spies(monkeypatch):
    from quantized_vit_amd import _lib
    return (_spy(monkeypatch, _lib, "gemm_wonly"), _spy(monkeypatch, _lib, "gemm_wgrad"),
            _spy(monkeypatch, torch, "mm"))


def _route(monkeypatch, route):
    from quantized_vit_amd import quant_layers as ql
    monkeypatch.setattr(ql, "BACKWARD_GEMM", route)


# ---- dgrad alone ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("path", ["int", "wonly", "wide16"])
def test_dgrad_on_the_weight_only_kernel(dev, monkeypatch, path, shape):
    kind = R.LINEAR
    M, K, N = shape
    _route(monkeypatch, "dgrad")
    layer, x, W, b, wq, aq = _build(dev, kind, path, shape)
    plan = layer.quant_plan()
    assert plan.int_path == (path == "int") and (path == "int" or plan.extra.get("wonly"))
    wonly, wgrad, mm = _spies(monkeypatch)
    xd = x.to(dev).requires_grad_(True)
    y = layer(xd)
    gen = torch.Generator().manual_seed(99)
    Gw = torch.randn(y.shape, generator=gen)
    del wonly[:], mm[:]
    (y * Gw.to(dev)).sum().backward()
    assert len(wonly) == 1 and len(wgrad) == 0 and len(mm) == 1      # dgrad on the kernel, wgrad on the library
    ref = T._reference(kind, x, W, b, wq, aq, Gw, False)
    bound = 4 * N * 2.0 ** -24 * (Gw.double().abs() @ ref["wq"].abs())
    err = (xd.grad.cpu().double() - ref["x"].grad).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"dgrad {path} {shape}: max err {float(err.max()):.3e}, worst err / bound {worst:.4f}")
    assert bool((err <= bound).all()), (float(err.max()), worst)
    assert "packed_t" in plan.extra                                  # the transposed image stays with the plan
    img = plan.extra["packed_t"][0]
    layer(xd).sum().backward()
    assert plan.extra["packed_t"][0] is img


@pytest.mark.parametrize("path,shape", [("int", SHAPES[0]), ("int", SHAPES[1]), ("wonly", SHAPES[0]),
                                        ("wonly", SHAPES[1]), ("wide16", SHAPES[0])])
def test_dgrad_exact_on_integers(dev, path, shape):
    """G small integers and d_wt a power of two: every product and partial sum is exact in fp32 (below 2^24 d_wt:
    8 * 7 * 1000 on int4 codes, 8 * 32767 * 48 on the 16-bit ones), so the result equals the float64 product."""
    kind = R.LINEAR
    M, K, N = shape
    level, d = (32767, 2.0 ** -16) if path == "wide16" else (7, 2.0 ** -4)
    wq = (d, level * d, None)
    layer, x, *_ = _build(dev, kind, path, shape, wq=wq)
    plan = layer.quant_plan()
    assert abs(plan.level_wt) == level
    gen = torch.Generator().manual_seed(5)
    G = torch.randint(-8, 9, (M, N), generator=gen, dtype=torch.int32).float()
    gx, _ = layer._gemm_grads_hip(plan, x.to(dev), None, None, G.to(dev), True, False)
    want = G.double() @ (d * layer.weight_codes().cpu().double())
    assert torch.equal(gx.cpu().double(), want)


# ---- route selection ------------------------------------------------------------------------------------------
def _backward_calls(dev, monkeypatch, route, path, freeze_weight=False):
    _route(monkeypatch, route)
    layer, x, *_ = _build(dev, R.LINEAR, path, SHAPES[0])
    if freeze_weight:
        for name in ("weight", "d_quant_wt", "q_m_wt"):
            getattr(layer, name).requires_grad_(False)
    wonly, wgrad, mm = _spies(monkeypatch)
    xd = x.to(dev).requires_grad_(True)
    y = layer(xd)
    del wonly[:], wgrad[:], mm[:]
    y.sum().backward()
    assert xd.grad is not None and bool(torch.isfinite(xd.grad).all())
    return len(wonly), len(wgrad), len(mm), layer


def test_hip_route_runs_both_kernels(dev, monkeypatch):
    wonly, wgrad, mm, layer = _backward_calls(dev, monkeypatch, "hip", "int")
    assert (wonly, wgrad, mm) == (1, 1, 0)      # fails without the feature: there is no _lib.gemm_wgrad
    assert layer.weight.grad is not None


def test_torch_route_is_the_library(dev, monkeypatch):
    assert _backward_calls(dev, monkeypatch, "torch", "int")[:3] == (0, 0, 2)


def test_single_op_routes(dev, monkeypatch):
    assert _backward_calls(dev, monkeypatch, "dgrad", "int")[:3] == (1, 0, 1)
    assert _backward_calls(dev, monkeypatch, "wgrad", "int")[:3] == (0, 1, 1)


def test_weight_only_layer_never_runs_wgrad(dev, monkeypatch):
    assert _backward_calls(dev, monkeypatch, "hip", "wonly")[:3] == (1, 0, 1)


def test_frozen_weight_skips_wgrad(dev, monkeypatch):
    wonly, wgrad, mm, layer = _backward_calls(dev, monkeypatch, "hip", "int", freeze_weight=True)
    assert (wonly, wgrad, mm) == (1, 0, 0)
    assert layer.weight.grad is None and layer.bias.grad is not None


def test_unknown_route_is_an_error(dev, monkeypatch):
    with pytest.raises(ValueError):
        _backward_calls(dev, monkeypatch, "cublas", "int")


# ---- both routes on one layer -----------------------------------------------------------------------------------
def _layer_grads(dev, monkeypatch, route, kind, shape):
    """Every gradient of an int-path layer on `route`, checked against the float64 graph with the bounds of
    tests/test_gpu_layer_autograd.py. Returns the six quantizer-scalar gradients and their sum_bounds."""
    M, K, N = shape
    _route(monkeypatch, route)
    layer, x, W, b, wq, aq = _build(dev, kind, "int", shape)
    assert layer.quant_plan().int_path
    xd = x.to(dev).requires_grad_(True)
    y = layer(xd)
    gen = torch.Generator().manual_seed(99)
    Gw = torch.randn(y.shape, generator=gen)
    (y * Gw.to(dev)).sum().backward()
    ref = T._reference(kind, x, W, b, wq, aq, Gw, False)
    G, u = Gw.double(), 2.0 ** -24
    checks = [("bias.grad", layer.bias.grad, ref["b"].grad, 4 * M * u * G.abs().sum(0)),
              ("weight.grad", layer.weight.grad, ref["W"].grad, 4 * M * u * (G.abs().t() @ ref["xq"].abs())),
              ("input.grad", xd.grad, ref["x"].grad, 4 * N * u * (G.abs() @ ref["wq"].abs()))]
    for name, got, want, bound in checks:
        err = (got.detach().cpu().double() - want).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{route} {kind} {shape} {name}: max err {float(err.max()):.3e}, worst err / bound {worst:.4f}")
        assert bool((err <= bound).all()), (route, name, float(err.max()), worst)
    scal, bnds = [], []
    for which, values, params, leaves, rec in (("wt", W, wq, ref["pw"], ref["rec_w"]),
                                               ("act", x, aq, ref["pa"], ref["rec_a"])):
        _, _, _, bounds = R.sum_bounds(values.reshape(-1), rec["grad_out"].reshape(-1).float(), kind, *params,
                                       clip=CLIP)
        for i, name in enumerate(("d_quant", "q_m", "t_quant")):
            p = getattr(layer, f"{name}_{which}", None)
            if p is None:
                continue
            err = abs(float(p.grad) - float(leaves[i].grad))
            print(f"{route} {kind} {shape} {name}_{which}.grad: err {err:.3e} bound {bounds[i]:.3e}")
            assert err <= bounds[i], (route, name, which, err, bounds[i])
            scal.append(float(p.grad))
            bnds.append(float(bounds[i]))
    return scal, bnds


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", [R.LINEAR, R.NONLINEAR])
def test_both_routes_match_float64(dev, monkeypatch, kind, shape):
    hip, bounds = _layer_grads(dev, monkeypatch, "hip", kind, shape)
    lib, _ = _layer_grads(dev, monkeypatch, "torch", kind, shape)
    assert len(hip) == len(lib) == (4 if kind == R.LINEAR else 6)
    for a, c, bound in zip(hip, lib, bounds):
        assert abs(a - c) <= bound, (a, c, bound)


# ---- a tiny ViT ---------------------------------------------------------------------------------------------------
# Worst per-parameter relative difference max|g_hip - g_torch| / max|g_torch| between the two routes, measured on
# the MI355X: both are fp32 evaluations of the same sums in different orders. The cap is
# four times the measured value rounded up to a power of two.
TINY_VIT_MEASURED = 4.17e-6        # blocks.1.attn.proj.d_quant_act
TINY_VIT_CAP = 2.0 ** -15          # 4 * 4.17e-6 = 1.67e-5 -> 3.05e-5


def test_tiny_vit_routes_agree(dev, monkeypatch):
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType
    from quantized_vit_amd.quant_model import model_to_quantize_model
    from quantized_vit_amd.vit_model import VisionTransformer
    torch.manual_seed(0)
    model = VisionTransformer(img_size=32, patch_size=16, embed_dim=192, depth=2, num_heads=3, num_classes=10)
    model = model_to_quantize_model(model.to(dev), num_bits=4, quant_type=QuantizationType.SYMMETRIC_LINEAR,
                                    quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION).eval()
    x = torch.randn(2, 3, 32, 32, device=dev)
    grads = {}
    for route in ("hip", "torch"):
        _route(monkeypatch, route)
        model.zero_grad(set_to_none=True)
        model(x).sum().backward()
        grads[route] = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
        for n, g in grads[route].items():
            assert bool(torch.isfinite(g).all()), (route, n)
    worst, where = 0.0, None
    for n, g in grads["torch"].items():
        scale = float(g.abs().max())
        diff = float((grads["hip"][n] - g).abs().max())
        rel = diff / scale if scale > 0 else (0.0 if diff == 0 else float("inf"))
        if rel > worst:
            worst, where = rel, n
    print(f"tiny ViT, hip vs torch backward GEMMs: worst per-parameter relative difference {worst:.3e} ({where})")
    assert worst <= TINY_VIT_CAP, (worst, where)
