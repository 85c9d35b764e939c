"""tests/ultra_backward_ref.py against torch autograd of the reference's own expressions in float64 (tanh, / max|.|,
a straight-through round, clamp, F.conv2d): the closed forms the HIP kernels implement, the tie rule and the clamp
mask's boundaries included. No GPU."""
import pytest
import torch
import torch.nn.functional as F

import ultra_backward_ref as R


def _autograd_weight_backward(w, g, w_bit=4):
    w = w.double().clone().requires_grad_(True)
    R.weight_quantize(w, w_bit).backward(g.double())
    return w.grad


@pytest.mark.parametrize("case", ["tie", "unique", "all_equal", "random"])
def test_weight_quant_backward_matches_autograd(case):
    gen = torch.Generator().manual_seed(1)
    if case == "tie":
        w = torch.tensor([0.5, -2.0, 2.0, 1.0])
    elif case == "unique":
        w = torch.tensor([0.5, -2.0, 1.5, 1.0, 0.0])
    elif case == "all_equal":
        w = torch.tensor([0.7, -0.7, 0.7, 0.7])
    else:
        w = torch.randn(257, generator=gen)
    g = torch.randn(w.shape, generator=gen)
    want = _autograd_weight_backward(w, g)
    got = R.weight_quant_backward(w, g)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-14), (got - want).abs().max()
    if case == "tie":   # both tied elements receive the share: their gradients differ from g / m (1 - t^2)
        t = torch.tanh(w.double())
        plain = g.double() / t.abs().max() * (1 - t * t)
        assert bool(((got - plain).abs()[1:3] > 1e-6).all()) and torch.allclose(got[[0, 3]], plain[[0, 3]])


def test_weight_quant_backward_nan_selects():
    w = torch.tensor([0.5, -2.0, 2.0, 1.0])
    g = torch.tensor([float("nan"), 1.0, 1.0, 1.0])
    got = R.weight_quant_backward(w, g)
    assert torch.isnan(got).tolist() == [True, True, True, False]   # element 0, and the ties through the sum
    want = _autograd_weight_backward(w, g)
    assert torch.isnan(want).tolist() == torch.isnan(got).tolist()


def test_act_quant_backward_is_the_clamp_mask():
    x = torch.tensor([0.0, 1.0, -0.1, 1.1, float("nan"), 0.5], dtype=torch.float64, requires_grad=True)
    g = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], dtype=torch.float64)
    R.act_quantize(x, 4).backward(g)
    got = R.act_quant_backward(x.detach(), g)
    assert got.tolist() == [1.0, 2.0, 0.0, 0.0, 0.0, 6.0]
    assert torch.equal(got, x.grad)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7, 5, 3, 1, 1, 1), (1, 4, 11, 13, 8, 3, 2, 1, 1),
                                   (1, 4, 11, 13, 8, 3, 1, 2, 2), (3, 8, 4, 4, 6, 1, 1, 0, 1)])
def test_conv_gradients_match_autograd(shape):
    B, C, H, W, N, k, s, p, d = shape
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn(N, C, k, k, generator=gen, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, s, p, d)
    G = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(G)
    args = ((k, k), (s, s), (p, p), (d, d))
    assert torch.allclose(R.conv_wgrad(G, x.detach(), *args), w.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.conv_dgrad(G, w.detach(), (H, W), *args[1:]), x.grad, rtol=1e-12, atol=1e-12)


def test_dgrad_is_a_forward_conv_on_the_flipped_transposed_weight():
    """The identity the HIP route uses: for stride 1, dX = conv2d(G, flip(w)^T, padding d (k - 1) - p)."""
    gen = torch.Generator().manual_seed(3)
    for (k, p, d) in ((3, 1, 1), (3, 2, 2), (1, 0, 1), (3, 0, 1)):
        G = torch.randn(2, 5, 9 + 2 * p - d * (k - 1), 8 + 2 * p - d * (k - 1), generator=gen, dtype=torch.float64)
        w = torch.randn(5, 4, k, k, generator=gen, dtype=torch.float64)
        wt = w.flip(2, 3).permute(1, 0, 2, 3)
        got = F.conv2d(G, wt, None, 1, d * (k - 1) - p, d)
        want = R.conv_dgrad(G, w, (9, 8), (1, 1), (p, p), (d, d))
        assert (got - want).abs().max() <= 1e-13 * want.abs().max()


def test_ultranet_restatement_shapes_and_grads():
    gen = torch.Generator().manual_seed(4)
    params = {}
    i = 0
    for cin, cout, pool in R.ULTRA_STACK:
        params[f"layers.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=gen) * 0.1
        params[f"layers.{i + 1}.weight"] = torch.ones(cout)
        params[f"layers.{i + 1}.bias"] = torch.full((cout,), 0.5)
        i += 4 if pool else 3
    params[f"layers.{i}.weight"] = torch.randn(36, 64, 1, 1, generator=gen) * 0.1
    params[f"layers.{i}.bias"] = torch.zeros(36)
    assert i == 28
    for v in params.values():
        v.requires_grad_(True)
    p = R.ultranet_forward(params, torch.rand(2, 3, 32, 32, generator=gen))
    assert p.shape == (2, 6, 2, 2, 6)
    p.square().mean().backward()
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in params.values())
