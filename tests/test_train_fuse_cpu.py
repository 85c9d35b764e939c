"""The float64 restatements of tests/train_fuse_ref.py against torch autograd (F.layer_norm / F.gelu composed with
the reference quantizer's float64 Function), their float32 runs against the floors the GPU tests use, and the
survival rate of the tie filter for every parametrisation of the GPU tests. No GPU."""
import pytest
import torch
import torch.nn.functional as F

import quant_backward_ref as R
import train_fuse_ref as T
from quant_backward_ref import CLIPS

_ids = lambda p: f"{p[0]}-t{p[3]}"


def _params64(d, q_m, t):
    f = lambda v: None if v is None else torch.tensor([float(torch.tensor(v, dtype=torch.float32))],
                                                      dtype=torch.float64, requires_grad=True)
    return f(d), f(q_m), f(t)


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("params", T.QUANTIZERS, ids=_ids)
def test_layernorm_restatement_is_autograd(params, clip):
    kind, d, q_m, t = params
    x, gamma, beta, g, _ = T.ln_inputs(9, 64, kind, d, q_m, t, clip)
    r = T.ln_quant_backward_ref(x, gamma, beta, g, kind, d, q_m, t, clip)
    xa = x.double().requires_grad_(True)
    ga, ba = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    pd, pq, pt = _params64(d, q_m, t)
    y = F.layer_norm(xa, (64,), ga, ba, T.LN_EPS)
    out = R.RefQuantizer.apply(y, pd, pq, pt, kind, clip, {})
    out.backward(g.double())
    assert torch.allclose(xa.grad, r["grad_x"], rtol=1e-10, atol=1e-12)
    assert torch.allclose(ga.grad, r["grad_gamma"], rtol=1e-10, atol=1e-12)
    assert torch.allclose(ba.grad, r["grad_beta"], rtol=1e-10, atol=1e-12)
    for p, s in zip((pd, pq, pt), r["sums"]):
        if p is not None:
            assert torch.allclose(p.grad.reshape(()), s, rtol=1e-10, atol=1e-12)
    assert 0 < int(r["masked"].sum()) < x.numel() or clip == CLIPS[0]


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("params", T.QUANTIZERS, ids=_ids)
def test_gelu_restatement_is_autograd(params, clip):
    kind, d, q_m, t = params
    h, g, _ = T.gelu_inputs(1023, kind, d, q_m, t, clip)
    r = T.gelu_quant_backward_ref(h, g, kind, d, q_m, t, clip)
    ha = h.double().requires_grad_(True)
    pd, pq, pt = _params64(d, q_m, t)
    out = R.RefQuantizer.apply(F.gelu(ha), pd, pq, pt, kind, clip, {})
    out.backward(g.double())
    assert torch.allclose(ha.grad, r["grad_h"], rtol=1e-10, atol=1e-14)
    for p, s in zip((pd, pq, pt), r["sums"]):
        if p is not None:
            assert torch.allclose(p.grad.reshape(()), s, rtol=1e-10, atol=1e-12)


def _ratio(v32, v64, floor):
    return float(((v32.double() - v64).abs() / floor.clamp(min=1e-300)).max())


@pytest.mark.parametrize("shape", [(5, 64), (333, 192), (7, 768), (2, 2048)])
@pytest.mark.parametrize("params", T.QUANTIZERS, ids=_ids)
def test_layernorm_float32_run_stays_below_the_floors(params, shape):
    """|ref32 - ref64| <= floor for grad_x (elementwise, where no side masks), the column sums and the scalar
    sums: plain float32 arithmetic in torch's order of operations sits inside the analytic floor."""
    kind, d, q_m, t = params
    clip = CLIPS[1]
    x, gamma, beta, g, _ = T.ln_inputs(*shape, kind, d, q_m, t, clip)
    r64 = T.ln_quant_backward_ref(x, gamma, beta, g, kind, d, q_m, t, clip)
    r32 = T.ln_quant_backward_ref(x, gamma, beta, g, kind, d, q_m, t, clip, dtype=torch.float32)
    assert torch.equal(r32["masked"], r64["masked"])   # the tie filter's purpose
    fg, fb = T.ln_col_floors(r64)
    ratios = {"grad_x": _ratio(r32["grad_x"], r64["grad_x"], T.ln_grad_x_floor(r64, gamma)),
              "grad_gamma": _ratio(r32["grad_gamma"], r64["grad_gamma"], fg),
              "grad_beta": _ratio(r32["grad_beta"], r64["grad_beta"], fb)}
    fl = T.sum_floors(r64, g, kind, d, q_m, t, T.ln_input_delta(r64, gamma, beta))
    for i, name in enumerate(("d", "q_m", "t")):
        ratios[name] = abs(float(r32["sums"][i]) - float(r64["sums"][i])) / fl[i]
    print(shape, kind, {k: f"{v:.3f}" for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("n", [4099, 1024 * 256 + 4099])
@pytest.mark.parametrize("params", T.QUANTIZERS, ids=_ids)
def test_gelu_float32_run_stays_below_the_floors(params, n):
    kind, d, q_m, t = params
    clip = CLIPS[1]
    h, g, _ = T.gelu_inputs(n, kind, d, q_m, t, clip)
    r64 = T.gelu_quant_backward_ref(h, g, kind, d, q_m, t, clip)
    r32 = T.gelu_quant_backward_ref(h, g, kind, d, q_m, t, clip, dtype=torch.float32)
    assert torch.equal(r32["masked"], r64["masked"])
    ratios = {"grad_h": _ratio(r32["grad_h"], r64["grad_h"], T.gelu_grad_h_floor(r64, h))}
    fl = T.sum_floors(r64, g, kind, d, q_m, t, T.gelu_input_delta(r64, h))
    for i, name in enumerate(("d", "q_m", "t")):
        ratios[name] = abs(float(r32["sums"][i]) - float(r64["sums"][i])) / fl[i]
    print(n, kind, {k: f"{v:.3f}" for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("params", T.QUANTIZERS, ids=_ids)
def test_at_least_nine_rows_in_ten_survive_the_filter(params, clip):
    """A condition of the GPU tests, not a tolerance: every parametrisation they draw keeps >= 90 % of its rows
    (LayerNorm) or elements (GELU)."""
    kind, d, q_m, t = params
    for rows, cols in T.LN_SHAPES:
        frac = T.ln_inputs(rows, cols, kind, d, q_m, t, clip)[4]
        assert frac >= 0.9, (rows, cols, frac)
    for n in T.GELU_SIZES[:-2] + [4 * 4099]:   # (the largest two draw the same distribution a hundredfold)
        frac = T.gelu_inputs(n, kind, d, q_m, t, clip)[2]
        assert frac >= 0.9, (n, frac)
