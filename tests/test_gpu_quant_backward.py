"""qvit_quant_backward on the device against the float64 restatement of the reference's backwards
(tests/quant_backward_ref.py), on tie-free inputs, plus the quantizer autograd Functions built on it.

Sums: |got - ref64| <= 4 max(|ref32 - ref64|, floor), floor = 2^-23 sum |g_i| (1 + |q_i|) c_i from the float64
restatement (one rounding in q, one in the product; nonlinear c_i = 4 (1 + |t ln a_i|) for the exp / log); the
factor 4 covers the summation order and the device's exp / log. tests/test_quant_backward_cpu.py shows the
reference's own float32 run stays below 0.14 floor."""
import pytest
import torch

import quant_backward_ref as R
from quant_backward_ref import CLIPS, PARAM_SETS, SIZES

pytestmark = pytest.mark.gpu

QT = {R.LINEAR: 0, R.NONLINEAR: 1}
# past the grid cap (1024 blocks x 256 threads x 4 floats): the second 16-byte pair of each lane, and past twice
# the cap: a second trip of the grid-stride loop
ALL_SIZES = SIZES + [2 * 1024 * 256 * 4 + 4099]
_ids = lambda p: f"{p[0]}-qm{p[2]}-t{p[3]}"


def _dev_params(dev, d, q_m, t):
    f = lambda v: None if v is None else torch.tensor([v], dtype=torch.float32, device=dev)
    return f(d), f(q_m), f(t)


def _run(dev, x, g, kind, d, q_m, t, clip, dge_k=0.0, qflag=0, grad_x=None):
    from quantized_vit_amd import _lib
    dd, dq, dt = _dev_params(dev, d, q_m, t)
    return _lib.quant_backward(x, g, QT[kind] | qflag, dd, dq, dt, clip[0], clip[1], dge_k, grad_x=grad_x)


@pytest.mark.parametrize("n", ALL_SIZES)
@pytest.mark.parametrize("params", PARAM_SETS, ids=_ids)
def test_grad_x_and_sums(dev, params, n):
    kind, d, q_m, t = params
    clip = CLIPS[0]
    x, g = R.make_inputs(n, kind, d, q_m, t, clip)
    r64, r32, floor, bounds = R.sum_bounds(x, g, kind, d, q_m, t, clip)
    gx, scal = _run(dev, x.to(dev), g.to(dev), kind, d, q_m, t, clip)
    assert torch.equal(gx.cpu(), r64["grad_x"].float())   # a masked copy: exact
    got = scal.cpu().double().tolist()
    for i, name in enumerate(("d", "q_m", "t")):
        err = abs(got[i] - float(r64["sums"][i]))
        print(f"n={n} grad_{name}: got {got[i]:+.6e} ref64 {float(r64['sums'][i]):+.6e} err {err:.3e} "
              f"|ref32-ref64| {abs(float(r32['sums'][i]) - float(r64['sums'][i])):.3e} floor {floor:.3e}")
        assert err <= bounds[i], (name, err, bounds[i])
    if kind == R.LINEAR:
        assert got[2] == 0.0


@pytest.mark.parametrize("params", PARAM_SETS, ids=_ids)
def test_clip_mask_through_the_interior(dev, params):
    kind, d, q_m, t = params
    clip, n = CLIPS[1], 4099
    x, g = R.make_inputs(n, kind, d, q_m, t, clip)
    r64, _, _, bounds = R.sum_bounds(x, g, kind, d, q_m, t, clip)
    gx, scal = _run(dev, x.to(dev), g.to(dev), kind, d, q_m, t, clip)
    ref_gx = r64["grad_x"].float()
    assert 0 < int((ref_gx == 0).sum()) < n
    assert torch.equal(gx.cpu(), ref_gx)
    for i in range(3):
        assert abs(float(scal[i]) - float(r64["sums"][i])) <= bounds[i]


@pytest.mark.parametrize("n", [1, 65, 4099, 1024 * 256 * 4 + 4099])
def test_dge_grad_x(dev, n):
    kind, d, q_m, t = PARAM_SETS[0]
    clip = CLIPS[0]
    x, g = R.make_inputs(n, kind, d, q_m, t, clip)
    for k in (5.0, 2.5):   # num_bits 4 and 8 (quant_layers.py:236)
        r64 = R.quant_backward_ref(x, g, kind, d, q_m, t, clip, dge_k=k)
        gx, scal = _run(dev, x.to(dev), g.to(dev), kind, d, q_m, t, clip, dge_k=k)
        assert torch.allclose(gx.cpu(), r64["grad_x"].float())
        assert float(gx.abs().max()) <= 3.0
        # the scalar sums do not depend on k
        _, scal0 = _run(dev, x.to(dev), g.to(dev), kind, d, q_m, t, clip)
        assert torch.equal(scal, scal0)


def test_dge_known_answer_through_the_function(dev):
    """The reference's test_dge_quantizer (tests/quantization/test_quant_layers.py:80-112) on the device."""
    from quantized_vit_amd.quant_layers import DGEQuantizer
    x = torch.tensor([0.3], device=dev, requires_grad=True)
    d = torch.tensor([0.2], device=dev, requires_grad=True)
    q_m = torch.tensor([1.0], device=dev, requires_grad=True)
    clip = torch.tensor([-1.0, 1.0], device=dev)
    out = DGEQuantizer.apply(x, d, q_m, clip, torch.tensor([0.0], device=dev), torch.tensor([4.0], device=dev))
    assert torch.allclose(out, d * torch.round(x / d))
    out.backward()
    k = 5.0
    assert torch.allclose(x.grad, (1 / k) * torch.pow(torch.abs(x.detach() - d.detach() / 2), 1 / k - 1))
    assert d.grad is not None and d.grad.shape == (1,) and q_m.grad is not None and q_m.grad.shape == (1,)


@pytest.mark.parametrize("params", [PARAM_SETS[0], PARAM_SETS[4]], ids=_ids)
def test_deterministic_and_aliased(dev, params):
    kind, d, q_m, t = params
    clip, n = CLIPS[0], 1024 * 256 * 4 + 4099
    x, g = R.make_inputs(n, kind, d, q_m, t, clip)
    xd, gd = x.to(dev), g.to(dev)
    gx1, s1 = _run(dev, xd, gd, kind, d, q_m, t, clip)
    gx2, s2 = _run(dev, xd, gd, kind, d, q_m, t, clip)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    assert torch.equal(gx1, gx2)
    alias = gd.clone()
    gx3, s3 = _run(dev, xd, alias, kind, d, q_m, t, clip, grad_x=alias)
    assert gx3.data_ptr() == alias.data_ptr()
    assert torch.equal(gx3, gx1) and torch.equal(s3.view(torch.int32), s1.view(torch.int32))


def test_empty_input_writes_zeros(dev):
    from quantized_vit_amd import _lib
    lib = _lib.load()
    d, q_m, _ = _dev_params(dev, 0.05, 0.37, None)
    buf = torch.zeros(4, device=dev)
    scal = torch.full((3,), 7.0, device=dev)
    ws = torch.empty(lib.qvit_quant_backward_workspace_bytes(0) // 8, dtype=torch.float64, device=dev)
    rc = lib.qvit_quant_backward(buf.data_ptr(), buf.data_ptr(), 0, 0, d.data_ptr(), q_m.data_ptr(), None, -2.0, 2.0,
                                 0.0, buf.data_ptr(), scal.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                 torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    assert scal.cpu().tolist() == [0.0, 0.0, 0.0]


def _apply(kind, x, d, q_m, t, clip):
    from quantized_vit_amd.quant_layers import SymQuantizerLinear, SymQuantizerNonLinear
    if kind == R.LINEAR:
        return SymQuantizerLinear.apply(x, d, q_m, clip, 0.0)
    return SymQuantizerNonLinear.apply(x, d, q_m, t, clip, 0.0)


@pytest.mark.parametrize("params", [PARAM_SETS[0], PARAM_SETS[2]], ids=_ids)
def test_functions_match_the_restatement(dev, params):
    """The reference's apply signatures and gradient tuples: forward = qvit_fake_quant_f32, scalar grads [1]."""
    from quantized_vit_amd import _lib
    from quantized_vit_amd.quant_layers import QuantizationType, _get_quantizer
    kind, d, q_m, t = params
    clip, n = CLIPS[0], 4099
    x, g = R.make_inputs(n, kind, d, q_m, t, clip)
    r64, _, _, bounds = R.sum_bounds(x, g, kind, d, q_m, t, clip)
    xd = x.to(dev).requires_grad_(True)
    ps = [None if p is None else p.requires_grad_(True) for p in _dev_params(dev, d, q_m, t)]
    y = _apply(kind, xd, ps[0], ps[1], ps[2], torch.tensor(clip, device=dev))
    assert y.grad_fn is not None
    assert torch.equal(y.detach(), _lib.fake_quant_f32(x.to(dev), QT[kind], *[None if p is None else p.detach()
                                                                               for p in ps]))
    assert torch.equal(y.detach().cpu(), R.quant_forward_ref(x, kind, d, q_m, t).float())
    y.backward(g.to(dev))
    assert torch.equal(xd.grad.cpu(), r64["grad_x"].float())
    for i, p in enumerate(ps):
        if p is not None:
            assert p.grad.shape == (1,)
            assert abs(float(p.grad) - float(r64["sums"][i])) <= bounds[i]
    qt = QuantizationType.SYMMETRIC_LINEAR if kind == R.LINEAR else QuantizationType.SYMMETRIC_NONLINEAR
    assert _get_quantizer(qt).__name__ == ("SymQuantizerLinear" if kind == R.LINEAR else "SymQuantizerNonLinear")
    assert _get_quantizer(QuantizationType.DGE).__name__ == "DGEQuantizer"


@pytest.mark.parametrize("params", [PARAM_SETS[0], PARAM_SETS[2]], ids=_ids)
def test_nan_in_grad_out_raises(dev, params):
    from quantized_vit_amd.quant_layers import NanInGradientError
    kind, d, q_m, t = params
    clip, n = CLIPS[0], 1023
    x, g = R.make_inputs(n, kind, d, q_m, t, clip)
    interior = int(torch.nonzero((x.abs() > 0) & (x.abs() < q_m))[0])
    g = g.clone()
    g[interior] = float("nan")
    xd = x.to(dev).requires_grad_(True)
    ps = [None if p is None else p.requires_grad_(True) for p in _dev_params(dev, d, q_m, t)]
    y = _apply(kind, xd, ps[0], ps[1], ps[2], clip)
    with pytest.raises(NanInGradientError) as e:
        y.backward(g.to(dev))
    assert "grad_d" in str(e.value) and "q_m" in str(e.value)


def test_dge_nan_in_grad_x_raises(dev):
    from quantized_vit_amd.quant_layers import DGEQuantizer, NanInGradientError
    x = torch.tensor([0.3, 0.1], device=dev, requires_grad=True)   # x = d / 2: 0^(1/k - 1) = inf, times 0
    d, q_m = torch.tensor([0.2], device=dev), torch.tensor([1.0], device=dev)
    out = DGEQuantizer.apply(x, d, q_m, (-1.0, 1.0), 0.0, 4.0)
    with pytest.raises(NanInGradientError):
        out.backward(torch.tensor([1.0, 0.0], device=dev))


def test_zero_input_does_not_raise(dev):
    """x = 0 under the nonlinear quantizer: 0 * -inf is computed and masked; finite grad_out, finite sums."""
    kind, d, q_m, t = PARAM_SETS[2]
    x = torch.tensor([0.0, -0.0, 0.11, 0.0, 0.5], device=dev, requires_grad=True)
    ps = [p.requires_grad_(True) for p in _dev_params(dev, d, q_m, t)]
    y = _apply(kind, x, ps[0], ps[1], ps[2], CLIPS[0])
    y.backward(torch.tensor([1.0, -2.0, 0.5, 3.0, 0.25], device=dev))
    assert all(bool(torch.isfinite(p.grad).all()) for p in ps)
    assert torch.equal(x.grad.cpu(), torch.tensor([1.0, -2.0, 0.5, 3.0, 0.25]))


@pytest.mark.parametrize("params", PARAM_SETS, ids=_ids)
def test_backward_uses_the_forward_codes(dev, params):
    """With one element and grad_out = 1 the d sum is sgn (rne(q) - q): the code it rounds to must be the
    forward's (fake_quant_f32 / d), also just beside rounding ties, where a re-derived quotient could round the
    other way. QVIT_QT_FORCE_CAREFUL (the careful path on every element) gives identical scalars."""
    from quantized_vit_amd import _lib
    kind, d, q_m, t = params
    clip = CLIPS[0]
    dd, dq, dt = _dev_params(dev, d, q_m, t)
    tp = 1.0 if t is None else t
    ties = [(d * (k + 0.5)) ** (1.0 / tp) for k in (0, 1, 2, 4)]
    xs = [v * s * (1.0 + e) for v in ties for s in (1.0, -1.0) for e in (0.0, 2e-7, -2e-7)]
    xs += R.make_inputs(63, kind, d, q_m, t, clip)[0][:8].tolist()
    x = torch.tensor(xs, dtype=torch.float32, device=dev)
    codes = (_lib.fake_quant_f32(x, QT[kind], dd, dq, dt) / dd).round().cpu()
    one = torch.ones(1, device=dev)
    ref = R.quant_backward_ref(x.cpu(), torch.ones(len(xs)), kind, d, q_m, t, clip)
    for i in range(len(xs)):
        _, s = _lib.quant_backward(x[i:i + 1].clone(), one, QT[kind], dd, dq, dt, clip[0], clip[1])
        sgn = 1.0 if xs[i] > 0 else -1.0
        # rne(q) = sgn * term_d + q, with q from float64: off by the rounding of q only (<< 0.5)
        rne = sgn * float(s[0]) + float(ref["q"][i])
        assert abs(rne - abs(float(codes[i]))) < 1e-3, (xs[i], rne, float(codes[i]))
    n = 4099
    xb, gb = R.make_inputs(n, kind, d, q_m, t, clip)
    xb = torch.cat([xb, x.cpu()])
    gb = torch.cat([gb, torch.ones(len(xs))])
    gx0, s0 = _lib.quant_backward(xb.to(dev), gb.to(dev), QT[kind], dd, dq, dt, clip[0], clip[1])
    gx1, s1 = _lib.quant_backward(xb.to(dev), gb.to(dev), QT[kind] | _lib.QT_FORCE_CAREFUL, dd, dq, dt, clip[0],
                                  clip[1])
    assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and torch.equal(gx0, gx1)
