"""bn_act_pool (BatchNorm2d on batch statistics -> activation_quantize_fn -> MaxPool2d(2, 2) as one autograd node,
DESIGN.md section 18) against the three modules on the device, and UltraNetQua.train() with QVIT_ULTRA_TRAIN_FUSE on
and off."""
import copy

import pytest
import torch
import torch.nn as nn

import test_gpu_ultra_train as T
import ultra_backward_ref as R17
import ultra_bn_fuse_ref as R
from quantized_vit_amd import _lib, quant_ultra as Q
from quantized_vit_amd.ultranet import UltraNetQua, _aten_batch_norm

pytestmark = pytest.mark.gpu

EPS = float(torch.finfo(torch.float32).eps)
# Both routes evaluate y in fp32 within a few 2^-24 (|xhat gamma| + |y|) of the float64 value, under 1e-6 for the
# |y| < 3 of these inputs; ten times that keeps a tie-free bias findable for the 3200 values a channel of the largest
# case holds.
TIE_BAND = 1e-5
KERNELS = ("bn_stats", "bn_act_pool_forward", "bn_act_pool_backward")


class Calls:
    """Counts the calls of the new _lib wrappers."""

    def __enter__(self):
        self.n = {k: 0 for k in KERNELS}
        self.real = {k: getattr(_lib, k) for k in KERNELS}
        for k in KERNELS:
            setattr(_lib, k, self._wrap(k))
        return self

    def _wrap(self, k):
        def f(*a, **kw):
            self.n[k] += 1
            return self.real[k](*a, **kw)
        return f

    def __exit__(self, *exc):
        for k in KERNELS:
            setattr(_lib, k, self.real[k])


@pytest.fixture
def fuse_on(monkeypatch):
    monkeypatch.setattr(Q, "ULTRA_TRAIN_FUSE", "1")


def _tie_free_case(shape, a_bit, affine):
    """(x, gamma, beta) whose pre-quantizer values (float64) keep TIE_BAND from every rounding tie and clamp edge:
    the BN bias is moved channel by channel in steps of 1e-4 (as tests/test_gpu_ultra_train.py does); without an
    affine pair the seed is."""
    levels = 2 ** a_bit - 1
    for seed in range(64):
        x, gamma, beta = R.gen_case(shape, levels, affine, seed=1000 + seed)
        mean, var, invstd, _, _ = R.stats(x, 1e-5)
        xhat = (x.double() - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
        if not affine:
            if float(R17.tie_distance(xhat, float(levels)).min()) >= 1.25 * TIE_BAND:
                return x, None, None
            continue
        steps = torch.arange(2000, dtype=torch.float64) * 1e-4
        for c in range(x.shape[1]):
            v = xhat[:, c].reshape(1, -1) * float(gamma[c]) + float(beta[c])
            ok = (R17.tie_distance(v + steps[:, None], float(levels)).min(dim=1).values >= 1.25 * TIE_BAND).nonzero()
            assert ok.numel(), "no tie-free bias found"
            beta[c] += float(steps[int(ok[0])])
        return x, gamma, beta
    raise AssertionError("no tie-free seed found")


CONFIGS = [  # (B, C, H, W, pool), a_bit, momentum, affine, track_running_stats
    ((2, 3, 5, 7, True), 4, 0.1, True, True),
    ((2, 16, 40, 40, True), 4, None, True, True),
    ((3, 5, 4, 6, False), 2, 0.3, False, True),
    ((2, 4, 8, 8, False), 7, None, False, True),
    ((2, 4, 8, 8, True), 4, 0.1, True, False),
]


@pytest.mark.parametrize("shape,a_bit,momentum,affine,track", CONFIGS)
def test_bn_act_pool_equals_the_three_modules(dev, shape, a_bit, momentum, affine, track):
    levels = 2 ** a_bit - 1
    pool_on = shape[4]
    x, gamma, beta = _tie_free_case(shape, a_bit, affine)
    G = R.gen_grad(shape, 21)
    bn = nn.BatchNorm2d(shape[1], momentum=momentum, affine=affine, track_running_stats=track)
    if affine:
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
    if track:
        with torch.no_grad():
            bn.running_mean.normal_(generator=torch.Generator().manual_seed(1))
            bn.running_var.uniform_(0.5, 1.5, generator=torch.Generator().manual_seed(2))
    rm0 = bn.running_mean.clone() if track else None
    rv0 = bn.running_var.clone() if track else None
    bn_m, bn_f = copy.deepcopy(bn).to(dev).train(), copy.deepcopy(bn).to(dev).train()
    act, pool = Q.activation_quantize_fn(a_bit), (nn.MaxPool2d(2, 2) if pool_on else None)

    xm = x.to(dev).requires_grad_(True)
    with _aten_batch_norm():
        ym = act(bn_m(xm))
        ym = pool(ym) if pool_on else ym
    ym.backward(G.to(dev))
    xf = x.to(dev).requires_grad_(True)
    with Calls() as calls:
        for step in range(2):   # two steps: the cumulative average moves with num_batches_tracked
            yf = Q.bn_act_pool(xf if step == 0 else xf.detach(), bn_f, act, pool)
            if step == 0:
                assert yf is not None and torch.equal(yf, ym)
                saved = yf.grad_fn.saved_tensors
                yf.backward(G.to(dev))
    assert calls.n == {"bn_stats": 2, "bn_act_pool_forward": 2, "bn_act_pool_backward": 1}
    with _aten_batch_norm():
        bn_m(xm.detach())

    # what the node keeps: x, mean, invstd, one flag byte per output, gamma; no full-size float beside x, no int64
    assert [t.dtype for t in saved[:4]] == [torch.float32, torch.float32, torch.float32, torch.uint8]
    assert saved[0].shape == xf.shape and saved[3].shape == yf.shape and saved[1].shape == (shape[1],)
    assert len(saved) == 5 and (saved[4] is None) == (not affine)
    assert all(t is None or t.dtype != torch.int64 for t in saved)

    out64, dx64, dg64, db64 = R.autograd_truth(x, gamma, beta, 1e-5, levels, pool_on, G)
    assert torch.equal(torch.round(yf.detach().cpu() * levels).double(), torch.round(out64 * levels))
    mean32, _, invstd32, _, _ = R.stats(x, 1e-5, dtype=torch.float32)
    flags = R.forward(x, *R.stats(x, 1e-5)[0:3:2], gamma, beta, levels, pool_on)[1]
    r32 = R.backward(x, G, flags, mean32, invstd32, gamma, pool_on, dtype=torch.float32)
    scale = R.dx_scale(G, invstd32, gamma)
    figures = [("input", xf.grad, xm.grad, dx64, r32[0], scale)]
    if affine:
        figures += [("gamma", bn_f.weight.grad, bn_m.weight.grad, dg64, r32[1], 0.0),
                    ("beta", bn_f.bias.grad, bn_m.bias.grad, db64, r32[2], 0.0)]
    for name, got, mod, ref, ref32, sc in figures:
        err, errm, err32 = R.rel(got, ref, sc), R.rel(mod, ref, sc), R.rel(ref32, ref, sc)
        print(f"{shape} a_bit {a_bit} {name}.grad: fused err {err:.3e}, modules err {errm:.3e}, fp32 CPU err "
              f"{err32:.3e}, ratio {err / max(err32, EPS):.3f}")
        assert err <= R.C_MODULE * max(err32, EPS), (name, err, err32)
    if track:
        assert int(bn_f.num_batches_tracked) == int(bn_m.num_batches_tracked) == 2
        f = [1.0, 0.5] if momentum is None else [momentum] * 2
        rm64, rv64 = R.stats(x, 1e-5, f[1], *R.stats(x, 1e-5, f[0], rm0, rv0)[3:])[3:]
        rm32, rv32 = R.stats(x, 1e-5, f[1], *R.stats(x, 1e-5, f[0], rm0, rv0, dtype=torch.float32)[3:],
                             dtype=torch.float32)[3:]
        for name, got, mod, ref, ref32 in (("running_mean", bn_f.running_mean, bn_m.running_mean, rm64, rm32),
                                           ("running_var", bn_f.running_var, bn_m.running_var, rv64, rv32)):
            err, errm, err32 = R.rel(got, ref), R.rel(mod, ref), R.rel(ref32, ref)
            print(f"{shape} {name}: fused err {err:.3e}, modules err {errm:.3e}, fp32 CPU err {err32:.3e}")
            assert err <= R.C_STATS * max(err32, EPS), (name, err, err32)
    else:
        assert bn_f.running_mean is None and bn_f.num_batches_tracked is None


def test_bn_act_pool_declines_what_does_not_fit(dev):
    x = torch.rand(2, 4, 6, 6, device=dev)
    bn, act = nn.BatchNorm2d(4).to(dev).train(), Q.activation_quantize_fn(4)
    with Calls() as calls:
        assert Q.bn_act_pool(x, copy.deepcopy(bn).eval(), act) is None           # eval BN on running statistics
        assert Q.bn_act_pool(x, bn, Q.activation_quantize_fn(8)) is None
        assert Q.bn_act_pool(x, bn, Q.activation_quantize_fn(32)) is None
        assert Q.bn_act_pool(x.double(), bn, act) is None
        assert Q.bn_act_pool(x[0], bn, act) is None
        assert Q.bn_act_pool(x, nn.BatchNorm2d(5).to(dev), act) is None
        assert Q.bn_act_pool(x, Q.batchNorm2d_Q_fn(4)(4).to(dev), act) is None
        for p in (nn.MaxPool2d(3, 2), nn.MaxPool2d(2, 1), nn.MaxPool2d(2, 2, padding=1), nn.MaxPool2d(2, 2, dilation=2),
                  nn.MaxPool2d(2, 2, ceil_mode=True), nn.MaxPool2d(2, 2, return_indices=True), nn.AvgPool2d(2, 2)):
            assert Q.bn_act_pool(x, bn, act, p) is None, p
        assert int(bn.num_batches_tracked) == 0
        with pytest.raises(ValueError, match="Expected more than 1 value per channel when training, got input size "
                                             r"torch.Size\(\[1, 4, 1, 1\]\)"):
            Q.bn_act_pool(x[:1, :, :1, :1], bn, act)
        assert calls.n == {k: 0 for k in KERNELS}
        # an eval-mode BatchNorm2d without running statistics normalises on the batch: it fits
        free = nn.BatchNorm2d(4, track_running_stats=False).to(dev).eval()
        y = Q.bn_act_pool(x, free, act, nn.MaxPool2d((2, 2), (2, 2)))
        assert y is not None and y.shape == (2, 4, 3, 3)
        assert calls.n["bn_act_pool_forward"] == 1


# ---- the network ------------------------------------------------------------------------------------------------
def _model_and_input(dev):
    torch.manual_seed(0)
    model = UltraNetQua().train()
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    pre = T._clear_of_ties(model, x)
    assert min(float(R17.tie_distance(v, 15.0).min()) for v in pre) >= T.TIE_BAND
    state = {k: v.clone() for k, v in model.state_dict().items()}
    return model.to(dev), x, state


def test_ultranet_trains_on_the_fused_route(dev, fuse_on):
    model, x, state = _model_and_input(dev)
    with Calls() as calls:
        grads, p = T._grads(model, x.to(dev), "hip")
    # each of the 8 blocks took the fused node exactly once, forward and backward
    assert calls.n == {"bn_stats": 8, "bn_act_pool_forward": 8, "bn_act_pool_backward": 8}
    g32, p32 = T._restatement(state, x, dev, torch.float32)
    g64, p64 = T._restatement(state, x, "cpu", torch.float64)
    perr, perr32 = T._rel(p, p64), T._rel(p32, p64)
    print(f"p (fused): err {perr:.3e}, fp32 restatement err {perr32:.3e}")
    assert perr <= R17.C_NET * max(perr32, EPS)
    for k in g64:
        g = grads[k]
        assert bool(torch.isfinite(g).all()) and bool((g != 0).any()), k
        err, err32 = T._rel(g, g64[k]), T._rel(g32[k], g64[k])
        print(f"{k} (fused): err {err:.3e}, fp32 restatement err {err32:.3e}, ratio {err / max(err32, EPS):.3f}")
        assert err <= R17.C_NET * max(err32, EPS), (k, err, err32)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            assert int(m.num_batches_tracked) == 1


def _module_walk(model, x):
    """The parent route of forward_modules in training mode, module by module."""
    with _aten_batch_norm():
        h = x
        for m in model.layers:
            h = m(h)
    return model.yololayer(h, x.shape[-2:])


def test_flag_off_is_the_parent_route(dev):
    assert Q.ULTRA_TRAIN_FUSE == "0" or Q.ULTRA_TRAIN_FUSE == "1"
    prev, Q.ULTRA_TRAIN_FUSE = Q.ULTRA_TRAIN_FUSE, "0"
    try:
        model, x, state = _model_and_input(dev)
        twin = copy.deepcopy(model)
        with Calls() as calls:
            out = model(x.to(dev))
            out[0].square().mean().backward()
        assert calls.n == {k: 0 for k in KERNELS}
        want = _module_walk(twin, x.to(dev))
        assert torch.equal(out[0].detach(), want.detach())
        for (k, a), (_, b) in zip(model.state_dict().items(), twin.state_dict().items()):
            assert torch.equal(a, b), k
    finally:
        Q.ULTRA_TRAIN_FUSE = prev


def test_hooked_batchnorm_keeps_the_module_route(dev, fuse_on):
    model, x, _ = _model_and_input(dev)
    seen = []
    bn = model.layers[5]
    assert isinstance(bn, nn.BatchNorm2d)
    handle = bn.register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
    try:
        with Calls() as calls:
            out = model(x.to(dev))
            out[0].square().mean().backward()
    finally:
        handle.remove()
    assert len(seen) == 1
    assert calls.n == {"bn_stats": 7, "bn_act_pool_forward": 7, "bn_act_pool_backward": 7}
    # no grad mode: the flag routes nothing
    with Calls() as calls, torch.no_grad():
        model(x.to(dev))
    assert calls.n == {k: 0 for k in KERNELS}
