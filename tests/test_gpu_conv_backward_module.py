"""The backward GEMMs of QuantizeConv2d on the HIP kernels (quant_layers.CONV_BACKWARD_GEMM): wgrad as
qvit_gemm_wgrad on the recomputed im2col codes, dgrad as qvit_gemm_wonly on the transposed weight codes followed by
qvit_col2im_quant_backward. Route selection by call counting, the module's gradients on the forced HIP route against
the float64 CPU graph of tests/test_gpu_layer_autograd.py with its bounds, exactness on integers, the forward's bits,
and a tiny ViT whose two routes must agree to summation-order rounding."""
import pytest
import torch

import quant_backward_ref as R
import test_gpu_layer_autograd as T

pytestmark = pytest.mark.gpu

# (kernel, stride, padding, dilation, input shape), 3 -> 8 channels, as test_gpu_layer_autograd's geometries
CONV_PATCH = (4, 4, 0, 1, (2, 3, 16, 20))          # the patch-embedding class: k == s, p == 0 (the 16-byte arm)
GEOMS = {"patch": CONV_PATCH, "asym": T.CONV_ASYM, "asym-unread-row": T.CONV_ASYM_UNREAD_ROW, "3x3": T.CONV_SQUARE}


def _route(monkeypatch, route):
    from quantized_vit_amd import quant_layers as ql
    monkeypatch.setattr(ql, "CONV_BACKWARD_GEMM", route)


def _spy(monkeypatch, obj, name):
    calls = []
    orig = getattr(obj, name)

    def wrapped(*a, **k):
        calls.append(name)
        return orig(*a, **k)
    monkeypatch.setattr(obj, name, wrapped)
    return calls


def _spies(monkeypatch):
    """Call lists of (gemm_wonly, gemm_wgrad, col2im_quant_backward, quant_backward, conv2d_input, conv2d_weight)."""
    from quantized_vit_amd import _lib
    return tuple(_spy(monkeypatch, obj, name) for obj, name in (
        (_lib, "gemm_wonly"), (_lib, "gemm_wgrad"), (_lib, "col2im_quant_backward"), (_lib, "quant_backward"),
        (torch.nn.grad, "conv2d_input"), (torch.nn.grad, "conv2d_weight")))


def _backward_calls(dev, monkeypatch, route, path="int", geom=CONV_PATCH, freeze=(), input_grad=True, make=None):
    _route(monkeypatch, route)
    if make is None:
        layer, x, *_ = T._build(dev, R.LINEAR, path, conv=True, geom=geom)
    else:
        layer, x = make()
    for name in freeze:
        getattr(layer, name).requires_grad_(False)
    spies = _spies(monkeypatch)
    xd = x.to(dev).requires_grad_(input_grad)
    y = layer(xd)
    for s in spies:
        del s[:]
    y.sum().backward()
    if input_grad:
        assert xd.grad is not None and bool(torch.isfinite(xd.grad).all())
    return tuple(len(s) for s in spies), layer


# ---- route selection --------------------------------------------------------------------------------------------
def test_hip_route_runs_the_kernels(dev, monkeypatch):
    """Fails without the feature: there is no _lib.col2im_quant_backward and no conv route."""
    for geom in (CONV_PATCH, T.CONV_SQUARE):     # forced: also where taps overlap
        calls, layer = _backward_calls(dev, monkeypatch, "hip", geom=geom)
        # dgrad GEMM, wgrad GEMM, fold + activation quantizer; quant_backward for the weight alone; no library conv
        assert calls == (1, 1, 1, 1, 0, 0), (geom, calls)
        assert layer.weight.grad is not None and layer.d_quant_act.grad is not None


def test_torch_route_is_the_library(dev, monkeypatch):
    assert _backward_calls(dev, monkeypatch, "torch")[0] == (0, 0, 0, 2, 1, 1)


def test_single_op_routes(dev, monkeypatch):
    assert _backward_calls(dev, monkeypatch, "dgrad")[0] == (1, 0, 1, 1, 0, 1)
    assert _backward_calls(dev, monkeypatch, "wgrad")[0] == (0, 1, 0, 2, 1, 0)


def test_default_route(dev, monkeypatch):
    """Unset: both ops on the kernels where no two taps reach one input element (the patch embedding, where both
    were measured faster), both on the library where taps overlap (the 3 x 3 stride-1 layer measured slower on both):
    DESIGN.md section 21."""
    assert _backward_calls(dev, monkeypatch, None, geom=CONV_PATCH)[0] == (1, 1, 1, 1, 0, 0)
    assert _backward_calls(dev, monkeypatch, None, geom=T.CONV_SQUARE)[0] == (0, 0, 0, 2, 1, 1)


def test_unknown_route_is_an_error(dev, monkeypatch):
    with pytest.raises(ValueError):
        _backward_calls(dev, monkeypatch, "miopen")
    with pytest.raises(ValueError):          # the unset state has no name
        _backward_calls(dev, monkeypatch, "auto")


def test_weight_only_layer_runs_dgrad_alone(dev, monkeypatch):
    calls, _ = _backward_calls(dev, monkeypatch, "hip", path="wonly")
    assert calls == (1, 0, 1, 1, 0, 1)          # fold only (no activation quantizer), wgrad on the library


def test_frozen_weight_skips_wgrad(dev, monkeypatch):
    calls, layer = _backward_calls(dev, monkeypatch, "hip", freeze=("weight", "d_quant_wt", "q_m_wt"))
    assert calls == (1, 0, 1, 0, 0, 0)
    assert layer.weight.grad is None and layer.bias.grad is not None


def test_frozen_activation_scalars_and_plain_input_skip_dgrad(dev, monkeypatch):
    calls, layer = _backward_calls(dev, monkeypatch, "hip", freeze=("d_quant_act", "q_m_act"), input_grad=False)
    assert calls == (0, 1, 0, 1, 0, 0)
    assert layer.weight.grad is not None and layer.d_quant_act.grad is None


def test_ineligible_layers_stay_on_the_library(dev, monkeypatch):
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeConv2d

    def grouped():
        conv = torch.nn.Conv2d(4, 8, 3, padding=1, groups=2)
        return conv, torch.randn(2, 4, 8, 8)

    def same():
        conv = torch.nn.Conv2d(3, 8, 3, padding="same")
        return conv, torch.randn(2, 3, 8, 8)

    for make in (grouped, same):
        def build():
            torch.manual_seed(0)
            conv, x = make()
            q = QuantizeConv2d.from_module(conv, quant_type=QuantizationType.SYMMETRIC_LINEAR,
                                           quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION, num_bits=4)
            return q.to(dev).eval(), x
        calls, _ = _backward_calls(dev, monkeypatch, "hip", make=build)
        assert calls[:3] == (0, 0, 0) and calls[3] == 2, (make.__name__, calls)


# ---- gradients against the float64 graph ----------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["int", "wonly"])
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("kind", [R.LINEAR, R.NONLINEAR])
def test_hip_route_matches_float64(dev, monkeypatch, kind, geom, path):
    """T._check_layer on the forced HIP route: weight within 4 rows 2^-24 conv2d_weight(|x_q|, |G|), input within
    4 N kh kw 2^-24 conv2d_input(|w_q|, |G|), the quantizer scalars within sum_bounds, an unread row exactly zero, the
    forward bit for bit."""
    _route(monkeypatch, "hip")
    spies = _spies(monkeypatch)
    assert T._unread_rows_cols(GEOMS["asym-unread-row"]) == [[8], []]
    T._check_layer(dev, kind, path, conv=True, geom=GEOMS[geom])
    # the fold ran once, wgrad on the integer path only (torch.nn.grad is not counted here: _check_layer itself
    # calls both functions on the CPU for its bounds)
    assert len(spies[0]) == 1 and len(spies[2]) == 1 and len(spies[1]) == (1 if path == "int" else 0)


# ---- exact on integers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["patch", "3x3", "asym"])
def test_exact_on_integers(dev, geom):
    """Integer G in [-8, 8], weight codes in [-7, 7] at d_wt = 2^-4, activation codes in [-60, 60] at d_act = 2^-5 (x =
    d_act code, inside the clip range): every product and partial sum is an integer below 2^24 times a power of two
    (wgrad: 8 * 60 * 128 rows; dgrad: 8 * 7 * 8 channels, at most 9 taps), so both results equal the float64 ones."""
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeConv2d
    k, s, p, dil, xshape = GEOMS[geom]
    d_wt, d_act = 2.0 ** -4, 2.0 ** -5
    layer = QuantizeConv2d(3, 8, k, stride=s, padding=p, dilation=dil, bias=False,
                           quant_type=QuantizationType.SYMMETRIC_LINEAR,
                           quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION).to(dev).eval()
    for name, v in (("d_quant_wt", d_wt), ("q_m_wt", 7 * d_wt), ("d_quant_act", d_act), ("q_m_act", 127 * d_act)):
        getattr(layer, name).data.fill_(v)
    gen = torch.Generator().manual_seed(5)
    wcodes = torch.randint(-7, 8, tuple(layer.weight.shape), generator=gen).float()
    layer.weight.data.copy_(wcodes * d_wt)
    layer.invalidate()
    layer.load_weight_codes(wcodes)
    plan = layer.quant_plan()
    assert plan.int_path and abs(plan.level_wt) == 7 and abs(plan.level_act) == 127
    xcodes = torch.randint(-60, 61, xshape, generator=gen).float()
    x = xcodes * d_act
    with torch.no_grad():
        yshape = layer(x.to(dev)).shape
    G = torch.randint(-8, 9, tuple(yshape), generator=gen).float()
    gx, gw, scal = layer._gemm_grads_hip(plan, x.to(dev), None, None, G.to(dev), True, True)
    want_x = torch.nn.grad.conv2d_input(xshape, (wcodes * d_wt).double(), G.double(), s, p, dil)
    want_w = torch.nn.grad.conv2d_weight(x.double(), tuple(wcodes.shape), G.double(), s, p, dil)
    assert gw.shape == layer.weight.shape and torch.equal(gw.cpu().double(), want_w)
    assert torch.equal(gx.cpu().double(), want_x)      # |x| < 2: the clip passes every element
    assert scal.shape == (3,)


# ---- the forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["hip", "torch"])
def test_forward_unchanged(dev, monkeypatch, route):
    _route(monkeypatch, route)
    layer, x, *_ = T._build(dev, R.NONLINEAR, "int", conv=True, geom=CONV_PATCH)
    with torch.no_grad():
        y0 = layer(x.to(dev))
    y = layer(x.to(dev).requires_grad_(True))
    assert y.grad_fn is not None and torch.equal(y.detach(), y0)


def test_channels_last_gradient_is_not_copied(dev, monkeypatch):
    """Behind PatchEmbed's flatten + transpose the incoming gradient is channels-last: the row view G2 the kernels
    read is that memory itself."""
    from quantized_vit_amd import _lib
    _route(monkeypatch, "hip")
    layer, x, *_ = T._build(dev, R.LINEAR, "int", conv=True, geom=CONV_PATCH)
    seen = []
    orig = _lib.gemm_wgrad
    monkeypatch.setattr(_lib, "gemm_wgrad", lambda G2, *a, **k: (seen.append(G2.data_ptr()), orig(G2, *a, **k))[1])
    y = layer(x.to(dev).requires_grad_(True))
    g = torch.randn(y.shape[0], y.shape[2] * y.shape[3], y.shape[1], device=dev)       # [B, tokens, N] rows
    y.flatten(2).transpose(1, 2).backward(g)
    assert seen == [g.data_ptr()]


def test_nan_grad_raises_through_the_conv_route(dev, monkeypatch):
    from quantized_vit_amd.quant_layers import NanInGradientError
    _route(monkeypatch, "hip")
    layer, x, *_ = T._build(dev, R.LINEAR, "int", conv=True, geom=CONV_PATCH)
    for p in (layer.weight, layer.d_quant_wt, layer.q_m_wt):     # the activation quantizer's check alone
        p.requires_grad_(False)
    y = layer(x.to(dev).requires_grad_(True))
    g = torch.ones_like(y)
    g[1, 2, 1, 3] = float("nan")
    with pytest.raises(NanInGradientError):
        y.backward(g)


# ---- output gradients that are not row-major rows -------------------------------------------------------------------
# With out_channels a multiple of 128 (every ViT patch embedding: 768 / 1024 / 1280) dgrad hands the [M, N] row view
# of the output gradient to qvit_gemm_wonly without a padded copy, so the view's own strides reach the kernel.
N128 = 128
GRADS = ["expanded", "inner-stride-2", "channels-last", "nchw"]


def _build128(dev):
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeConv2d
    kind = R.LINEAR
    _, wq, aq = T._case(kind, "int")
    k, s, p, dil, xshape = CONV_PATCH
    layer = QuantizeConv2d(3, N128, k, stride=s, padding=p, dilation=dil, bias=True,
                           quant_type=QuantizationType.SYMMETRIC_LINEAR,
                           quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION).to(dev).eval()
    layer.weight.data.copy_(R.tie_free_values(tuple(layer.weight.shape), kind, *wq, seed=10))
    layer.bias.data.zero_()
    for name, v in zip(("d_quant_wt", "q_m_wt", "d_quant_act", "q_m_act"), wq[:2] + aq[:2]):
        getattr(layer, name).data.fill_(v)
    layer.invalidate()
    assert layer.quant_plan().int_path
    return layer, R.tie_free_values(xshape, kind, *aq, seed=30), aq


def _grad_view(kind, yshape, dev):
    """(gradient tensor handed to backward, the same values as a dense CPU tensor)."""
    B, N, OH, OW = yshape
    gen = torch.Generator().manual_seed(77)
    if kind == "expanded":                       # what sum().backward() produces: one element, every stride 0
        g = torch.ones((), device=dev).expand(yshape)
        assert g.stride() == (0, 0, 0, 0)
    elif kind == "inner-stride-2":               # channels-last rows whose channel stride is 2
        big = torch.randn(B, OH, OW, N, 2, generator=gen).to(dev)
        g = big[..., 0].permute(0, 3, 1, 2)
        assert g.stride(1) == 2
    elif kind == "channels-last":
        g = torch.randn(B, OH, OW, N, generator=gen).to(dev).permute(0, 3, 1, 2)
    else:
        g = torch.randn(yshape, generator=gen).to(dev)
    return g, g.detach().cpu().contiguous()


@pytest.mark.parametrize("grad", GRADS)
def test_gradient_layouts_at_128_channels(dev, monkeypatch, grad):
    """Every layout of the incoming gradient gives the gradients of its dense copy: on the default route (the kernels,
    for this patch geometry) the input gradient stays within 4 N kh kw 2^-24 conv2d_input(|w_q|, |G|) of the float64
    result masked by the clip, weight.grad within 4 rows 2^-24 conv2d_weight(|x_q|, |G|), the activation scalars
    within sum_bounds on the float64 grad_out; and they agree with the torch route within twice those bounds."""
    from quantized_vit_amd import _lib
    k, s, p, dil, xshape = CONV_PATCH
    got = {}
    for route in (None, "torch"):
        _route(monkeypatch, route)
        layer, x, aq = _build128(dev)
        wonly = _spy(monkeypatch, _lib, "gemm_wonly")
        xd = x.to(dev).requires_grad_(True)
        y = layer(xd)
        g, G = _grad_view(grad, tuple(y.shape), dev)
        del wonly[:]
        if grad == "expanded":
            y.sum().backward()
        else:
            y.backward(g)
        assert len(wonly) == (1 if route is None else 0)
        got[route] = (xd.grad.cpu().double(), layer.weight.grad.cpu().double(),
                      torch.stack([layer.d_quant_act.grad, layer.q_m_act.grad]).reshape(-1).cpu().double())
    plan = layer.quant_plan()
    w_q = layer.w_fakequant(plan).view_as(layer.weight).cpu().double()
    x_q = _lib.fake_quant_f32(x.to(dev), plan.qtype, plan.d_act, plan.qm_act, plan.t_act).cpu().double()
    G64, u = G.double(), 2.0 ** -24
    gxq = torch.nn.grad.conv2d_input(xshape, w_q, G64, s, p, dil)
    want_x = torch.where((x >= T.CLIP[1]) | (x <= T.CLIP[0]), torch.zeros_like(gxq), gxq)
    want_w = torch.nn.grad.conv2d_weight(x_q, tuple(w_q.shape), G64, s, p, dil)
    rows = G.shape[0] * G.shape[2] * G.shape[3]
    x_bound = 4 * N128 * k * k * u * torch.nn.grad.conv2d_input(xshape, w_q.abs(), G64.abs(), s, p, dil)
    w_bound = 4 * rows * u * torch.nn.grad.conv2d_weight(x_q.abs(), tuple(w_q.shape), G64.abs(), s, p, dil)
    r64, _, _, s_bounds = R.sum_bounds(x.reshape(-1), gxq.reshape(-1).float(), R.LINEAR, *aq, clip=T.CLIP)
    want_s = torch.stack([r64["sums"][0], r64["sums"][1]]).double()
    for route, (gx, gw, sc) in got.items():
        ex, ew = (gx - want_x).abs(), (gw - want_w).abs()
        print(f"{grad} route {route}: input worst err / bound {float((ex / x_bound.clamp_min(1e-300)).max()):.4f}, "
              f"weight {float((ew / w_bound.clamp_min(1e-300)).max()):.4f}, scalars err "
              f"{[f'{float(v):.2e}' for v in (sc - want_s).abs()]} bounds {[f'{b:.2e}' for b in s_bounds[:2]]}")
        assert bool((ex <= x_bound).all()) and bool((ew <= w_bound).all()), route
        assert all(abs(float(sc[i] - want_s[i])) <= s_bounds[i] for i in range(2)), route
    assert bool(((got[None][0] - got["torch"][0]).abs() <= 2 * x_bound).all())
    assert bool(((got[None][1] - got["torch"][1]).abs() <= 2 * w_bound).all())


# ---- a tiny ViT -----------------------------------------------------------------------------------------------------
# Worst per-parameter relative difference max|g_hip - g_torch| / max|g_torch| between the two conv routes, measured
# on the MI355X: both are fp32 evaluations of the same sums in different orders, and only the
# patch embedding's own gradients differ. The cap is four times the measured value rounded up to a power of two.
TINY_VIT_MEASURED = 5.63e-7        # patch_embed.proj.q_m_act
TINY_VIT_CAP = 2.0 ** -18          # 4 * 5.63e-7 = 2.25e-6 -> 3.81e-6


def test_tiny_vit_conv_routes_agree(dev, monkeypatch):
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
    print(f"tiny ViT, hip vs torch conv backward: worst per-parameter relative difference {worst:.3e} ({where})")
    assert worst <= TINY_VIT_CAP, (worst, where)
