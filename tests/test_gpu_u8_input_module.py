"""QuantizeConv2d.set_uint8_input and VisionTransformer.set_uint8_input on the device: a torch.uint8 image gives,
on every forward route and in both layouts, the bits of the forward on the fp32 image V[c][input] (ToTensor +
Normalize as a table, tests/u8_input_ref.py); the setting's lifecycle; autograd on the integer path; a tiny ViT.

Bars: torch.equal throughout. Both sides run the library's own quantizer on the same fp32 values (the table is
built by it), so rounding ties cannot separate them."""
import pytest
import torch
import torch.nn as nn

import u8_input_ref as U
from quantized_vit_amd import calibrate, quant_layers, vit_model
from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeConv2d
from quantized_vit_amd.quant_model import model_to_quantize_model
from test_gpu_conv_geometry import PATHS

pytestmark = pytest.mark.gpu

MEAN, STD = U.IMAGENET
CASES = {c.id: c for c in U.U8_CASES}
GEOMETRIES = ["U1", "U2", "A1"]
LAYOUTS = ["nchw", "nhwc"]


def _on_device(img, layout, dev):
    """[B, C, H, W] uint8 on the device: contiguous, or channels_last (a decoder's [B, H, W, C] through permute)."""
    if layout == "nchw":
        return img.to(dev)
    x = img.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)
    assert not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
    return x


def _v_image(img, mean=MEAN, std=STD):
    return U.value_image(img, U.value_table(mean, std))


def _build(dev, case, path, cout=24):
    torch.manual_seed(PATHS.index(path) + 10 * U.U8_CASE_IDS.index(case.id))
    conv = nn.Conv2d(case.C, cout, case.k, stride=case.s, padding=case.p, dilation=case.d, bias=True)
    mode = QuantizationMode.WEIGHT_AND_ACTIVATION if path.startswith("wa") else QuantizationMode.WEIGHT_ONLY
    bits = {"wa4-int": 4, "wonly4": 4, "wonly16": 16, "wa32-library": 32}[path]
    q = QuantizeConv2d.from_module(conv, quant_type=QuantizationType.SYMMETRIC_NONLINEAR, quant_mode=mode,
                                   num_bits=bits).to(dev).eval()
    if path == "wa4-int":
        with torch.no_grad():
            q.q_m_act.fill_(2.0)
            q.d_quant_act.fill_(2.0 / 127)
        q.invalidate()
    plan = q.quant_plan()
    if path == "wa4-int":
        assert plan.int_path
    elif path in ("wonly4", "wonly16"):
        assert not plan.int_path and plan.extra.get("wonly")
    else:
        assert not plan.int_path and not plan.extra.get("wonly")
    return q


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_uint8_forward_equals_v_image_forward(dev, geometry, path):
    case = CASES[geometry]
    q = _build(dev, case, path)
    img = U.make_image(case)
    with torch.no_grad():
        want = q(_v_image(img).to(dev))
    q.set_uint8_input(MEAN, STD)
    assert q.uint8_input == (tuple(float(torch.tensor(m, dtype=torch.float32)) for m in MEAN),
                             tuple(float(torch.tensor(s, dtype=torch.float32)) for s in STD))
    for layout in LAYOUTS:
        x = _on_device(img, layout, dev)
        with torch.no_grad():
            got = q(x)
        assert got.dtype == torch.float32 and torch.equal(got, want), layout
        live = q(x)                                   # a live autograd graph: the fp32 image is expanded first
        assert live.grad_fn is not None and torch.equal(live.detach(), want), layout
    with torch.no_grad():                             # a float input is taken as already normalised
        assert torch.equal(q(_v_image(img).to(dev)), want)
        strided = _on_device(torch.cat([img, img], 3), "nchw", dev)[..., :case.W]   # neither layout: copied first
        assert not strided.is_contiguous() and not strided.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(q(strided), want)


def test_uint8_forward_on_the_grouped_route(dev):
    """groups > 1 leaves the integer path for the library convolution: the image is expanded first."""
    case = CASES["A1"]
    torch.manual_seed(3)
    conv = nn.Conv2d(case.C, 6, case.k, stride=case.s, padding=case.p, dilation=case.d, bias=True, groups=3)
    q = QuantizeConv2d.from_module(conv, quant_type=QuantizationType.SYMMETRIC_LINEAR,
                                   quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION, num_bits=4).to(dev).eval()
    with torch.no_grad():
        q.q_m_act.fill_(2.0)
        q.d_quant_act.fill_(2.0 / 127)
    q.invalidate()
    assert q.groups == 3 and not q._int_conv_ok()
    img = U.make_image(case)
    q.set_uint8_input(MEAN, STD)
    with torch.no_grad():
        want = q(_v_image(img).to(dev))
        for layout in LAYOUTS:
            assert torch.equal(q(_on_device(img, layout, dev)), want), layout


def test_setting_lifecycle(dev):
    case = CASES["U1"]
    q = _build(dev, case, "wa4-int")
    img = U.make_image(case)
    x = _on_device(img, "nchw", dev)
    keys = list(q.state_dict().keys())
    values = [v.clone() for v in q.state_dict().values()]
    assert q.uint8_input is None
    with torch.no_grad():
        raw = q(x.float())
        assert torch.equal(q(x), raw)                 # no setting: today's raw .float() conversion
        q.set_uint8_input(MEAN, STD)
        assert list(q.state_dict().keys()) == keys
        assert all(torch.equal(a, b) for a, b in zip(q.state_dict().values(), values))
        assert not any("u8" in n for n, _ in list(q.named_buffers()) + list(q.named_parameters()))
        assert torch.equal(q(x), q(_v_image(img).to(dev)))
        assert not torch.equal(q(x), raw)
        # a quantizer update drops the tables with the plan
        q.d_quant_act.data.fill_(2.0 / 100)
        q.invalidate()
        assert "u8_tables" not in q.quant_plan().extra
        assert torch.equal(q(x), q(_v_image(img).to(dev)))
        assert "u8_tables" in q.quant_plan().extra
        # another mean: the cached tables are replaced
        q.set_uint8_input(0.5, 0.5)
        assert q.uint8_input == ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
        half = q(_v_image(img, *U.HALF).to(dev))
        assert torch.equal(q(x), half) and not torch.equal(half, q(_v_image(img).to(dev)))
        q.clear_uint8_input()
        assert q.uint8_input is None and torch.equal(q(x), q(x.float()))   # the raw conversion again
    with pytest.raises(AttributeError):
        q.uint8_input = (MEAN, STD)                   # read-only


@pytest.mark.parametrize("mean,std", [(0.5, 0.0), ((0.5, 0.5, 0.5), (0.5, 0.0, 0.5)), (float("nan"), 0.5),
                                      (0.5, float("inf")), ((0.5, 0.5), 0.5), (0.5, (0.5, 0.5, 0.5, 0.5))])
def test_setting_rejects_bad_values(dev, mean, std):
    q = _build(dev, CASES["U1"], "wonly4")
    with pytest.raises(ValueError):
        q.set_uint8_input(mean, std)
    assert q.uint8_input is None


def test_autograd_on_the_integer_path(dev):
    """Output and every parameter gradient of the uint8 run equal the fp32 run's bit for bit."""
    case = CASES["U1"]
    q = _build(dev, case, "wa4-int").train(False)
    img = U.make_image(case)
    q.set_uint8_input(MEAN, STD)
    torch.manual_seed(9)
    runs = []
    for x in (_v_image(img).to(dev), _on_device(img, "nchw", dev), _on_device(img, "nhwc", dev)):
        q.zero_grad(set_to_none=True)
        y = q(x)
        assert y.grad_fn is not None
        if not runs:
            G = torch.randn_like(y)
        (y * G).sum().backward()
        grads = {n: p.grad.clone() for n, p in q.named_parameters() if p.grad is not None}
        runs.append((y.detach().clone(), grads))
    y0, g0 = runs[0]
    assert {"weight", "bias", "d_quant_act", "d_quant_wt"} <= set(g0)
    for y, g in runs[1:]:
        assert torch.equal(y, y0) and set(g) == set(g0)
        for n in g0:
            assert torch.equal(g[n], g0[n]), n


def test_tiny_vit(dev):
    """Depth 2, embed 192, 3 heads, 32 x 32, patch 16, W4A8, calibrated as calibrate.build_quantized_vit does:
    logits and the patch embedding's traced codes from bytes equal those from the V-image."""
    torch.manual_seed(0)
    model = vit_model.VisionTransformer(img_size=32, patch_size=16, embed_dim=192, depth=2, num_heads=3,
                                        num_classes=10, representation_size=None)
    calibrate.redraw_init_artifacts(model)
    model = model.eval()
    with pytest.raises(TypeError):
        model.set_uint8_input()                       # not quantized yet: patch_embed.proj is an nn.Conv2d
    gen = torch.Generator().manual_seed(1)
    calib = torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1
    absmax = calibrate.collect_input_absmax(model, calib)
    model = model_to_quantize_model(model, num_bits=4, quant_type=QuantizationType.SYMMETRIC_NONLINEAR,
                                    quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    calibrate.set_activation_quant(model, absmax, bits=8, t=1.0)
    model = model.to(dev).eval()
    proj = model.patch_embed.proj
    assert isinstance(proj, QuantizeConv2d) and proj.quant_plan().int_path
    model.set_uint8_input()
    assert proj.uint8_input == ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    img = torch.randint(0, 256, (2, 3, 32, 32), dtype=torch.uint8, generator=gen)
    img[0, :, 0, :2] = torch.tensor([0, 255], dtype=torch.uint8)

    def run(x):
        quant_layers.CODE_TRACE = {}
        try:
            with torch.no_grad():
                y = model(x)
            return y, quant_layers.CODE_TRACE[proj]
        finally:
            quant_layers.CODE_TRACE = None

    want, want_codes = run(_v_image(img, *U.HALF).to(dev))
    assert torch.isfinite(want).all() and want_codes.abs().max() > 0
    for layout in LAYOUTS:
        got, got_codes = run(_on_device(img, layout, dev))
        assert torch.equal(got_codes, want_codes), layout
        assert torch.equal(got, want), layout
