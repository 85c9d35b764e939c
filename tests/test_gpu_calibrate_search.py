"""The clip search of calibrate.py on a tiny ViT (embed_dim 192, depth 2, 3 heads, 224 px): two calibration batches of
2 images, the second scaled so that every layer's max|x| differs between the batches. Error bars are those of
tests/test_gpu_quant_error.py (the search runs the nonlinear type at t = 1)."""
import copy

import pytest
import torch
import torch.nn as nn

from quantized_vit_amd import _lib, calibrate, vit_model
from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeConv2d, QuantizeLinear
from quantized_vit_amd.quant_model import model_to_quantize_model
from test_gpu_quant_error import LINEAR_BAR, NONLINEAR_BAR

pytestmark = pytest.mark.gpu

CFG = dict(img_size=224, patch_size=16, embed_dim=192, depth=2, num_heads=3)


@pytest.fixture(scope="module")
def fp32_model(dev):
    torch.manual_seed(0)
    model = vit_model.VisionTransformer(num_classes=10, representation_size=None, **CFG)
    calibrate.redraw_init_artifacts(model)
    return model.to(dev).eval()


@pytest.fixture(scope="module")
def batches():
    a = calibrate.synthetic_images(2, 224, seed=3)
    b = calibrate.synthetic_images(2, 224, seed=4) * 1.7
    return [a, b]


@pytest.fixture(scope="module")
def act_choices(fp32_model, batches):
    return calibrate.search_activation_quant(fp32_model, batches, bits=8)


def _layer_inputs(model, batches, names, dev):
    got = {n: [] for n in names}
    hooks = [mod.register_forward_hook(lambda m, inp, out, n=n: got[n].append(inp[0].detach().clone()))
             for n, mod in model.named_modules() if n in got]
    with torch.no_grad():
        for x in batches:
            model(x.to(dev))
    for h in hooks:
        h.remove()
    return got


def test_activation_search_covers_every_layer(fp32_model, batches, act_choices, dev):
    """Fails without the feature: calibrate has no search_activation_quant."""
    names = [n for n, m in fp32_model.named_modules() if isinstance(m, (nn.Linear, nn.Conv2d))]
    assert sorted(act_choices) == sorted(names) and len(names) == 2 * 4 + 2
    first = calibrate.collect_input_absmax(fp32_model, batches[0].to(dev))
    both = calibrate.collect_input_absmax(fp32_model, batches[1].to(dev))
    for n, c in act_choices.items():
        assert first[n] != both[n], n                         # the batches differ in every layer's range
        assert c.err <= c.err_absmax and c.err > 0 and c.numel > 0 and 0 < c.q_m <= max(first[n], both[n]), n
        assert c.t == 1.0 and c.clipped >= 1, n               # |x| >= q_m holds at least for the maximum itself


@pytest.mark.parametrize("name", ["blocks.1.mlp.fc2", "head"])
def test_stored_errors_match_a_recomputation(fp32_model, batches, act_choices, dev, name):
    """err and err_absmax against _lib.fake_quant_f32 and a torch double sum over both batches; err_absmax is the
    last candidate's error (q_m = max|x| over both batches)."""
    c = act_choices[name]
    xs = _layer_inputs(fp32_model, batches, [name], dev)[name]
    absmax = max(float(x.abs().max()) for x in xs)
    one = lambda v: torch.tensor([v], dtype=torch.float32, device=dev)
    for q_m, d, want in ((c.q_m, c.d, c.err), (absmax, calibrate.d_quant_for_bits(8, absmax, 1.0), c.err_absmax)):
        got = 0.0
        for x in xs:
            fq = _lib.fake_quant_f32(x, _lib.QT_NONLINEAR, one(d), one(q_m), one(1.0))
            p = torch.sign(x) * torch.exp(torch.log(x.abs()))            # t = 1: the un-rounded power
            got += float((p.double() - fq.reshape(x.shape).double()).square().sum())
        print(f"{name}: stored {want:.9e}, recomputed {got:.9e}, relative {abs(got - want) / got:.3e}")
        assert abs(got - want) <= NONLINEAR_BAR * got, (name, q_m, got, want)
    assert c.numel == sum(x.numel() for x in xs)


def _quantize(fp32_model, batches):
    return calibrate.quantize_pretrained(copy.deepcopy(fp32_model), batches)


def test_quantize_pretrained_stays_on_the_integer_path(fp32_model, batches, dev):
    plain = model_to_quantize_model(copy.deepcopy(fp32_model), num_bits=4,
                                    quant_type=QuantizationType.SYMMETRIC_NONLINEAR,
                                    quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    model, report = _quantize(fp32_model, batches)
    assert list(model.state_dict()) == list(plain.state_dict())
    layers = {n: m for n, m in model.named_modules() if isinstance(m, (QuantizeLinear, QuantizeConv2d))}
    assert sorted(report) == sorted(layers) and len(layers) == 10
    for n, m in layers.items():
        plan = m.quant_plan()
        act, wt = report[n]
        assert plan.int_path, n
        assert abs(plan.level_wt) <= 7 and abs(plan.level_act) <= 127, (n, plan.level_wt, plan.level_act)
        assert float(m.q_m_act) == torch.tensor(act.q_m).item() and float(m.d_quant_act) == torch.tensor(act.d).item()
        assert float(m.q_m_wt) == torch.tensor(wt.q_m).item() and float(m.d_quant_wt) == torch.tensor(wt.d).item()
        assert wt.err <= wt.err_absmax and act.err <= act.err_absmax, n
    img = calibrate.synthetic_images(2, 224, seed=9, device=dev)
    with torch.no_grad():
        y = model(img)
    assert bool(torch.isfinite(y).all())
    model2, report2 = _quantize(fp32_model, batches)
    assert report2 == report
    with torch.no_grad():
        assert torch.equal(model2(img), y)


def test_widened_step_fits_the_level():
    """A pair whose saturation code exceeds the level (a very small q_m: the reference adds 1e-6 to it) gets the
    smallest fp32 d that fits, and says so; a fitting pair is left alone."""
    from quantized_vit_amd.quant_layers import saturation_level
    import numpy as np
    c = calibrate.QuantChoice(q_m=1e-5, d=calibrate.d_quant_for_bits(4, 1e-5), t=1.0, err=0.0, err_absmax=0.0,
                              clipped=0, numel=1)
    assert saturation_level(_lib.QT_NONLINEAR, c.d, c.q_m, 1.0) > 7
    w = calibrate._fit_level(c, _lib.QT_NONLINEAR, 4)
    assert w.widened and w.d > c.d and saturation_level(_lib.QT_NONLINEAR, w.d, w.q_m, 1.0) == 7
    below = float(np.nextafter(np.float32(w.d), np.float32(0)))
    assert saturation_level(_lib.QT_NONLINEAR, below, w.q_m, 1.0) > 7
    ok = calibrate.QuantChoice(q_m=0.5, d=calibrate.d_quant_for_bits(8, 0.5), t=1.0, err=0.0, err_absmax=0.0,
                               clipped=0, numel=1)
    assert calibrate._fit_level(ok, _lib.QT_NONLINEAR, 8) is ok


def test_build_quantized_vit_still_uses_absmax(dev):
    """build_quantized_vit with its defaults gives the parameters the untouched collect_input_absmax /
    set_activation_quant give."""
    model = calibrate.build_quantized_vit("vit_tiny_patch16_224", seed=0, depth=2, device=dev)
    torch.manual_seed(0)
    ref = vit_model.VisionTransformer(num_classes=1000, representation_size=None,
                                      **dict(calibrate.VIT_CONFIGS["vit_tiny_patch16_224"], depth=2))
    calibrate.redraw_init_artifacts(ref)
    ref = ref.to(dev).eval()
    gen = torch.Generator(device="cpu").manual_seed(1)
    img = (torch.rand(2, 3, 224, 224, generator=gen) * 2 - 1).to(dev)
    absmax = calibrate.collect_input_absmax(ref, img)
    ref = model_to_quantize_model(ref, num_bits=4, quant_type=QuantizationType.SYMMETRIC_NONLINEAR,
                                  quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    calibrate.set_activation_quant(ref, absmax, bits=8, t=1.0)
    a, b = model.state_dict(), ref.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for n, m in model.named_modules():
        if isinstance(m, (QuantizeLinear, QuantizeConv2d)):
            assert float(m.q_m_act) == torch.tensor(max(absmax[n], 1e-8)).item(), n


def test_nan_input_names_the_layer(fp32_model, batches):
    bad = batches[0].clone()
    bad[1, 2, 100, 50] = float("nan")
    with pytest.raises(ValueError, match="patch_embed.proj"):
        calibrate.search_activation_quant(fp32_model, [batches[1], bad])
