"""FrozenLinear / prepare_teacher: the frozen full-precision teacher on qvit_gemm_f32w.

A Block and a depth-2 VisionTransformer against the same module in float64 on the CPU: the "fp32" route within 2x the
error of the fp32 torch module itself (same seed, same device; the factor covers another summation order at equal
accuracy), the "bf16x2" route within 2^-10 of the output's largest magnitude (TF32-class accuracy from the operand
width, not from a measurement). A model that never meets prepare_teacher runs the modules' own route bit for bit."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from quantized_vit_amd import FrozenLinear, prepare_teacher
from quantized_vit_amd.vit_model import Block, VisionTransformer

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16x2"]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def cases(dev):
    """kind -> (fp32 module on the CPU, input, float64 CPU output, max error of the fp32 torch module on the device)"""
    torch.manual_seed(0)
    mods = {"block": (Block(dim=128, num_heads=2), _randn((3, 5, 128), 1)),
            "vit": (VisionTransformer(img_size=32, patch_size=16, num_classes=10, embed_dim=128, depth=2,
                                      num_heads=2), _randn((3, 3, 32, 32), 2))}
    out = {}
    with torch.no_grad():
        for kind, (m, x) in mods.items():
            m.eval()
            ref = copy.deepcopy(m).double()(x.double())
            err = float((copy.deepcopy(m).to(dev)(x.to(dev)).cpu().double() - ref).abs().max())
            out[kind] = (m, x, ref, err)
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
def test_frozen_linear(dev, precision):
    torch.manual_seed(3)
    lin = nn.Linear(100, 48).to(dev)
    f = FrozenLinear.from_linear(lin, precision)
    x = _randn((257, 100), 4).to(dev)
    rel = (4 * 100 + 9) * 2.0 ** -24 + (2.0 ** -13 + 2.0 ** -20 if precision == "bf16x2" else 0.0)

    def check():   # the kernel's bound on the product, plus the rounding of the one fp32 bias add
        with torch.no_grad():
            got = f(x).double()
            mag = x.double().abs() @ lin.weight.double().abs().t()
            ref = F.linear(x.double(), lin.weight.double(), lin.bias.double())
            assert bool(((got - ref).abs() <= rel * mag + 2.0 ** -24 * (mag + lin.bias.double().abs())).all())
        return got
    first = check()
    with torch.no_grad():
        lin.weight.copy_(_randn((48, 100), 5))      # the shared parameter: the cached image must follow it
    assert not torch.equal(check(), first)
    y = f(x)                                         # autograd live: F.linear, and gradients flow
    assert torch.equal(y, F.linear(x, lin.weight, lin.bias))
    y.sum().backward()
    assert lin.weight.grad is not None and lin.bias.grad is not None


@pytest.mark.parametrize("kind", ["block", "vit"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_block_and_vit_against_float64(dev, cases, precision, kind):
    m, x, ref, err_torch = cases[kind]
    t = prepare_teacher(copy.deepcopy(m).to(dev), precision)
    blk = t if kind == "block" else t.blocks[0]
    assert blk.frozen_ok(torch.empty(3, 5, 128, device=dev))
    with torch.no_grad():
        err = float((t(x.to(dev)).cpu().double() - ref).abs().max())
    print(f"teacher {kind} {precision}: err {err:.3e}, torch fp32 err {err_torch:.3e}, ratio {err / err_torch:.3f}, "
          f"err / max|ref| {err / float(ref.abs().max()):.3e}")
    if precision == "fp32":
        assert err <= 2.0 * err_torch
    else:
        assert err <= 2.0 ** -10 * float(ref.abs().max())


def test_unprepared_model_runs_the_modules_route(dev, cases):
    m, img = cases["vit"][0], cases["vit"][1].to(dev)
    m = copy.deepcopy(m).to(dev)
    assert not any(isinstance(l, FrozenLinear) for l in m.modules())
    with torch.no_grad():
        t = m.patch_embed(img)
        t = torch.cat((m.cls_token.expand(3, -1, -1), t), dim=1) + m.pos_embed
        for b in m.blocks:
            t = t + b.attn(b.norm1(t))
            t = t + b.mlp(b.norm2(t))
        assert torch.equal(m(img), m.head(m.norm(t[:, 0])))


def test_state_dict_keys_and_scope(cases):
    m = copy.deepcopy(cases["vit"][0])
    keys = list(m.state_dict().keys())
    t = prepare_teacher(m, "bf16x2")
    assert list(t.state_dict().keys()) == keys
    assert isinstance(t.head, FrozenLinear) and isinstance(t.blocks[1].mlp.fc2, FrozenLinear)
    assert not t.training and not any(p.requires_grad for p in t.parameters())
