"""80-wide heads on the split inference path at the module level: under no_grad a quantized block runs
qvit_gemm_qkv_split_hd -> qvit_attention_split (int8 codes for proj), as the 64-wide models do; with split_ok forced
off it runs the previous route (fp32 qkv GEMM -> qvit_attention -> proj's quantizer on its own).

The two routes quantize an fp32 attention output; a code of proj's input may differ between them only by one, where the
value lies at a rounding tie of proj's quantizer. LOGITS_BAR bounds max |logits_split - logits_previous| /
max |logits_previous| of the tiny model: twice the worst figure measured on an MI355X, rounded up to a power of two.
The measured figure is 0 with no differing code, and that is by construction: the GEMM
epilogue splits the QVIT_EPI_F32 value by the formula the fp32-input kernel applies to it, the split kernel repeats
that kernel's arithmetic in its order (test_gpu_attention_split_hd80.py asserts equal bits), and both quantizers
are the one device function. So the bar is 0: any difference is a change of arithmetic, not noise."""
import pytest
import torch

from test_gpu_attention_hd80 import HD
from test_gpu_attention_hd80_module import _tiny_vit

pytestmark = pytest.mark.gpu

LOGITS_BAR = 0.0     # 2 x the measured 0.0


def _count(monkeypatch):
    """Counts the calls of the three attention wrappers and the qkv split GEMM: {name: [(head_dim, out_mode)]}."""
    from quantized_vit_amd import _lib
    calls = {"attention": [], "attention_split": [], "gemm_qkv_split": [], "attention_backward": []}
    real = {k: getattr(_lib, k) for k in calls}
    monkeypatch.setattr(_lib, "attention", lambda *a, **kw: (
        calls["attention"].append((a[4], a[7] if len(a) > 7 else kw.get("out_mode", _lib.ATT_F32))),
        real["attention"](*a, **kw))[1])
    monkeypatch.setattr(_lib, "attention_split", lambda *a, **kw: (
        calls["attention_split"].append((a[5], a[8] if len(a) > 8 else kw.get("out_mode", _lib.ATT_F32))),
        real["attention_split"](*a, **kw))[1])
    monkeypatch.setattr(_lib, "gemm_qkv_split", lambda *a, **kw: (
        calls["gemm_qkv_split"].append(kw.get("head_dim", 64)), real["gemm_qkv_split"](*a, **kw))[1])
    monkeypatch.setattr(_lib, "attention_backward", lambda *a, **kw: (
        calls["attention_backward"].append(a[6]), real["attention_backward"](*a, **kw))[1])
    return calls


def _traced(model, x, monkeypatch):
    """(logits, proj input codes per block) of a no_grad forward with the code trace on."""
    from quantized_vit_amd import quant_layers as ql
    trace = {}
    monkeypatch.setattr(ql, "CODE_TRACE", trace)
    with torch.no_grad():
        logits = model(x)
    torch.cuda.synchronize()
    monkeypatch.setattr(ql, "CODE_TRACE", None)
    return logits.double().cpu(), [trace[b.attn.proj].cpu().to(torch.int32) for b in model.blocks]


def test_tiny_vit_routes_through_the_split_kernels(dev, monkeypatch):
    from quantized_vit_amd import _lib
    from quantized_vit_amd.vit_model import ViTAttention
    model, x, _ = _tiny_vit(dev)
    depth = len(model.blocks)
    calls = _count(monkeypatch)
    with torch.no_grad():
        l_plain = model(x)      # the last block computes its class rows only (behind the same attention calls)
    assert calls["attention_split"] == [(HD, _lib.ATT_I8)] * depth and calls["gemm_qkv_split"] == [HD] * depth
    assert calls["attention"] == [] and bool(torch.isfinite(l_plain).all())
    l_new, c_new = _traced(model, x, monkeypatch)
    assert calls["attention_split"] == [(HD, _lib.ATT_I8)] * (2 * depth) and calls["attention"] == []
    assert torch.equal(l_plain.double().cpu(), l_new)     # class-row tail and full last block: the same logits
    # the previous route: split_ok off
    monkeypatch.setattr(ViTAttention, "split_ok", lambda self, p_qkv: False)
    l_old, c_old = _traced(model, x, monkeypatch)
    assert calls["attention"] == [(HD, _lib.ATT_F32)] * depth and len(calls["attention_split"]) == 2 * depth
    assert len(calls["gemm_qkv_split"]) == 2 * depth
    for i, (a, b) in enumerate(zip(c_new, c_old)):
        d = (a - b).abs()
        print(f"block {i}: {int((d > 0).sum())} of {d.numel()} proj input codes differ between the routes, "
              f"max difference {int(d.max())}")
        assert int(d.max()) <= 1, i
    dist = float((l_new - l_old).abs().max()) / float(l_old.abs().max())
    print(f"tiny ViT (hd 80) logits, split route against the previous route: {dist:.3e} (bar {LOGITS_BAR:.3e})")
    assert dist <= LOGITS_BAR


def test_tiny_vit_under_autograd_keeps_the_autograd_core(dev, monkeypatch):
    model, x, w = _tiny_vit(dev)
    calls = _count(monkeypatch)
    model.zero_grad(set_to_none=True)
    (model(x) * w).sum().backward()
    assert [h for h, _ in calls["attention"]] == [HD, HD] and calls["attention_backward"] == [HD, HD]
    assert calls["attention_split"] == [] and calls["gemm_qkv_split"] == []


def test_vit_huge_block_routes_through_the_split_kernels(dev, monkeypatch):
    from quantized_vit_amd import _lib
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType
    from quantized_vit_amd.quant_model import model_to_quantize_model
    from quantized_vit_amd.vit_model import Block
    torch.manual_seed(0)
    blk = model_to_quantize_model(Block(1280, 16).to(dev), num_bits=4, quant_type=QuantizationType.SYMMETRIC_LINEAR,
                                  quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION).eval()
    x = torch.randn(1, 257, 1280, device=dev)
    calls = _count(monkeypatch)
    with torch.no_grad():
        y = blk(x)
    torch.cuda.synchronize()
    assert calls["attention_split"] == [(HD, _lib.ATT_I8)] and calls["gemm_qkv_split"] == [HD]
    assert calls["attention"] == [] and bool(torch.isfinite(y).all())
