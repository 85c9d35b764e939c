"""head_dim 80 at the module level: ViTAttention.core, a tiny ViT with 80-wide heads and one ViT-Huge/14 block run
their attention core on qvit_attention / qvit_attention_backward, as the 64-wide models do.

Bounds: C_BWD is the kernel-level constant of test_gpu_attention_hd80.py. C_MODEL bounds the distance between the
HIP-core route and the torch-branch route of a whole model, per parameter, in units of
max|g_torch| * 80 * eps32 (80 eps: the fp32 yardstick's own scale for sums over head_dim = 80 products, as the
width-64 tiny-ViT test takes 64 eps); it is the next power of two at or above twice the worst figure measured on an
MI355X."""
import pytest
import torch

import attention_hd_ref as R
from test_gpu_attention_hd80 import C_BWD, HD, check_bwd

pytestmark = pytest.mark.gpu

MB, MN, MDIM, MH = 2, 17, 160, 2
C_MODEL = 2.0     # worst 0.672 units: the tiny ViT's blocks.1.attn.proj.d_quant_act gradient
TRAIN_FUSE_CAP = 2.0 ** -10     # DESIGN.md section 14's bar for the fused route against the modules route


def _module(dev, drop=0.0):
    from quantized_vit_amd.vit_model import ViTAttention
    torch.manual_seed(0)
    attn = ViTAttention(MDIM, num_heads=MH, qkv_bias=True, attn_drop_ratio=drop).to(dev)
    assert attn.head_dim == HD
    return attn


def test_core_under_autograd_is_the_no_grad_kernel(dev, monkeypatch):
    from quantized_vit_amd.vit_model import ViTAttention, _AttentionCore
    attn = _module(dev).eval()
    qkv_c, dO_c, _, _, g64, g32 = R.case(MB, MN, MH, HD, 2)
    qkv = qkv_c.reshape(MB, MN, -1).to(dev)
    with torch.no_grad():
        y0 = attn.core(qkv, MB, MN)
    x = qkv.clone().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        y = attn.core(x, MB, MN)
    assert torch.equal(y, y0)
    fn = y.grad_fn
    while fn is not None and "AttentionCore" not in type(fn).__name__:
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert fn is not None and type(fn).__name__.startswith(_AttentionCore.__name__)
    assert saved, "the Function saves qkv and the output"
    for shp in saved:
        assert not (len(shp) >= 2 and shp[-1] == MN and shp[-2] == MN), shp
        n = 1
        for d in shp:
            n *= d
        assert n != MB * MH * MN * MN and n <= MB * MN * 3 * MDIM, shp
    y.backward(dO_c.reshape(MB, MN, -1).to(dev))
    g_hip = x.grad.reshape(MB * MN, -1).clone()
    check_bwd("module core", g_hip, g64, g32, MH)
    # the torch branch of the same module: both are within C max(err_t, eps) of the truth
    monkeypatch.setattr(ViTAttention, "hip_ok", lambda self, qkv: False)
    x2 = qkv.clone().requires_grad_(True)
    y2 = attn.core(x2, MB, MN)
    assert "AttentionCore" not in type(y2.grad_fn).__name__
    y2.backward(dO_c.reshape(MB, MN, -1).to(dev))
    g_t = x2.grad.reshape(MB * MN, -1)
    et = R.section_errs(g_t, g64, MH, HD)
    d = R.section_errs(g_hip, g_t.double().cpu(), MH, HD)
    for sec, dist, e_t, e_32 in zip(("dq", "dk", "dv"), d, et, R.section_errs(g32, g64, MH, HD)):
        bound = C_BWD * max(e_32, R.EPS32) + e_t
        print(f"module core vs torch branch {sec}: {dist:.3e} (bound {bound:.3e})")
        assert dist <= bound * (1 + 1e-6), sec


def test_attention_dropout_keeps_the_torch_branch(dev, monkeypatch):
    from quantized_vit_amd import _lib
    attn = _module(dev, drop=0.1).train()
    calls = []
    real = _lib.attention
    monkeypatch.setattr(_lib, "attention", lambda *a, **kw: (calls.append(a[4]), real(*a, **kw))[1])
    x = R.case(MB, MN, MH, HD, 2)[0].reshape(MB, MN, -1).to(dev).requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        y = attn.core(x, MB, MN)
    assert "AttentionCore" not in type(y.grad_fn).__name__ and not calls
    assert any(len(s) == 4 and s[-1] == MN and s[-2] == MN for s in saved)


def _tiny_vit(dev):
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType
    from quantized_vit_amd.quant_model import model_to_quantize_model
    from quantized_vit_amd.vit_model import VisionTransformer
    torch.manual_seed(0)
    model = VisionTransformer(img_size=56, patch_size=14, embed_dim=160, depth=2, num_heads=2, num_classes=10)
    model = model_to_quantize_model(model.to(dev), num_bits=4, quant_type=QuantizationType.SYMMETRIC_LINEAR,
                                    quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION).eval()
    assert all(b.attn.head_dim == HD for b in model.blocks)
    return model, torch.randn(2, 3, 56, 56, device=dev), torch.randn(2, 10, device=dev)


def _run(model, x, w):
    model.zero_grad(set_to_none=True)
    logits = model(x)
    (logits * w).sum().backward()
    return logits.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}


def _worst(a, ref):
    worst, where = 0.0, None
    for n in ref:
        den = float(ref[n].abs().max())
        err = float((a[n] - ref[n]).abs().max()) / den if den > 0 else float(a[n].abs().max())
        print(f"  {n}: {err:.3e}")
        if err > worst:
            worst, where = err, n
    return worst, where


def test_tiny_vit_matches_the_torch_branch(dev, monkeypatch):
    from quantized_vit_amd import _lib, vit_model as vm
    model, x, w = _tiny_vit(dev)
    calls = {"fwd": [], "bwd": []}
    real_f, real_b = _lib.attention, _lib.attention_backward
    monkeypatch.setattr(_lib, "attention", lambda *a, **kw: (calls["fwd"].append(a[4]), real_f(*a, **kw))[1])
    monkeypatch.setattr(_lib, "attention_backward",
                        lambda *a, **kw: (calls["bwd"].append(a[6]), real_b(*a, **kw))[1])
    l_hip, g_hip = _run(model, x, w)
    assert calls == {"fwd": [HD, HD], "bwd": [HD, HD]}   # both blocks, forward and backward, on the HIP core
    monkeypatch.setattr(vm, "TRAIN_FUSE", True)
    l_fus, g_fus = _run(model, x, w)
    assert calls == {"fwd": [HD] * 4, "bwd": [HD] * 4}
    monkeypatch.setattr(vm, "TRAIN_FUSE", False)
    monkeypatch.setattr(vm.ViTAttention, "hip_ok", lambda self, qkv: False)
    l_ref, g_ref = _run(model, x, w)
    assert calls == {"fwd": [HD] * 4, "bwd": [HD] * 4}   # the torch branch made no call
    unit = HD * R.EPS32
    e_log = float((l_hip - l_ref).abs().max()) / float(l_ref.abs().max())
    worst, where = _worst(g_hip, g_ref)
    print(f"tiny ViT (hd 80), HIP core vs torch branch: logits {e_log:.3e} = {e_log / unit:.3f} units, worst gradient "
          f"{worst:.3e} = {worst / unit:.3f} units ({where})")
    assert e_log <= C_MODEL * unit and worst <= C_MODEL * unit, (e_log, worst, where)
    assert all(bool(torch.isfinite(g).all()) for g in g_fus.values()) and set(g_fus) == set(g_hip)
    e_fl = float((l_fus - l_hip).abs().max()) / float(l_hip.abs().max())
    w_fus, where_f = _worst(g_fus, g_hip)
    print(f"tiny ViT (hd 80), TRAIN_FUSE vs modules route: logits {e_fl:.3e}, worst gradient {w_fus:.3e} ({where_f})")
    assert w_fus <= TRAIN_FUSE_CAP and e_fl <= TRAIN_FUSE_CAP, (w_fus, where_f, e_fl)


def test_vit_huge_block_runs_one_hd80_kernel_and_no_score_tensor(dev, monkeypatch):
    """Block(1280, 16) at ViT-Huge/14's 257 tokens under no_grad. The check is the call count (exactly one
    qvit_attention call, with head_dim 80) and the comparison with the torch branch below. The peak allocation over
    that call is reported and asserted below one [1, 16, 257, 257] fp32 tensor, but the call writes into a buffer
    its caller allocated, so that figure is 0 by construction; over the whole block it cannot be measured at
    B = 1, where the MLP's [257, 5120] hidden tensor (5.3 MB) is larger than one score tensor (4.2 MB)."""
    from quantized_vit_amd import _lib
    from quantized_vit_amd.vit_model import Block
    torch.manual_seed(0)
    blk = Block(1280, 16).to(dev).eval()
    x = torch.randn(1, 257, 1280, device=dev)
    calls, rise = [], []
    real = _lib.attention

    def counted(*a, **kw):
        calls.append(a[4])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out = real(*a, **kw)
        torch.cuda.synchronize()
        rise.append(torch.cuda.max_memory_allocated(dev) - before)
        return out
    monkeypatch.setattr(_lib, "attention", counted)
    with torch.no_grad():
        y = blk(x)
    assert calls == [HD] and bool(torch.isfinite(y).all())
    scores = 16 * 257 * 257 * 4
    print(f"peak allocation over the attention call: {rise[0]} B (one score tensor: {scores} B)")
    assert rise[0] < scores
    monkeypatch.setattr(_lib, "attention", real)
    monkeypatch.setattr(type(blk.attn), "hip_ok", lambda self, qkv: False)
    with torch.no_grad():
        y_t = blk(x)
    err = float((y - y_t).abs().max()) / float(y_t.abs().max())
    print(f"block output, HIP core vs torch branch: {err:.3e}")
    assert err <= C_MODEL * HD * R.EPS32
