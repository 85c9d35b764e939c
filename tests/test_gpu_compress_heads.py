"""compress_pruned_heads on the device: a model whose blocks keep different head counts gives the logits of its
uncompressed form, bit for bit, on the routes that form took: the fused qkv + attention kernel (block 0), its
class-token arm (the last block), the split pair, the unfused core; at head dim 80 through the split pair; and under
autograd through qvit_attention_backward.

Why equality is exact: a dead head's q, k and v are exact zeros, so its output columns and its codes into proj are
zeros and add nothing to proj's int32 sums; a surviving head's arithmetic reads its own columns only; the qkv layer's
output bound, which sizes the attention input scale, does not move because a dead head's bias entries are zeros.

Freshly calibrated W4A8 models, as tests/test_gpu_prune_step.py's compression test and for its reason: the statement is
about the integer path. Routes are observed as the dispatch-path tests observe them: vit_model.KERNEL_TIMING's hooks
for the fused block's launches and wrappers around the _lib entry points."""
import numpy as np
import pytest
import torch

import prune_heads_common as C
import prune_heads_ref as P
from prune_step_ref import PruneF64, PruneHyper

pytestmark = pytest.mark.gpu
WATCHED = ("qkv_attention", "qkv_attention_q", "gemm_qkv_split", "attention_split", "attention", "attention_backward")
TIMED = ("qkv_attn", "qkv_attn_cls", "proj", "proj_cls")
HEADS_ARG = {"qkv_attention": 9, "qkv_attention_q": 10, "attention_split": 4, "attention": 3, "attention_backward": 5}


def watch(monkeypatch):
    """{entry point: [num_heads of each call]} (the split GEMM: its N / 3 / head_dim)."""
    from quantized_vit_amd import _lib
    calls = {k: [] for k in WATCHED}

    def wrap(name, real):
        def f(*a, **kw):
            if name == "gemm_qkv_split":
                calls[name].append(a[5] // (3 * kw.get("head_dim", 64)))
            else:
                calls[name].append(a[HEADS_ARG[name]])
            return real(*a, **kw)
        return f
    for k in WATCHED:
        monkeypatch.setattr(_lib, k, wrap(k, getattr(_lib, k)))
    return calls


def forward(model, img, calls):
    """(logits, the entry points called, the fused block's timed launches) of one no_grad forward."""
    from quantized_vit_amd import vit_model
    for k in calls:
        calls[k].clear()
    for n in TIMED:
        vit_model.KERNEL_TIMING[n] = []
    try:
        with torch.no_grad():
            y = model(img).clone()
        torch.cuda.synchronize()
        timed = {n: len(vit_model.KERNEL_TIMING[n]) for n in TIMED}
    finally:
        for n in TIMED:
            vit_model.KERNEL_TIMING.pop(n, None)
    return y, {k: list(v) for k, v in calls.items()}, timed


def zero_heads(model, sets):
    with torch.no_grad():
        for blk, heads in zip(model.blocks, sets):
            rows = P.rows_of_units(heads, C.VIT_HEADS, C.VIT_HD)
            blk.attn.qkv.weight[rows] = 0
            blk.attn.qkv.bias[rows] = 0
        for m in model.modules():
            if callable(getattr(m, "invalidate", None)):
                m.invalidate()


@pytest.fixture(scope="module")
def schedule_sets(dev):
    """The head and MLP sets of the schedule test's reference run (the cosine criterion), computed on the host."""
    from test_gpu_prune_step import NSTEPS, SCHEDULE
    model = C.head_vit(dev)
    start = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    ref = PruneF64(P.permute({k: v.numpy() for k, v in start.items()}, C.VIT_SPECS),
                   PruneHyper(**SCHEDULE, criteria=C.COSINE), C.vit_ref_groups())
    for s in range(NSTEPS):
        ref.step(P.permute({k: v.numpy() for k, v in C.vit_grads(start, s).items()}, C.VIT_SPECS))
    pr = ref.pruned_rows()
    heads = [pr[f"blocks.{i}.attn"] for i in range(2)]
    assert any(heads) and all(len(h) < C.VIT_HEADS for h in heads)
    return heads, [pr[f"blocks.{i}.mlp"] for i in range(2)]


MODES = ("full", "split", "unfused")


def set_mode(mp, mode):
    from quantized_vit_amd import _lib
    from quantized_vit_amd.vit_model import ViTAttention
    if mode == "split":      # the fused kernel's token limit at 0: every block takes the split pair
        mp.setattr(_lib, "QKV_ATT_MAX_N", 0)
    elif mode == "unfused":  # neither: the qkv GEMM, then qvit_attention writing proj's codes
        mp.setattr(_lib, "QKV_ATT_MAX_N", 0)
        mp.setattr(ViTAttention, "split_ok", lambda self, p_qkv: False)


EXPECT = {   # the entry points of (block 0, last block) per mode, before and after compression alike
    "full": dict(qkv_attention=1, qkv_attention_q=1, gemm_qkv_split=0, attention_split=0, attention=0),
    "split": dict(qkv_attention=0, qkv_attention_q=0, gemm_qkv_split=2, attention_split=2, attention=0),
    "unfused": dict(qkv_attention=0, qkv_attention_q=0, gemm_qkv_split=0, attention_split=0, attention=2),
}


@pytest.mark.parametrize("case", ["schedule", "by_hand"])
def test_compressed_model_gives_the_same_logits_on_the_same_routes(dev, monkeypatch, schedule_sets, case):
    from quantized_vit_amd import _lib, compress_pruned_heads, compress_pruned_mlp
    from quantized_vit_amd.calibrate import synthetic_images
    from quantized_vit_amd.vit_model import attention_in_scale
    img = synthetic_images(2, 32, seed=9, device=dev)
    model = C.head_vit(dev, seed=0 if case == "schedule" else 2)
    if case == "schedule":
        heads, mlps = schedule_sets
        with torch.no_grad():
            for blk, rows in zip(model.blocks, mlps):
                blk.mlp.fc1.weight[rows] = 0
                blk.mlp.fc1.bias[rows] = 0
    else:
        heads = [[2], [0, 1, 3]]     # 3 of 4 and 1 of 4: proj has K = 192 and K = 64, both off the K tile
    zero_heads(model, heads)
    left = [C.VIT_HEADS - len(h) for h in heads]
    assert all((n * C.VIT_HD) % _lib.TILE_K for n in left)
    calls = watch(monkeypatch)
    before = {}
    for mode in MODES:
        with monkeypatch.context() as mp:
            set_mode(mp, mode)
            before[mode] = forward(model, img, calls)
    scale_before = [attention_in_scale(b.attn.qkv.quant_plan()) for b in model.blocks]
    bound_before = [b.attn.qkv.quant_plan().extra["out_bound"] for b in model.blocks]
    if case == "schedule":
        assert compress_pruned_mlp(model) is model
    assert compress_pruned_heads(model) is model
    assert [b.attn.num_heads for b in model.blocks] == left
    for blk, n in zip(model.blocks, left):
        a = blk.attn
        assert a.head_dim == C.VIT_HD and a.qkv.out_features == 3 * n * C.VIT_HD and a.proj.in_features == n * C.VIT_HD
        assert a.qkv.quant_plan().int_path and a.proj.quant_plan().int_path
        assert a.proj.quant_plan().k == n * C.VIT_HD
    assert [attention_in_scale(b.attn.qkv.quant_plan()) for b in model.blocks] == scale_before
    assert [b.attn.qkv.quant_plan().extra["out_bound"] for b in model.blocks] == bound_before
    for mode in MODES:
        with monkeypatch.context() as mp:
            set_mode(mp, mode)
            got, route, timed = forward(model, img, calls)
        want, route_before, timed_before = before[mode]
        assert {k: len(v) for k, v in route.items()} == {k: len(v) for k, v in route_before.items()}, mode
        assert {k: len(route[k]) for k in EXPECT[mode]} == EXPECT[mode], (mode, route)
        assert timed == timed_before, (mode, timed, timed_before)
        for k, v in route.items():          # the kernels were given the compressed head counts, block 0 first
            assert v == {"qkv_attention": left[:1], "qkv_attention_q": left[1:]}.get(k, left)[:len(v)], (mode, k, v)
        for k, v in route_before.items():
            assert all(h == C.VIT_HEADS for h in v), (mode, k, v)
        assert torch.isfinite(want).all()
        assert torch.equal(got, want), (mode, float((got - want).abs().max()))
    # the fused kernel on block 0 and the class-token arm on the last block, under the hooks the benchmark times
    assert before["full"][2]["qkv_attn"] == 1 and before["full"][2]["qkv_attn_cls"] == 1


def test_a_compressed_state_dict_loads_back(dev, schedule_sets):
    from quantized_vit_amd import compress_pruned_heads, compress_pruned_mlp, convert
    from quantized_vit_amd.calibrate import synthetic_images
    model = C.head_vit(dev)
    zero_heads(model, [[2], [0, 1, 3]])
    with torch.no_grad():
        model.blocks[1].mlp.fc1.weight[:99] = 0
        model.blocks[1].mlp.fc1.bias[:99] = 0
    compress_pruned_mlp(compress_pruned_heads(model))
    again = convert.vit_from_state_dict({k: v.cpu() for k, v in model.state_dict().items()}, device=dev)
    assert [b.attn.num_heads for b in again.blocks] == [3, 1]
    assert [b.mlp.fc1.out_features for b in again.blocks] == [C.VIT_HIDDEN, C.VIT_HIDDEN - 99]
    img = synthetic_images(2, 32, seed=9, device=dev)
    with torch.no_grad():
        assert torch.equal(again(img), model(img))


def test_head_dim_80_through_the_split_pair(dev, monkeypatch):
    """One block of two 80-wide heads, head 0 zeroed: the surviving head's codes into proj after compression (H = 1)
    are the bits of the uncompressed call's columns 80 .. 159."""
    from quantized_vit_amd import compress_pruned_heads, quant_layers as ql
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType
    from quantized_vit_amd.quant_model import model_to_quantize_model
    from quantized_vit_amd.vit_model import Block
    import torch.nn as nn
    torch.manual_seed(0)
    blk = model_to_quantize_model(Block(160, 2, qkv_bias=True).to(dev), num_bits=4,
                                  quant_type=QuantizationType.SYMMETRIC_LINEAR,
                                  quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION).eval()
    assert blk.attn.head_dim == 80
    with torch.no_grad():
        blk.attn.qkv.bias.copy_(torch.randn(480, device=dev) * 0.1)
        rows = P.rows_of_units([0], 2, 80)
        blk.attn.qkv.weight[rows] = 0
        blk.attn.qkv.bias[rows] = 0
    blk.attn.qkv.invalidate()
    holder = nn.Module()
    holder.blocks = nn.ModuleList([blk])
    x = torch.randn(2, 37, 160, device=dev)
    calls = watch(monkeypatch)
    out = []
    for _ in range(2):
        for k in calls:
            calls[k].clear()
        trace = {}
        monkeypatch.setattr(ql, "CODE_TRACE", trace)
        with torch.no_grad():
            y = blk(x)
        torch.cuda.synchronize()
        monkeypatch.setattr(ql, "CODE_TRACE", None)
        out.append((y.clone(), trace[blk.attn.proj].clone(), {k: list(v) for k, v in calls.items()}))
        compress_pruned_heads(holder)
    (y2, c2, r2), (y1, c1, r1) = out
    assert blk.attn.num_heads == 1 and blk.attn.qkv.out_features == 240 and blk.attn.proj.in_features == 80
    assert r2["gemm_qkv_split"] == [2] and r2["attention_split"] == [2] and r2["attention"] == []
    assert r1["gemm_qkv_split"] == [1] and r1["attention_split"] == [1] and r1["attention"] == []
    assert c2.shape[1] >= 160 and c1.shape[1] >= 80
    assert not c2[:, :80].any() and c2[:, 80:160].any()
    assert torch.equal(c1[:, :80], c2[:, 80:160])
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("train_fuse", [False, True], ids=["modules", "train_fuse"])
def test_backward_on_a_compressed_model(dev, monkeypatch, train_fuse):
    from quantized_vit_amd import compress_pruned_heads, vit_model
    from quantized_vit_amd.calibrate import synthetic_images
    monkeypatch.setattr(vit_model, "TRAIN_FUSE", train_fuse)
    model = C.head_vit(dev, seed=2)
    zero_heads(model, [[2], [0, 1, 3]])
    compress_pruned_heads(model)
    calls = watch(monkeypatch)
    img = synthetic_images(2, 32, seed=9, device=dev)
    model.zero_grad(set_to_none=True)
    loss = model(img).square().sum()
    loss.backward()
    assert calls["attention"] == [3, 1] and calls["attention_backward"] == [1, 3]
    assert calls["qkv_attention"] == [] and calls["attention_split"] == []
    for i, n in enumerate((3, 1)):
        a = model.blocks[i].attn
        for p, shape in ((a.qkv.weight, (3 * n * 64, 256)), (a.qkv.bias, (3 * n * 64,)), (a.proj.weight, (256, n * 64))):
            assert p.grad is not None and tuple(p.grad.shape) == shape and torch.isfinite(p.grad).all()
            assert p.grad.abs().sum() > 0
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in model.parameters())
