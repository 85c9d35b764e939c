"""The fused ViT block takes the launches it took before ViTAttention.fused_route named the attention routes and
forward_fused_chain_ got one tail: for every case of fused_block_trace.CASES (the four routes, LAST_BLOCK_CLS_ONLY on
and off, FUSE_RESID_LN, FC1_WEIGHT_STATIONARY, two tokens) the ordered list of `_lib` wrapper calls with their
arguments equals tests/golden/fused_block_launches_parent.json element for element, and the logits are the same
bits. The recording was made by fused_block_trace.main at the parent commit. A change to a kernel that moves the
logits, or to a wrapper's signature, re-records it with that script; a change to the block's Python does not.
The timing events of one forward are counted per route as well: the "qkv_attn" and "proj" names belong to the fused
route alone.
"""
import json

import pytest
import torch

import fused_block_trace as fbt
from quantized_vit_amd import _lib, vit_model

pytestmark = pytest.mark.gpu

# the launches that tell a route from the others, and the route ViTAttention.fused_route must name
ROUTE_OF = {"fused": ("fused", {"qkv_attention"}), "fused768": ("fused", {"qkv_attention"}),
            "split128": ("split", {"gemm_qkv_split", "attention_split"}),
            "split_hd80": ("split", {"gemm_qkv_split", "attention_split"}),
            "attention_i8": ("attention_i8", {"attention"}), "core": ("core", set())}


@pytest.fixture(scope="module")
def golden():
    with open(fbt.GOLDEN) as f:
        return json.load(f)


def test_cases_are_the_recorded_ones(golden):
    assert sorted(golden["cases"]) == sorted(fbt.CASES)


@pytest.mark.parametrize("name", list(fbt.CASES))
def test_launches_and_logits_equal_parent(dev, golden, name):
    want = golden["cases"][name]
    switches = {s: getattr(vit_model, s) for s in fbt.SWITCHES}
    split_ok = vit_model.ViTAttention.split_ok
    try:
        events = {}
        launches, logits, model = fbt.run_case(dev, name, events)
    finally:   # run_case restores them itself; this test does not rely on that
        vit_model.ViTAttention.split_ok = split_ok
        for s, v in switches.items():
            setattr(vit_model, s, v)
    # the case's preconditions: every linear of every block on the int path with W4 codes, and the route it is named for
    plans = fbt.block_plans(model)
    assert all(p.int_path and p.wfmt == _lib.W4 for p in plans)
    route, marks = ROUTE_OF[name.split("-")[0]]
    called = {n for n, _ in launches}
    others = set().union(*(m for _, m in ROUTE_OF.values())) - marks
    assert marks <= called and not (others & called), sorted(called)
    assert ("qkv_attention_q" in called) == (route == "fused" and fbt.CASES[name][4]["LAST_BLOCK_CLS_ONLY"])
    a = model.blocks[0].attn
    N = model.patch_embed.num_patches + model.num_tokens
    if name.startswith("attention_i8"):
        a.split_ok = lambda p_qkv: False
    assert a.fused_route(a.qkv.quant_plan(), N) == route
    if "fc1_a32" in name:
        assert "gemm_a32" in called and "layernorm_quant_i8_t32" in called
    if "fuse_ln" in name:   # proj stays the plain GEMM off the fused route: one fused launch per fc2 -> next norm1
        fused_ln = sum(n == "gemm_resid_ln" for n, _ in launches)
        last = fbt.CASES[name][4]["LAST_BLOCK_CLS_ONLY"]
        assert fused_ln == ((2 if last else 3) if route == "fused" else 1)

    got = json.loads(json.dumps(launches))   # tuples -> lists, as the recording was stored
    assert len(got) == len(want["launches"]), [n for n, _ in got]
    for i, (g, w) in enumerate(zip(got, want["launches"])):
        assert g == w, f"launch {i}: {g} != {w}"
    # KERNEL_TIMING events of the forward, per name, as recorded; "qkv_attn" and "proj" are the fused route's alone
    assert events == want["events"]
    assert route == "fused" or events["qkv_attn"] == events["proj"] == events["qkv_attn_cls"] == 0
    assert list(logits.shape) == want["logits_shape"]
    recorded = torch.tensor(want["logits_bits"], dtype=torch.int32).view(torch.float32).reshape(logits.shape)
    assert torch.isfinite(recorded).all()
    assert torch.equal(logits, recorded)
    assert fbt.logits_bits(logits) == want["logits_bits"]
