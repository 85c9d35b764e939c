"""Plan lifecycle: the cached weight images of QuantizeLinear / QuantizeConv2d (QuantPlan), of the ViT's fused block
routes and of UltraNet's caches must follow the parameters, whatever way the parameters change.

Yardstick (tests/plan_lifecycle_ref.py): after a mutation every route of the mutated layer equals, bit for bit
(torch.equal), the same route of a FRESH TWIN built from its state_dict(); the twin is pinned per scenario to the CPU
oracle's weight codes (proven rounding ties aside, at most 1e-3 of the codes), to w_fakequant == d_wt * codes, and to
the float64 restatement of the forward at the bar of tests/test_gpu_layer_autograd.py::_check_layer. No tolerance of
this file's own.

The stale contract (a `.data` edit without invalidate(), which the plan's key cannot see): every route that reads an
image of the plan answers for the parameters the plan was built from, bit-equal to a twin built before the edit; the
first invalidate() moves all of them to the new parameters. The weight-side gradients (wgrad through the weight
quantizer's backward, the weight scalars' gradients) differentiate with respect to the live fp32 master weight,
which no plan holds: on a stale eval-mode plan they are pinned to the NEW twin's bits (they depend on the live weight,
the output gradient and the activation codes only), every other route to the OLD twin's. A training-mode call
rebuilds the plan, so it cannot be stale and is not part of the stale comparison.
"""
import copy
import gc

import pytest
import torch
import torch.nn as nn

import plan_lifecycle_ref as P

pytestmark = pytest.mark.gpu

WREG_MODES = ("w4r", "w8r", "w4")


class _wreg:
    """quant_layers.GEMM_WREG set for a block and restored (as test_quant_linear_plan_holds_w4r does)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from quantized_vit_amd import quant_layers as QL
        self.saved = QL.GEMM_WREG
        if self.mode is not None:
            QL.GEMM_WREG = self.mode

    def __exit__(self, *exc):
        from quantized_vit_amd import quant_layers as QL
        QL.GEMM_WREG = self.saved


def _warm(layer, x):
    """An eval forward: the plan exists, and on a W4 int-path plan the register image is built and the packed
    codes are released; nothing else has been derived yet."""
    with torch.no_grad():
        layer(x)
    return layer.quant_plan()


def _applicable(layer, mutation: str) -> bool:
    touched = P.MUTATIONS[mutation][0]
    return all(getattr(layer, n, None) is not None for n in touched) or mutation in ("sgd_step",)


LAYER_CASES = [("qkv", m) for m in WREG_MODES] + [(n, None) for n in ("fc1", "fc2", "lin", "wonly", "conv")]


@pytest.mark.parametrize("name,wreg", LAYER_CASES)
def test_layer_follows_every_mutation(dev, name, wreg):
    """Every route of a warm layer follows every mutation of the table without invalidate()."""
    x = P.layer_input(name).to(dev)
    failures = {}
    with _wreg(wreg):
        for mutation, (touched, mutate) in P.MUTATIONS.items():
            layer = P.build_layer(name, dev)
            if not _applicable(layer, mutation):
                continue
            before = P.fresh_twin(layer)
            _warm(layer, x)
            mutate(layer)
            assert not layer.training
            got = P.run_routes(layer, x)
            twin = P.fresh_twin(layer)
            want = P.run_routes(twin, x)
            P.assert_twin_pinned(twin, x, want)
            bad = P.unequal_routes(got, want)
            if bad:
                failures[mutation] = bad
            if touched:   # the comparer can tell: the twin from before the mutation is another layer
                assert P.unequal_routes(P.run_routes(before, x), want), mutation
    assert not failures, failures


@pytest.mark.parametrize("name", ["qkv", "lin"])
def test_storage_class_moves(dev, name):
    """In-place scalar edits move one warm plan W4 -> W8 -> W4 -> weight-only GEMM -> int path -> W16 -> W24 -> fp32
    fake-quant -> W4; after each move the class is the expected one and every route equals the twin's."""
    x = P.layer_input(name).to(dev)
    layer = P.build_layer(name, dev)
    assert P.plan_class(_warm(layer, x)) == ("W4", True, False)
    failures = {}
    for move, edit, expect in P.CLASS_MOVES:
        edit(layer)
        plan = _warm(layer, x)
        assert P.plan_class(plan) == expect, (move, P.plan_class(plan))
        got = P.run_routes(layer, x)
        twin = P.fresh_twin(layer)
        want = P.run_routes(twin, x)
        P.assert_twin_pinned(twin, x, want)
        bad = P.unequal_routes(got, want)
        if bad:
            failures[move] = bad
        _warm(layer, x)
    assert not failures, failures


@pytest.mark.parametrize("name,wreg", [("qkv", m) for m in WREG_MODES] + [("fc2", None), ("conv", None)])
def test_stale_contract(dev, name, wreg):
    """`.data` edit of the weight, no invalidate(): every route that reads the plan answers for the OLD weight (a mix
    of old and new routes is the failure: before the plan derived its later images from what it holds, packed_codes(),
    packed_t(), w_fakequant and weight_codes() gave the new weight's codes beside the old register image)."""
    x = P.layer_input(name).to(dev)
    with _wreg(wreg):
        layer = P.build_layer(name, dev)
        old_twin = P.fresh_twin(layer)
        plan = _warm(layer, x)
        if wreg in ("w4r", "w8r"):
            assert plan.packed is None and plan.extra.get("wreg") is not None
        layer.weight.data.mul_(1.25)
        layer.weight.data[0].neg_()
        got = P.run_routes(layer, x, weight_grads="eval")
        assert layer.quant_plan() is plan
        new_twin = P.fresh_twin(layer)
        old = P.run_routes(old_twin, x, weight_grads="eval")
        new = P.run_routes(new_twin, x, weight_grads="eval")
        verdict = P.classify_routes(got, old, new)
        moved = [k for k, v in P.classify_routes(new, old, new).items() if v != "both"]
        # (weight.grad itself is the straight-through mask times a product that has no weight in it: only a weight
        # crossing the clip range would move it; the weight quantizer's scalar gradient does move)
        assert {"forward", "weight_codes", "w_fakequant", "eval.hip.x.grad", "eval.hip.d_quant_wt.grad"} <= set(moved)
        assert name == "conv" or "eval.torch.x.grad" in moved
        # the gradients with respect to the live master weight and its quantizer's scalars: the new weight's
        live = {k: v for k, v in verdict.items() if k.endswith(("weight.grad", "_wt.grad"))}
        plan_routes = {k: v for k, v in verdict.items() if k not in live}
        assert live and set(live.values()) <= {"new", "both"}, live
        assert not P.is_mixed(plan_routes), plan_routes
        assert set(plan_routes.values()) <= {"old", "both"}, plan_routes
        layer.invalidate()
        assert not P.unequal_routes(P.run_routes(layer, x), P.run_routes(new_twin, x))


def test_released_codes_come_back_bit_for_bit(dev):
    """packed_codes() after the release returns the bytes qvit_pack_weight wrote, from either register image."""
    x = P.layer_input("fc1").to(dev)
    for mode in ("w4r", "w8r"):
        with _wreg(mode):
            layer = P.build_layer("fc1", dev)
            plan = layer.quant_plan()
            first = plan.packed.clone()
            _warm(layer, x)
            assert plan.packed is None
            assert torch.equal(plan.packed_codes(), first)


def _reuse_address(dev, values: torch.Tensor, ptr: int, tries: int = 8):
    """A new device tensor holding `values`, at address `ptr` if the caching allocator hands that block out again
    within a few allocations of the size. Returns (tensor, whether the address repeated)."""
    kept = []
    for _ in range(tries):
        cand = values.to(dev)
        if cand.data_ptr() == ptr:
            return cand, True
        kept.append(cand)
    return kept[0], False


@pytest.mark.parametrize("which", ["bias", "weight"])
def test_replaced_parameter_at_a_recycled_address(dev, which, record_property):
    """layer.<p> = nn.Parameter(new) after the old tensor is dropped: the allocator may give the new tensor the old
    address, at version 0 like the old one. The plan holds a view of every tensor its key names, so the address
    cannot repeat while the plan lives; whether it repeated is recorded, and the routes must equal the twin's either
    way."""
    x = P.layer_input("qkv").to(dev)
    layer = P.build_layer("qkv", dev)
    _warm(layer, x)
    old = getattr(layer, which)
    ptr, values = old.data_ptr(), (old.detach() * -1.5).cpu()
    setattr(layer, which, None)
    del old
    gc.collect()
    new, repeated = _reuse_address(dev, values, ptr)
    record_property("address_repeated", repeated)
    print(f"replaced {which}: data_ptr repeated = {repeated}")
    setattr(layer, which, nn.Parameter(new))
    got = P.run_routes(layer, x)
    want = P.run_routes(P.fresh_twin(layer), x)
    assert not P.unequal_routes(got, want)


def test_deepcopy_of_a_layer_with_a_plan(dev):
    """The copy builds its own plan: it follows its own parameters and not the original's, and the original does not
    follow the copy's."""
    x = P.layer_input("qkv").to(dev)
    layer = P.build_layer("qkv", dev)
    _warm(layer, x)
    dup = copy.deepcopy(layer)
    base = P.run_routes(P.fresh_twin(layer), x)
    assert not P.unequal_routes(P.run_routes(dup, x), base)
    P.MUTATIONS["weight.mul_"][1](dup)
    dup.weight.data[1].neg_()   # and one edit the key cannot see, on top: it must not reach the original's images
    dup.invalidate()
    assert not P.unequal_routes(P.run_routes(dup, x), P.run_routes(P.fresh_twin(dup), x))
    assert not P.unequal_routes(P.run_routes(layer, x), base)
    P.MUTATIONS["bias.add_"][1](layer)
    after = P.run_routes(P.fresh_twin(dup), x)
    assert not P.unequal_routes(P.run_routes(dup, x), after)


def test_load_weight_codes_lifecycle(dev):
    """Bound codes are used on every route; any parameter edit drops them; None unbinds; a code above the saturation
    level raises."""
    x = P.layer_input("qkv").to(dev)
    layer = P.build_layer("qkv", dev)
    _warm(layer, x)
    own, _ = P.oracle_weight_codes(layer)
    codes = own.clone()
    codes[::3] = torch.where(codes[::3].abs() < 7, codes[::3] + 1, codes[::3])   # not the device's own codes
    plain = P.run_routes(P.fresh_twin(layer), x)

    layer.load_weight_codes(codes)
    got = P.run_routes(layer, x)
    twin = P.fresh_twin(layer)
    twin.load_weight_codes(codes)
    want = P.run_routes(twin, x)
    assert not P.unequal_routes(got, want)
    assert torch.equal(got["weight_codes"].cpu(), codes.float())
    assert torch.equal(got["w_fakequant"], layer.d_quant_wt.detach() * got["weight_codes"])
    assert "forward" in P.unequal_routes(got, plain)
    # the forward multiplies by exactly these codes: the float64 contraction of d_a k_a and d_w codes
    plan = layer.quant_plan()
    a = layer._act_codes(x.reshape(-1, plan.k).contiguous(), plan)[:, :plan.k].cpu().double()
    ref = (float(layer.d_quant_act) * a) @ (float(layer.d_quant_wt) * codes.double()).t() + layer.bias.detach().cpu().double()
    assert torch.allclose(got["forward"].reshape(-1, plan.n).cpu().double(), ref, rtol=P.FORWARD_RTOL,
                          atol=P.FORWARD_ATOL)

    P.MUTATIONS["bias.add_"][1](layer)            # any parameter edit drops the bound codes
    assert not P.unequal_routes(P.run_routes(layer, x), P.run_routes(P.fresh_twin(layer), x))
    layer.load_weight_codes(codes)
    layer.load_weight_codes(None)                 # None unbinds
    assert not P.unequal_routes(P.run_routes(layer, x), P.run_routes(P.fresh_twin(layer), x))
    too_big = codes.clone()
    too_big[0, 0] = 8
    layer.load_weight_codes(too_big)
    with pytest.raises(ValueError, match="saturation"):
        layer.quant_plan()
    layer.load_weight_codes(None)


def test_conv_uint8_tables_follow(dev):
    """set_uint8_input with new mean / std, a quantizer-scalar edit in between, clear_uint8_input: the value and code
    tables and the uint8 forward follow each, against a twin given the same setting."""
    x = P.layer_input("conv").to(dev)
    layer = P.build_layer("conv", dev)
    _warm(layer, x)
    steps = [lambda l: l.set_uint8_input((0.5, 0.4, 0.3), (0.25, 0.5, 0.75)),
             lambda l: P.MUTATIONS["d_quant_act.mul_"][1](l),
             lambda l: l.set_uint8_input(0.45, 0.225),
             lambda l: P.MUTATIONS["q_m_act.mul_"][1](l),
             lambda l: l.clear_uint8_input()]
    seen = []
    for i, step in enumerate(steps):
        step(layer)
        got = P.run_routes(layer, x)
        want = P.run_routes(P.fresh_twin(layer), x)
        assert not P.unequal_routes(got, want), i
        assert ("u8_codes" in got) == (layer.uint8_input is not None)
        if "u8_codes" in got:
            assert all(not torch.equal(got["u8_codes"], s) for s in seen), i   # every step moved the code table
            seen.append(got["u8_codes"])


# ---- the model: producer / consumer coupling and the fused routes -------------------------------------------------
def _quantize(m):
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType
    from quantized_vit_amd.quant_model import model_to_quantize_model
    return model_to_quantize_model(m, num_bits=4, quant_type=QuantizationType.SYMMETRIC_NONLINEAR,
                                   quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)


def _vit_factory():
    from quantized_vit_amd.vit_model import VisionTransformer
    torch.manual_seed(5)
    return _quantize(VisionTransformer(img_size=32, patch_size=16, embed_dim=256, depth=2, num_heads=4,
                                       num_classes=10))


def _vit(dev):
    from quantized_vit_amd.calibrate import collect_input_absmax, redraw_init_artifacts, set_activation_quant, \
        synthetic_images
    from quantized_vit_amd.vit_model import VisionTransformer
    torch.manual_seed(5)
    m = VisionTransformer(img_size=32, patch_size=16, embed_dim=256, depth=2, num_heads=4, num_classes=10)
    redraw_init_artifacts(m)
    img = synthetic_images(2, 32, seed=1)
    absmax = collect_input_absmax(m.eval(), img)
    m = _quantize(m)
    set_activation_quant(m, absmax, bits=8)
    return m.to(dev).eval(), img.to(dev), absmax


def _model_routes(model, img):
    """{route: logits or traced codes} of every block mode: the fused qkv + attention arm (with the class-token arm
    in the last block, and without), the residual GEMM with LayerNorm, and the unfused module route (autograd live)."""
    from quantized_vit_amd import quant_layers as QL
    from quantized_vit_amd import vit_model as V
    out = {}
    saved = (V.FUSE_RESID_LN, V.LAST_BLOCK_CLS_ONLY)
    try:
        with torch.no_grad():
            out["fused_cls"] = model(img)
            V.LAST_BLOCK_CLS_ONLY = False
            out["fused_full"] = model(img)
            V.FUSE_RESID_LN = True
            out["fused_resid_ln"] = model(img)
            V.FUSE_RESID_LN = saved[0]
            QL.CODE_TRACE = {}
            model(img)
            names = {m: n for n, m in model.named_modules()}
            for layer, codes in QL.CODE_TRACE.items():
                out["codes." + names[layer]] = codes
            QL.CODE_TRACE = None
        xi = img.clone().requires_grad_(True)
        y = model(xi)                      # every block on the module route, the attention core unfused
        y.square().sum().backward()
        out["modules"] = y.detach()
        out["modules.x.grad"] = xi.grad
        for n, p in model.named_parameters():
            if p.grad is not None:
                out["grad." + n] = p.grad.clone()
                p.grad = None
    finally:
        V.FUSE_RESID_LN, V.LAST_BLOCK_CLS_ONLY = saved
        QL.CODE_TRACE = None
    return out


def _model_twin(model):
    return P.fresh_twin_module(model, _vit_factory)


def _set_levels(model, suffix: str, which: str, level: float):
    for n, m in model.named_modules():
        if n.endswith(suffix):
            P._set_level(m, which, level)


def test_model_routes_follow_mutations(dev):
    """The ViT (dim 256, 4 heads, depth 2, N = 5) on the fused qkv + attention arm, the split pair (qkv moved to W8)
    and the module route: after each mutation every route equals the twin model's. fc2's activation scalar feeds
    fc1's epilogue code table: its in-place edit must change the codes fc1's GEMM writes."""
    from quantized_vit_amd import _lib
    from quantized_vit_amd.calibrate import QuantChoice, apply_quant_choices, set_activation_quant, set_weight_quant_t
    from quantized_vit_amd.quant_layers import QuantizeMixin
    model, img, absmax = _vit(dev)
    base = _model_routes(model, img)
    assert model.blocks[0].attn.qkv.quant_plan().wfmt == _lib.W4
    twin = _model_twin(model)
    assert not P.unequal_routes(base, _model_routes(twin, img))
    # the twin model itself, once: every quantized layer's codes against the CPU oracle's (proven ties aside). The
    # forward of these classes against the oracle end to end: tests/test_gpu_model.py (tie_resolved_vit_check).
    pinned = [P.assert_codes_match_oracle(m, m.weight_codes()) for m in twin.modules() if isinstance(m, QuantizeMixin)]
    assert len(pinned) == 4 * 2 + 2       # four linears per block, the patch embedding and the head

    def apply_choices(m):
        f = lambda p: float(p.detach().cpu().reshape(-1)[0])
        fc1, proj = m.blocks[0].mlp.fc1, m.blocks[1].attn.proj
        pick = lambda q_m, d, t: QuantChoice(q_m=q_m, d=d, t=t, err=0.0, err_absmax=0.0, clipped=0, numel=0)
        apply_quant_choices(
            m, act={"blocks.0.mlp.fc1": pick(0.75 * f(fc1.q_m_act), 1.125 * f(fc1.d_quant_act), f(fc1.t_quant_act))},
            wt={"blocks.1.attn.proj": pick(0.875 * f(proj.q_m_wt), 1.0625 * f(proj.d_quant_wt), f(proj.t_quant_wt))})

    def fc2_scalar(m):
        with torch.no_grad():
            m.blocks[0].mlp.fc2.d_quant_act.mul_(1.5)

    def weights(m):
        with torch.no_grad():
            m.blocks[0].attn.qkv.weight.mul_(1.25)
            m.blocks[1].attn.proj.weight.mul_(0.75)
            m.blocks[1].mlp.fc2.bias.add_(0.5)

    def sgd(m):
        m.train()
        opt = torch.optim.SGD(m.parameters(), lr=1e-4)
        m(img).square().mean().backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        m.eval()

    def qat(m):
        from quantized_vit_amd import QuantAwareOptimizer
        m.train()
        opt = QuantAwareOptimizer(m, variant="adamw", lr=1e-3, lr_quant=1e-4, first_momentum=0.9,
                                  second_momentum=0.999, weight_decay=1e-2, start_projection_step=0,
                                  projection_steps=8, projection_periods=4, fix_after_step=10, bit_reduction=4,
                                  min_bit_wt=4, max_bit_wt=16, min_bit_act=4, max_bit_act=16)
        opt.zero_grad()
        m(img).square().mean().backward()
        opt.step()
        m.eval()
        for p in m.parameters():
            p.grad = None

    steps = [("fc2.d_quant_act", fc2_scalar), ("weights", weights),
             ("split_pair", lambda m: _set_levels(m, "attn.qkv", "wt", 127)),
             ("calibrate", lambda m: set_activation_quant(m, {k: 1.25 * v for k, v in absmax.items()}, bits=8)),
             ("set_weight_quant_t", lambda m: set_weight_quant_t(m, 1.125, bits=4)),
             ("apply_quant_choices", apply_choices),
             ("sgd", sgd), ("load_state_dict", lambda m: m.load_state_dict(
                 {k: (v * 1.125 if k.endswith("fc1.weight") else v.clone()) for k, v in m.state_dict().items()})),
             ("qat_step", qat)]
    failures = {}
    last = base
    for name, step in steps:
        step(model)
        got = _model_routes(model, img)
        want = _model_routes(_model_twin(model), img)
        bad = P.unequal_routes(got, want)
        if bad:
            failures[name] = bad
        assert P.unequal_routes(want, last), name          # the step moved the model
        if name == "fc2.d_quant_act":
            assert not torch.equal(want["codes.blocks.0.mlp.fc2"], base["codes.blocks.0.mlp.fc2"])
        if name == "split_pair":
            assert model.blocks[0].attn.qkv.quant_plan().wfmt == _lib.W8
        last = want
    assert not failures, failures


def test_model_stale_contract(dev):
    """A `.data` edit of qkv and proj weights without invalidate(): qvit_gemm (register image), qvit_qkv_attention
    and qvit_gemm_resid_ln (packed_codes()) all keep multiplying by the old weights; invalidate() moves them."""
    model, img, _ = _vit(dev)
    old = _model_routes(_model_twin(model), img)
    with torch.no_grad():
        model(img)
    for blk in model.blocks:
        blk.attn.qkv.weight.data.mul_(1.25)
        blk.attn.proj.weight.data.mul_(-0.75)
    keep = lambda r: {k: v for k, v in r.items() if k.startswith(("fused", "codes."))}
    got = keep(_model_routes(model, img))
    new = keep(_model_routes(_model_twin(model), img))
    verdict = P.classify_routes(got, keep(old), new)
    assert P.classify_routes(new, keep(old), new)["fused_resid_ln"] == "new"
    assert not P.is_mixed(verdict) and set(verdict.values()) <= {"old", "both"}, verdict
    for m in model.modules():
        if hasattr(m, "invalidate"):
            m.invalidate()
    assert not P.unequal_routes(keep(_model_routes(model, img)), new)


# ---- UltraNet's caches ------------------------------------------------------------------------------------------
def _ultra_pair(dev):
    from quantized_vit_amd.quant_ultra import activation_quantize_fn, conv2d_Q_fn
    torch.manual_seed(3)
    conv = conv2d_Q_fn(4)(16, 32, 3, padding=1, bias=False).to(dev).eval()
    bn = nn.BatchNorm2d(32).to(dev).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.1)
        bn.running_mean.normal_(0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)
    return conv, bn, activation_quantize_fn(4)


def _ultra_twin(conv, bn, dev):
    c2, b2, act = _ultra_pair(dev)
    c2.load_state_dict({k: v.clone() for k, v in conv.state_dict().items()})
    b2.load_state_dict({k: v.clone() for k, v in bn.state_dict().items()})
    return c2, b2, act


def _ultra_routes(conv, bn, act, x):
    with torch.no_grad():
        out = {"conv": conv(x), "fused": conv.forward_bn_act(x, bn, act)}
    xr = x.clone().requires_grad_(True)
    y = conv(xr)
    y.square().sum().backward()
    out["x.grad"], out["w.grad"] = xr.grad, conv.weight.grad.clone()
    conv.weight.grad = None
    return out


def test_ultra_conv_and_bn_fold_follow(dev):
    """Conv2d_Q's packed codes and its BatchNorm fold follow in-place edits, load_state_dict, a replaced parameter
    at a recycled address, running-statistics updates in train mode and num_batches_tracked."""
    conv, bn, act = _ultra_pair(dev)
    x = (torch.randint(0, 16, (1, 16, 8, 8), generator=torch.Generator().manual_seed(1)).float() / 15).to(dev)
    _ultra_routes(conv, bn, act, x)

    def replace_weight(c, b):
        old = c.weight
        ptr, values = old.data_ptr(), (old.detach() * -0.5).cpu()
        c.weight = None
        del old
        gc.collect()
        new, repeated = _reuse_address(dev, values, ptr)
        print(f"Conv2d_Q weight: data_ptr repeated = {repeated}")
        c.weight = nn.Parameter(new)

    def replace_bn_bias(c, b):
        old = b.bias
        ptr, values = old.data_ptr(), (old.detach() + 0.5).cpu()
        b.bias = None
        del old
        gc.collect()
        new, repeated = _reuse_address(dev, values, ptr)
        print(f"BatchNorm2d bias: data_ptr repeated = {repeated}")
        b.bias = nn.Parameter(new)

    def running_stats(c, b):
        b.train()
        with torch.no_grad():
            b(torch.randn(4, 32, 8, 8, device=dev) * 2 + 1)
        b.eval()

    def inplace(c, b):
        with torch.no_grad():
            c.weight.mul_(1.5)
            b.weight.add_(0.25)

    steps = [("inplace", inplace),
             ("load_state_dict", lambda c, b: c.load_state_dict({"weight": c.weight.detach().flip(0).clone()})),
             ("replace_weight", replace_weight), ("replace_bn_bias", replace_bn_bias),
             ("running_stats", running_stats),
             ("running_var", lambda c, b: b.running_var.mul_(2.0)),
             ("num_batches_tracked", lambda c, b: b.num_batches_tracked.add_(1))]
    failures = {}
    for name, step in steps:
        before = _ultra_routes(*_ultra_twin(conv, bn, dev), x)
        step(conv, bn)
        got = _ultra_routes(conv, bn, act, x)
        want = _ultra_routes(*_ultra_twin(conv, bn, dev), x)
        bad = P.unequal_routes(got, want)
        if bad:
            failures[name] = bad
        if name != "num_batches_tracked":     # a counter the fold does not read: nothing may move
            assert P.unequal_routes(before, want), name
        else:
            assert not P.unequal_routes(before, want)
    assert not failures, failures


def test_ultranet_deploy_cache_follows(dev):
    """UltraNetQua's model-level plan (forward_fused) follows in-place edits of a conv weight, BN parameters and
    running statistics, load_state_dict and a replaced parameter, against a fresh model with the same state."""
    from quantized_vit_amd.ultranet import UltraNetQua
    torch.manual_seed(2)
    model = UltraNetQua().to(dev).eval()
    img = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(dev)
    assert model.fused_ok(img)

    def run(m):
        with torch.no_grad():
            io, (p,) = m(img)
        return {"io": io, "p": p}

    def twin(m):
        t = UltraNetQua().to(dev).eval()
        t.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
        return t

    def replace(m):
        conv = m.layers[4]
        old = conv.weight
        ptr, values = old.data_ptr(), (old.detach() * -1.0).cpu()
        conv.weight = None
        del old
        gc.collect()
        new, repeated = _reuse_address(dev, values, ptr)
        print(f"UltraNetQua layers.4.weight: data_ptr repeated = {repeated}")
        conv.weight = nn.Parameter(new)

    def inplace(m):
        with torch.no_grad():
            m.layers[0].weight.mul_(1.5)
            m.layers[5].weight.mul_(0.5)
            m.layers[1].running_mean.add_(0.05)

    steps = [("inplace", inplace), ("replace", replace),
             ("load_state_dict", lambda m: m.load_state_dict(
                 {k: (v.flip(0).clone() if k == "layers.8.weight" else v.clone()) for k, v in m.state_dict().items()}))]
    last = run(model)
    assert not P.unequal_routes(last, run(twin(model)))
    failures = {}
    for name, step in steps:
        step(model)
        got, want = run(model), run(twin(model))
        bad = P.unequal_routes(got, want)
        if bad:
            failures[name] = bad
        assert P.unequal_routes(want, last), name
        last = want
    assert not failures, failures
