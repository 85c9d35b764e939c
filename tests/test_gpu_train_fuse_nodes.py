"""layernorm_linear / gelu_linear (one autograd node around pre-op + quantizer + contraction) and the TRAIN_FUSE
route of a Block, on the device.

Node gradients are checked against the float64 graph F.layer_norm / F.gelu -> reference quantizer -> matmul. The
bounds are those of the parts: the kernel tests' C max(|ref32 - ref64|, floor) for the fused pre-op backward, with
the backward GEMMs' bound of tests/test_gpu_layer_backward_gemm.py (4 n u sum |G| |operand|, u = 2^-24) carried
through the pre-op's (linear) backward in absolute values."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import quant_backward_ref as R
import test_gpu_layer_autograd as LA
import train_fuse_ref as T
from test_gpu_train_fuse import C_GELU, C_LN

pytestmark = pytest.mark.gpu

CLIP = LA.CLIP
SHAPES = [(10, 64, 48), (70, 192, 1000)]   # (M, K, N)
U = 2.0 ** -24


def _quantizers(kind):
    tw, ta = (None, None) if kind == R.LINEAR else (1.25, 0.9)
    return (LA._level_d(kind, 0.37, tw, 7), 0.37, tw), (LA._level_d(kind, 0.37, ta, 7), 0.37, ta)


def _layer(dev, kind, K, N, mode="wa"):
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeLinear
    wq, aq = _quantizers(kind)
    qt = QuantizationType.SYMMETRIC_LINEAR if kind == R.LINEAR else QuantizationType.SYMMETRIC_NONLINEAR
    qm = QuantizationMode.WEIGHT_AND_ACTIVATION if mode == "wa" else QuantizationMode.WEIGHT_ONLY
    layer = QuantizeLinear(K, N, bias=True, quant_type=qt, quant_mode=qm).to(dev).eval()
    W = R.tie_free_values((N, K), kind, *wq, seed=11)
    b = 0.1 * torch.randn(N, generator=torch.Generator().manual_seed(12))
    layer.weight.data.copy_(W)
    layer.bias.data.copy_(b)
    for name, v in zip(("d_quant_wt", "q_m_wt", "t_quant_wt"), wq):
        LA._set(getattr(layer, name, None), v)
    if mode == "wa":
        for name, v in zip(("d_quant_act", "q_m_act", "t_quant_act"), aq):
            LA._set(getattr(layer, name, None), v)
    layer.invalidate()
    return layer, W, b, wq, aq


def _case(dev, kind, shape, pre, mode="wa"):
    M, K, N = shape
    layer, W, b, wq, aq = _layer(dev, kind, K, N, mode)
    if pre == "ln":
        x, gamma, beta, _, frac = T.ln_inputs(M, K, kind, *aq, CLIP, seed=3)
        norm = nn.LayerNorm(K, eps=T.LN_EPS).to(dev)
        norm.weight.data.copy_(gamma)
        norm.bias.data.copy_(beta)
    else:
        x, _, frac = T.gelu_inputs(M * K, kind, *aq, CLIP, seed=3)
        x, norm, gamma, beta = x.view(M, K), None, None, None
    assert frac >= 0.9
    Gw = torch.randn(M, N, generator=torch.Generator().manual_seed(99))
    return layer, norm, x, gamma, beta, W, b, wq, aq, Gw


def _apply(layer, norm, xd):
    from quantized_vit_amd import quant_layers as ql
    return ql.layernorm_linear(norm, layer, xd) if norm is not None else ql.gelu_linear(layer, xd)


def _reference(kind, pre, x, gamma, beta, W, b, wq, aq, Gw):
    leaf = lambda v: None if v is None else torch.tensor([float(torch.tensor(v, dtype=torch.float32))],
                                                         dtype=torch.float64, requires_grad=True)
    xr, Wr, br = (t.double().requires_grad_(True) for t in (x, W, b))
    gr = None if gamma is None else gamma.double().requires_grad_(True)
    btr = None if beta is None else beta.double().requires_grad_(True)
    pw, pa = [leaf(v) for v in wq], [leaf(v) for v in aq]
    rec_w, rec_a = {}, {}
    a = F.layer_norm(xr, (x.shape[1],), gr, btr, T.LN_EPS) if pre == "ln" else F.gelu(xr)
    xq = R.RefQuantizer.apply(a, pa[0], pa[1], pa[2], kind, CLIP, rec_a)
    wq_ = R.RefQuantizer.apply(Wr, pw[0], pw[1], pw[2], kind, CLIP, rec_w)
    y = xq @ wq_.t() + br
    (y * Gw.double()).sum().backward()
    return dict(x=xr, W=Wr, b=br, gamma=gr, beta=btr, pw=pw, pa=pa, rec_w=rec_w, rec_a=rec_a, xq=xq.detach(),
                wq=wq_.detach())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pre", ["ln", "gelu"])
@pytest.mark.parametrize("kind", [R.LINEAR, R.NONLINEAR])
def test_node_gradients_match_float64(dev, kind, pre, shape):
    from quantized_vit_amd import _lib
    M, K, N = shape
    layer, norm, x, gamma, beta, W, b, wq, aq, Gw = _case(dev, kind, shape, pre)
    xd = x.to(dev).requires_grad_(True)
    y = _apply(layer, norm, xd)
    assert type(y.grad_fn).__name__.startswith("_PreOpLinearFunction")
    # the forward: gemm_codes on the kernel's own codes, bit for bit
    plan = layer.quant_plan()
    codes = torch.empty((M, plan.kpad), dtype=torch.int8, device=dev)
    with torch.no_grad():
        if pre == "ln":
            _lib.layernorm_quant_i8(xd.detach(), norm.weight.detach(), norm.bias.detach(), T.LN_EPS, plan.qtype,
                                    plan.d_act, plan.qm_act, plan.t_act, 0, codes, plan.kpad)
        else:
            _lib.gelu_quant_i8(xd.detach(), plan.qtype, plan.d_act, plan.qm_act, plan.t_act, 0, codes, plan.kpad)
        want = layer.gemm_codes(codes, plan, _lib.EPI_F32)[:, :N]
    assert torch.equal(y.detach(), want)
    (y * Gw.to(dev)).sum().backward()

    ref = _reference(kind, pre, x, gamma, beta, W, b, wq, aq, Gw)
    G = Gw.double()
    e = 4 * N * U * (G.abs() @ ref["wq"].abs())            # dgrad's bound, elementwise on grad_y
    g_act = ref["rec_a"]["grad_out"]                       # the grad_y of the float64 graph
    checks = [("bias.grad", layer.bias.grad, ref["b"].grad, 4 * M * U * G.abs().sum(0)),
              ("weight.grad", layer.weight.grad, ref["W"].grad, 4 * M * U * (G.abs().t() @ ref["xq"].abs()))]
    if pre == "ln":
        r64 = T.ln_quant_backward_ref(x, gamma, beta, g_act, kind, *aq, CLIP)
        r32 = T.ln_quant_backward_ref(x, gamma, beta, g_act.float(), kind, *aq, CLIP, dtype=torch.float32)
        ea = gamma.double().abs() * e * (~r64["masked"])
        xh, m = r64["xhat"].abs(), (lambda v: v.mean(-1, keepdim=True))
        fg, fb = T.ln_col_floors(r64)
        bnd = lambda k, fl: C_LN * torch.maximum((r32[k].double() - r64[k]).abs(), fl)
        checks += [("input.grad", xd.grad, ref["x"].grad,
                    bnd("grad_x", T.ln_grad_x_floor(r64, gamma)) + r64["rstd"] * (ea + m(ea) + xh * m(ea * xh))),
                   ("norm.weight.grad", norm.weight.grad, ref["gamma"].grad,
                    bnd("grad_gamma", fg) + (e * (~r64["masked"]) * xh).sum(0)),
                   ("norm.bias.grad", norm.bias.grad, ref["beta"].grad,
                    bnd("grad_beta", fb) + (e * (~r64["masked"])).sum(0))]
        floors = T.sum_floors(r64, g_act, kind, *aq, T.ln_input_delta(r64, gamma, beta))
        c = C_LN
    else:
        r64 = T.gelu_quant_backward_ref(x, g_act, kind, *aq, CLIP)
        r32 = T.gelu_quant_backward_ref(x, g_act.float(), kind, *aq, CLIP, dtype=torch.float32)
        fl = T.gelu_grad_h_floor(r64, x)
        bound = C_GELU * torch.maximum((r32["grad_h"].double() - r64["grad_h"]).abs(), fl) \
            + r64["slope"].abs() * e.reshape(-1) * (~r64["masked"])
        checks += [("input.grad", xd.grad.reshape(-1), ref["x"].grad.reshape(-1), bound)]
        floors = T.sum_floors(r64, g_act, kind, *aq, T.gelu_input_delta(r64, x))
        c = C_GELU
    for name, got, want_, bound in checks:
        err = (got.detach().cpu().double() - want_).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{pre} {kind} {shape} {name}: max err {float(err.max()):.3e}, worst err / bound {worst:.4f}")
        assert bool((err <= bound).all()), (name, float(err.max()), worst)
    # the six quantizer scalars: the weight quantizer as in the layer tests; the activation quantizer with the
    # fused kernel's floors plus dgrad's bound through each term
    _, _, _, wb = R.sum_bounds(W.reshape(-1), ref["rec_w"]["grad_out"].reshape(-1).float(), kind, *wq, clip=CLIP)
    for i, name in enumerate(("d_quant", "q_m", "t_quant")):
        p = getattr(layer, f"{name}_wt", None)
        if p is not None:
            assert abs(float(p.grad) - float(ref["pw"][i].grad)) <= wb[i], (name, "wt")
        p = getattr(layer, f"{name}_act", None)
        if p is not None:
            s32, s64 = float(r32["sums"][i]), float(r64["sums"][i])
            bound = c * max(abs(s32 - s64), floors[i]) + float((e.reshape(-1) * r64["q"]["terms"][i].abs()).sum())
            err = abs(float(p.grad) - float(ref["pa"][i].grad))
            print(f"{pre} {kind} {shape} {name}_act.grad: err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (name, "act", err, bound)


def _spy(monkeypatch, name):
    from quantized_vit_amd import _lib
    calls, orig = [], getattr(_lib, name)

    def wrapped(*a, **k):
        calls.append(name)
        return orig(*a, **k)
    monkeypatch.setattr(_lib, name, wrapped)
    return calls


@pytest.mark.parametrize("pre", ["ln", "gelu"])
def test_frozen_operands_skip_their_launches(dev, monkeypatch, pre):
    names = ("gemm_wonly", "gemm_wgrad", "layernorm_quant_backward", "gelu_quant_backward", "quant_backward",
             "quantize_act_i8")
    fused = "layernorm_quant_backward" if pre == "ln" else "gelu_quant_backward"
    for freeze in ("none", "weight", "input"):
        layer, norm, x, *_ , Gw = _case(dev, R.LINEAR, SHAPES[0], pre)
        if freeze == "weight":
            for n in ("weight", "d_quant_wt", "q_m_wt"):
                getattr(layer, n).requires_grad_(False)
        if freeze == "input":
            for n in ("d_quant_act", "q_m_act"):
                getattr(layer, n).requires_grad_(False)
            if norm is not None:
                norm.weight.requires_grad_(False)
                norm.bias.requires_grad_(False)
        xd = x.to(dev).requires_grad_(freeze != "input")
        y = _apply(layer, norm, xd)
        with monkeypatch.context() as mp:
            calls = {n: _spy(mp, n) for n in names}
            (y * Gw.to(dev)).sum().backward()
            n = {k: len(v) for k, v in calls.items()}
        assert n["quantize_act_i8"] == 0                       # wgrad reads the saved codes: no recompute
        assert n["gemm_wonly"] == n[fused] == (0 if freeze == "input" else 1), (freeze, n)
        assert n["gemm_wgrad"] == n["quant_backward"] == (0 if freeze == "weight" else 1), (freeze, n)
        assert layer.bias.grad is not None


@pytest.mark.parametrize("pre", ["ln", "gelu"])
@pytest.mark.parametrize("why", ["weight_only", "bwd_gemm_torch", "cols_mod_4"])
def test_ineligible_pairs_compose_the_modules(dev, monkeypatch, pre, why):
    """Same values as the modules route, bit for bit, and no error."""
    from quantized_vit_amd import quant_layers as ql
    shape = (10, 66, 48) if why == "cols_mod_4" else SHAPES[0]
    layer, norm, x, *_, Gw = _case(dev, R.LINEAR, shape, pre, mode="w" if why == "weight_only" else "wa")
    if why == "bwd_gemm_torch":
        monkeypatch.setattr(ql, "BACKWARD_GEMM", "torch")
    params = [p for p in list(layer.parameters()) + ([] if norm is None else list(norm.parameters()))]

    def run(fn):
        for p in params:
            p.grad = None
        xd = x.to(dev).requires_grad_(True)
        y = fn(xd)
        (y * Gw.to(dev)).sum().backward()
        return [y.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in params]
    got = run(lambda xd: _apply(layer, norm, xd))
    want = run(lambda xd: layer(norm(xd)) if norm is not None else layer(F.gelu(xd)))
    for a, b_ in zip(got, want):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("pre", ["ln", "gelu"])
def test_nan_gradient_raises(dev, pre):
    from quantized_vit_amd.quant_layers import NanInGradientError
    layer, norm, x, *_, Gw = _case(dev, R.LINEAR, SHAPES[0], pre)
    y = _apply(layer, norm, x.to(dev).requires_grad_(True))
    Gw = Gw.clone()
    Gw[2, 3] = float("nan")
    with pytest.raises(NanInGradientError):
        y.backward(Gw.to(dev))


# ---- a tiny ViT ---------------------------------------------------------------------------------------------------
# Worst per-parameter max|g_fused - g_modules| / max|g_modules| on the MI355X; the cap is four
# times the measured value rounded up to a power of two.
TINY_VIT_MEASURED = 1.371e-4       # blocks.1.mlp.fc1.d_quant_act; 0 of 33408 traced activation codes differed
TINY_VIT_CAP = 2.0 ** -10          # 4 * 1.371e-4 = 5.48e-4 -> 9.77e-4


def _tiny_vit(dev):
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType
    from quantized_vit_amd.quant_model import model_to_quantize_model
    from quantized_vit_amd.vit_model import VisionTransformer
    torch.manual_seed(0)
    model = VisionTransformer(img_size=32, patch_size=16, embed_dim=192, depth=2, num_heads=3, num_classes=10)
    model = model_to_quantize_model(model.to(dev), num_bits=4, quant_type=QuantizationType.SYMMETRIC_LINEAR,
                                    quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION).eval()
    return model, torch.randn(2, 3, 32, 32, device=dev)


def _run(model, x, trace=False):
    from quantized_vit_amd import quant_layers as ql
    model.zero_grad(set_to_none=True)
    ql.CODE_TRACE = {} if trace else None
    try:
        logits = model(x)
        codes = dict(ql.CODE_TRACE or {})
    finally:
        ql.CODE_TRACE = None
    logits.sum().backward()
    return logits.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, codes


def test_switch_off_is_the_parent_behaviour(dev, monkeypatch):
    """TRAIN_FUSE off: logits and every gradient equal, bit for bit, the run of the Block.forward this change found
    (the modules composed in place), which never looks at the switch."""
    from quantized_vit_amd import vit_model as vm
    assert vm.TRAIN_FUSE is False   # the default
    model, x = _tiny_vit(dev)
    off = _run(model, x)

    def parent_forward(self, x):
        if self.fused_ok(x):
            return self.forward_fused_(x.contiguous().clone())
        x = x + self.drop_path(self.attn(self.norm1(x)))
        return x + self.drop_path(self.mlp(self.norm2(x)))
    monkeypatch.setattr(vm.Block, "forward", parent_forward)
    parent = _run(model, x)
    assert torch.equal(off[0], parent[0])
    for n in parent[1]:
        assert torch.equal(off[1][n], parent[1][n]), n


def test_tiny_vit_fused_route_against_modules(dev, monkeypatch):
    from quantized_vit_amd import vit_model as vm
    model, x = _tiny_vit(dev)
    _, g_mod, c_mod = _run(model, x, trace=True)
    monkeypatch.setattr(vm, "TRAIN_FUSE", True)
    _, g_fus, c_fus = _run(model, x, trace=True)
    assert set(g_fus) == set(g_mod) and all(g is not None and bool(torch.isfinite(g).all()) for g in g_fus.values())
    differ = sum(int((c_mod[k] != c_fus[k]).sum()) for k in c_mod)
    total = sum(v.numel() for v in c_mod.values())
    assert set(c_mod) == set(c_fus)
    worst, where = 0.0, None
    for n, g in g_mod.items():
        scale, diff = float(g.abs().max()), float((g_fus[n] - g).abs().max())
        rel = diff / scale if scale > 0 else (0.0 if diff == 0 else float("inf"))
        print(f"  {n}: {rel:.3e}")
        if rel > worst:
            worst, where = rel, n
    print(f"tiny ViT, fused vs modules route: worst per-parameter relative difference {worst:.3e} ({where}); "
          f"{differ} of {total} traced activation codes differ")
    assert worst <= TINY_VIT_CAP, (worst, where)


def test_fused_route_saves_codes_not_fp32(dev, monkeypatch):
    """Saved-tensor bytes per block under saved_tensors_hooks: the fused route saves int8 codes where the modules
    route saves the fp32 LayerNorm and GELU outputs."""
    from quantized_vit_amd import vit_model as vm
    model, x = _tiny_vit(dev)
    blk = model.blocks[0]
    xin = torch.randn(2, 5, 192, device=dev)
    M, C, H = 10, 192, blk.mlp.fc1.out_features
    def measure():
        seen = {}   # distinct saved tensors: (address, dtype, shape) -> bytes

        def pack(t):
            seen[(t.data_ptr(), t.dtype, tuple(t.shape))] = t.numel() * t.element_size()
            return t
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            y = blk(xin.clone().requires_grad_(True))
        y.sum().backward()
        return sum(seen.values()), [(dt, sh) for _, dt, sh in seen]
    b_mod, s_mod = measure()
    monkeypatch.setattr(vm, "TRAIN_FUSE", True)
    b_fus, s_fus = measure()
    kpads = sum(l.quant_plan().kpad for l in (blk.attn.qkv, blk.mlp.fc1, blk.mlp.fc2))
    want = M * (4 * (2 * C + H) - kpads) - 64 * M
    print(f"saved bytes per block: modules {b_mod}, fused {b_fus}, difference {b_mod - b_fus} (required >= {want})")
    assert b_mod - b_fus >= want
    # of the fp32 tensors shaped like a LayerNorm output, the fused route saves exactly two fewer (the outputs of
    # norm1 and norm2; what remains are the residual stream entering the norms and proj's input, saved by both), and
    # none of the MLP's hidden shape but fc1's output itself; int8 codes appear only on the fused route
    shaped = lambda s, last: sum(1 for dt, sh in s if dt == torch.float32 and sh[-1] == last
                                 and sh[:-1] in ((2, 5), (10,)))
    assert shaped(s_mod, C) - shaped(s_fus, C) == 2
    assert shaped(s_mod, H) - shaped(s_fus, H) == 1 and shaped(s_fus, H) == 1
    assert any(dt == torch.int8 for dt, _ in s_fus) and not any(dt == torch.int8 for dt, _ in s_mod)
