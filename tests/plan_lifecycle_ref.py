"""Helpers of the plan lifecycle tests: layers at the smallest shapes that reach every route, the fresh twin, the
mutation table, the route runner and the comparers.

The yardstick is a FRESH TWIN: a new layer of the same construction, on the same device, loaded from the mutated
layer's state_dict(). A layer whose cached plan followed the mutation gives the twin's bits on every route
(torch.equal); one that did not gives the bits of a twin built before the mutation. The twin is pinned to an
independent reference once per scenario: its weight codes against oracle.quant_oracle.quant_codes of the fp32 weight
on the CPU (oracle.ties.tie_check: a differing code must be a proven rounding tie, and at most TIE_SHARE_CAP of the
codes may differ), w_fakequant against d_wt * codes exactly, and its forward against the float64 restatement of
tests/quant_backward_ref.py at the bar of tests/test_gpu_layer_autograd.py::_check_layer (rtol 1e-4, atol 1e-5).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

import quant_backward_ref as R

TIE_SHARE_CAP = 1e-3          # share of weight codes that may differ from the oracle's (each a proven tie)
FORWARD_RTOL, FORWARD_ATOL = 1e-4, 1e-5   # tests/test_gpu_layer_autograd.py::_check_layer, forward against float64
ROWS = (2, 17)                # token rows of the linear layers

PARAM_NAMES = ["weight", "bias", "d_quant_wt", "q_m_wt", "t_quant_wt", "d_quant_act", "q_m_act", "t_quant_act"]


def level_d(kind: str, q_m: float, t: Optional[float], level: float) -> float:
    """d that puts the saturation level at `level`, 0.3 of a step from a rounding tie
    (tests/test_gpu_layer_autograd.py::_level_d)."""
    rp = abs(q_m) if kind == R.LINEAR else math.exp(t * math.log(abs(q_m) + 1e-6))
    return float(np.float32(rp / (level + 0.3)))


# name -> (class, constructor arguments, quantizer kind, W+A?, seed)
LAYERS = {
    "qkv": ("linear", (256, 192), R.NONLINEAR, True, 1),       # one 64-wide head; K % 256 == 0 (the fused kernel)
    "fc1": ("linear", (256, 1024), R.NONLINEAR, True, 2),
    "fc2": ("linear", (1024, 256), R.NONLINEAR, True, 3),
    "lin": ("linear", (256, 192), R.LINEAR, True, 4),          # SYMMETRIC_LINEAR
    "wonly": ("linear", (256, 192), R.NONLINEAR, False, 5),    # WEIGHT_ONLY
    "conv": ("conv", (3, 256, 16), R.NONLINEAR, True, 6),      # the patch embedding: kernel = stride = 16
}
QM_WT, QM_ACT = 0.37, 2.545


def quantizer_scalars(kind: str, wa: bool, level_wt: float = 7, level_act: float = 127):
    tw, ta = (None, None) if kind == R.LINEAR else (1.25, 0.9)
    wq = (level_d(kind, QM_WT, tw, level_wt), QM_WT, tw)
    aq = (level_d(kind, QM_ACT, ta, level_act), QM_ACT, ta) if wa else None
    return wq, aq


def construct(name: str):
    """A new layer of LAYERS[name] on the CPU, parameters at their constructor values."""
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeConv2d, QuantizeLinear
    cls, args, kind, wa, _ = LAYERS[name]
    qt = QuantizationType.SYMMETRIC_LINEAR if kind == R.LINEAR else QuantizationType.SYMMETRIC_NONLINEAR
    qm = QuantizationMode.WEIGHT_AND_ACTIVATION if wa else QuantizationMode.WEIGHT_ONLY
    if cls == "conv":
        cin, cout, ks = args
        return QuantizeConv2d(cin, cout, ks, stride=ks, padding=0, bias=True, quant_type=qt, quant_mode=qm)
    return QuantizeLinear(*args, bias=True, quant_type=qt, quant_mode=qm)


def weight_values(name: str) -> torch.Tensor:
    """The layer's initial fp32 weight: tie-free at its initial quantizer (no code within 0.05 of a rounding tie)."""
    _, _, kind, wa, seed = LAYERS[name]
    wq, _ = quantizer_scalars(kind, wa)
    return R.tie_free_values(tuple(construct(name).weight.shape), kind, *wq, seed=100 + seed)


def build_layer(name: str, dev) -> "torch.nn.Module":
    """LAYERS[name] on `dev` in eval mode: 4-bit weights (level 7), int8 activation codes (level 127)."""
    _, _, kind, wa, seed = LAYERS[name]
    layer = construct(name)
    wq, aq = quantizer_scalars(kind, wa)
    gen = torch.Generator().manual_seed(200 + seed)
    with torch.no_grad():
        layer.weight.copy_(weight_values(name))
        layer.bias.copy_(0.1 * torch.randn(layer.bias.shape, generator=gen))
        for n, v in zip(("d_quant_wt", "q_m_wt", "t_quant_wt"), wq):
            if v is not None:
                getattr(layer, n).fill_(v)
        if aq is not None:
            for n, v in zip(("d_quant_act", "q_m_act", "t_quant_act"), aq):
                if v is not None:
                    getattr(layer, n).fill_(v)
    return layer.to(dev).eval()


def layer_input(name: str) -> torch.Tensor:
    """fp32 input on the CPU: tie-free at the layer's initial activation quantizer (normal values for weight-only)."""
    cls, args, kind, wa, seed = LAYERS[name]
    shape = (2, args[0], 32, 32) if cls == "conv" else ROWS + (args[0],)
    _, aq = quantizer_scalars(kind, wa)
    if aq is None:
        return torch.randn(shape, generator=torch.Generator().manual_seed(300 + seed))
    return R.tie_free_values(shape, kind, *aq, seed=300 + seed)


def fresh_twin(layer):
    """A new layer of the same construction on the same device and in the same mode, loaded from state_dict(); the
    uint8 setting of a conv (a plain attribute, not in the state) is set again. Shares no tensor with `layer`."""
    from quantized_vit_amd.quant_layers import QuantizeConv2d, QuantizeLinear
    dev = layer.weight.device
    if isinstance(layer, QuantizeConv2d):
        twin = QuantizeConv2d(layer.in_channels, layer.out_channels, layer.kernel_size, stride=layer.stride,
                              padding=layer.padding, dilation=layer.dilation, groups=layer.groups,
                              bias=layer.bias is not None, quant_type=layer.quant_type, quant_mode=layer.quant_mode)
    elif isinstance(layer, QuantizeLinear):
        twin = QuantizeLinear(layer.in_features, layer.out_features, bias=layer.bias is not None,
                              quant_type=layer.quant_type, quant_mode=layer.quant_mode)
    else:
        raise TypeError(type(layer).__name__)
    twin = twin.to(dev)
    twin.load_state_dict({k: v.detach().clone() for k, v in layer.state_dict().items()})
    if getattr(layer, "uint8_input", None) is not None:
        twin.set_uint8_input(*layer.uint8_input)
    twin.train(layer.training)
    mine = {p.data_ptr() for p in layer.parameters()}
    assert not mine & {p.data_ptr() for p in twin.parameters()}
    return twin


def fresh_twin_module(model, factory: Callable[[], "torch.nn.Module"]):
    """The twin of a whole model: `factory()` builds the same architecture, the state comes from `model`."""
    twin = factory().to(next(model.parameters()).device)
    twin.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
    return twin.train(model.training)


# ---- the mutation table ---------------------------------------------------------------------------------------
def _set_level(layer, which: str, level: float, redraw_seed: Optional[int] = None) -> None:
    """In-place: d_quant_<which> so that the saturation level is `level`. With `redraw_seed`, the weight is also
    overwritten in place with values that are tie-free at the NEW weight quantizer (0.05 of a code from every
    rounding tie): beyond some 2^15 levels one fp32 ulp of the nonlinear quantizer's power is more code units than
    oracle.ties.TIE_TOL, so on weights drawn for another grid two faithful implementations differ by codes that
    tie_check cannot prove ties; on the redrawn weights they do not differ at all."""
    kind = R.LINEAR if not hasattr(layer, "t_quant_wt") else R.NONLINEAR
    qm = float(getattr(layer, f"q_m_{which}").detach().cpu())
    t = float(getattr(layer, f"t_quant_{which}").detach().cpu()) if kind == R.NONLINEAR else None
    d = level_d(kind, qm, t, level)
    with torch.no_grad():
        getattr(layer, f"d_quant_{which}").fill_(d)
        if redraw_seed is not None:
            w = R.tie_free_values(tuple(layer.weight.shape), kind, d, qm, t, seed=redraw_seed)
            layer.weight.copy_(w.to(layer.weight.device))


def _inplace(name: str, op: Callable[[torch.Tensor], None]):
    def fn(layer):
        p = getattr(layer, name, None)
        if p is not None:
            with torch.no_grad():
                op(p)
    return fn


def _replace(name: str, scale: float):
    def fn(layer):
        old = getattr(layer, name)
        setattr(layer, name, torch.nn.Parameter((old.detach() * scale).clone()))
    return fn


def _load_state(layer):
    sd = {k: v.detach().clone() for k, v in layer.state_dict().items()}
    sd["weight"] = sd["weight"].flip(0)
    sd["bias"] = sd["bias"] * -1.5
    sd["d_quant_wt"] = sd["d_quant_wt"] * 1.03125
    layer.load_state_dict(sd)


def _sgd_step(layer):
    """A backward in training mode, one SGD step on every parameter, then eval()."""
    layer.train()
    opt = torch.optim.SGD(layer.parameters(), lr=1e-4)
    x = layer_input_like(layer)
    layer(x).square().mean().backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    layer.eval()


def layer_input_like(layer) -> torch.Tensor:
    """A deterministic input of the layer's own geometry on its device (the SGD mutation's batch)."""
    from quantized_vit_amd.quant_layers import QuantizeConv2d
    gen = torch.Generator().manual_seed(7)
    shape = (2, layer.in_channels, 32, 32) if isinstance(layer, QuantizeConv2d) else ROWS + (layer.in_features,)
    return torch.randn(shape, generator=gen).to(layer.weight.device)


def _data_edit_invalidate(layer):
    """The documented protocol for edits the version counters cannot see."""
    layer.weight.data.mul_(0.875)
    layer.bias.data.sub_(0.125)
    layer.invalidate()


# name -> (parameters it touches, what it does to the layer). Every entry leaves the layer in eval mode and needs no
# invalidate() from the caller (the one that edits `.data` calls it itself: that is the documented protocol).
MUTATIONS: Dict[str, Tuple[Tuple[str, ...], Callable]] = {
    "weight.mul_": (("weight",), _inplace("weight", lambda p: p.mul_(1.25))),
    "bias.add_": (("bias",), _inplace("bias", lambda p: p.add_(0.25))),
    "d_quant_wt.mul_": (("d_quant_wt",), _inplace("d_quant_wt", lambda p: p.mul_(1.0625))),
    "q_m_wt.mul_": (("q_m_wt",), _inplace("q_m_wt", lambda p: p.mul_(0.75))),
    "t_quant_wt.mul_": (("t_quant_wt",), _inplace("t_quant_wt", lambda p: p.mul_(1.03125))),
    "d_quant_act.mul_": (("d_quant_act",), _inplace("d_quant_act", lambda p: p.mul_(1.0625))),
    "q_m_act.mul_": (("q_m_act",), _inplace("q_m_act", lambda p: p.mul_(0.5))),
    "t_quant_act.mul_": (("t_quant_act",), _inplace("t_quant_act", lambda p: p.mul_(1.03125))),
    "sgd_step": (tuple(PARAM_NAMES), _sgd_step),
    "load_state_dict": (("weight", "bias", "d_quant_wt"), _load_state),
    "replace_weight": (("weight",), _replace("weight", -0.75)),
    "replace_bias": (("bias",), _replace("bias", 2.0)),
    "train_eval": ((), lambda layer: layer.train().eval()),
    "data_edit_invalidate": (("weight", "bias"), _data_edit_invalidate),
}

# storage-class moves by in-place edits: name -> (edit, (wfmt name, int_path, wonly) expected afterwards)
CLASS_MOVES = [
    ("w8", lambda l: _set_level(l, "wt", 127), ("W8", True, False)),
    ("w4", lambda l: _set_level(l, "wt", 7), ("W4", True, False)),
    ("act_wide", lambda l: _set_level(l, "act", 1000), ("W4", False, True)),          # weight-only GEMM
    ("act_int8", lambda l: _set_level(l, "act", 127), ("W4", True, False)),
    # (the wide levels also redraw the weight in place, tie-free at the new quantizer: _set_level)
    ("w16", lambda l: _set_level(l, "wt", 32000, redraw_seed=16), ("W16", False, True)),
    ("w24", lambda l: _set_level(l, "wt", 60000, redraw_seed=24), ("W24", False, True)),
    ("fp32", lambda l: _set_level(l, "wt", 100000, redraw_seed=32), (0, False, False)),
    ("back_w4", lambda l: _set_level(l, "wt", 7, redraw_seed=4), ("W4", True, False)),
]


def plan_class(plan) -> tuple:
    from quantized_vit_amd import _lib
    names = {_lib.W4: "W4", _lib.W8: "W8", _lib.W16: "W16", _lib.W24: "W24", 0: 0}
    return names[plan.wfmt], bool(plan.int_path), bool(plan.extra.get("wonly"))


# ---- routes ---------------------------------------------------------------------------------------------------
def _grads(layer, x: torch.Tensor, G: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Forward and backward of (layer(x) * G).sum() with every parameter and the input requiring grad."""
    for p in layer.parameters():
        p.grad = None
    xr = x.clone().requires_grad_(True)
    y = layer(xr)
    (y * G).sum().backward()
    out = {"y": y.detach().clone(), "x.grad": xr.grad.clone()}
    for n, p in layer.named_parameters():
        out[n + ".grad"] = p.grad.clone()
        p.grad = None
    return out


def run_routes(layer, x: torch.Tensor, weight_grads: bool = True) -> Dict[str, torch.Tensor]:
    """Every route of one layer in its current state, as {route: tensor} (routes 1, 2, 4, 5, 6 of DESIGN.md section 28). Leaves
    the layer in the mode it came in. `weight_grads`: False keeps only the input gradient of the backward routes
    (the routes that read the plan's images: dgrad through packed_t or w_fakequant); "eval" keeps every gradient of
    the eval-mode backward and runs no training-mode call (the stale tests: a training call rebuilds the plan)."""
    from quantized_vit_amd import _lib
    from quantized_vit_amd import quant_layers as QL
    from quantized_vit_amd.quant_layers import QuantizeConv2d, epilogue_table
    out: Dict[str, torch.Tensor] = {}
    was_training = layer.training
    with torch.no_grad():
        out["forward"] = layer(x)                                              # 1: through gemm_weights()
        plan = layer.quant_plan()
        if plan.int_path and plan.wfmt == _lib.W4 and not isinstance(layer, QuantizeConv2d):
            # 2: the W4 GEMM on packed_codes() (what qvit_gemm_resid_ln and qvit_qkv_attention read)
            x2 = x.reshape(-1, plan.k).contiguous()
            codes = layer._act_codes(x2, plan)
            y = torch.empty((x2.shape[0], plan.n), dtype=torch.float32, device=x.device)
            _lib.gemm(codes, x2.shape[0], plan.kpad, plan.packed_codes(), _lib.W4, plan.n, plan.npad, plan.d_act,
                      plan.d_wt, plan.bias_pad, _lib.EPI_F32, y, out_qtype=0)
            out["packed_codes_gemm"] = y.view(out["forward"].shape)
        out["weight_codes"] = layer.weight_codes()                            # 5
        out["w_fakequant"] = layer.w_fakequant(plan).reshape(plan.n, plan.k)
        out["bits"] = torch.tensor([layer.weight_bit, layer.activation_bit])
        if plan.extra.get("act_host"):                                         # 6
            for epi, key in ((_lib.EPI_I8, "epi_table"), (_lib.EPI_I8_GELU, "epi_table_gelu")):
                tab = epilogue_table(plan, epi)
                out[key] = torch.zeros(0) if tab is None else tab.clone()
        if isinstance(layer, QuantizeConv2d) and layer.uint8_input is not None:
            V, T = layer._u8_tables(plan)
            out["u8_values"] = V.clone()
            if T is not None:
                out["u8_codes"] = T.clone()
            img = (x.detach().abs() * 97).clamp(0, 255).to(torch.uint8)
            out["forward_u8"] = layer(img)
    G = torch.randn(out["forward"].shape, generator=torch.Generator().manual_seed(11)).to(x.device)
    switch = "CONV_BACKWARD_GEMM" if isinstance(layer, QuantizeConv2d) else "BACKWARD_GEMM"
    saved = getattr(QL, switch)
    # the library's convolution gradients are not bit-stable between two layers (its algorithm search), so a conv
    # runs the backward on the project's kernels only
    modes = ("hip",) if isinstance(layer, QuantizeConv2d) else ("hip", "torch")
    try:
        for mode in modes:                                                     # 4
            setattr(QL, switch, mode)
            runs = [("eval", False)] + ([("train", True)] if weight_grads is True else [])
            for label, training in runs:
                layer.train(training)
                for k, v in _grads(layer, x, G).items():
                    if weight_grads or k in ("y", "x.grad"):
                        out[f"{label}.{mode}.{k}"] = v
    finally:
        setattr(QL, switch, saved)
        layer.train(was_training)
    return out


# ---- comparers ------------------------------------------------------------------------------------------------
def unequal_routes(got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor]) -> List[str]:
    """Routes whose tensors differ in any bit that torch.equal sees (or that only one side has)."""
    bad = [k for k in sorted(set(got) | set(want)) if k not in got or k not in want]
    for k in sorted(set(got) & set(want)):
        a, b = got[k], want[k]
        if a.shape != b.shape or a.dtype != b.dtype or not torch.equal(a.cpu(), b.cpu()):
            bad.append(k)
    return bad


def classify_routes(got: Dict[str, torch.Tensor], old: Dict[str, torch.Tensor], new: Dict[str, torch.Tensor]):
    """{route: "old" | "new" | "both" | "neither"} for the routes of `got`: whose bits each route answers with.
    "both": the mutation did not move that route (it tells nothing)."""
    verdict = {}
    for k, v in got.items():
        eq_old = k in old and not unequal_routes({k: v}, {k: old[k]})
        eq_new = k in new and not unequal_routes({k: v}, {k: new[k]})
        verdict[k] = "both" if eq_old and eq_new else "old" if eq_old else "new" if eq_new else "neither"
    return verdict


def is_mixed(verdict: Dict[str, str]) -> bool:
    """A set of routes is mixed unless all of them can be read as answering for ONE parameter state."""
    seen = {v for v in verdict.values() if v != "both"}
    return "neither" in seen or len(seen) > 1


# ---- the twin's own reference ---------------------------------------------------------------------------------
def oracle_weight_codes(layer) -> Tuple[torch.Tensor, dict]:
    """(the oracle's codes of the layer's current fp32 weight, quantizer arguments for tie_check), on the CPU."""
    from oracle import quant_oracle as O
    kind = O.NONLINEAR if hasattr(layer, "t_quant_wt") else O.LINEAR
    f = lambda p: float(p.detach().cpu().reshape(-1)[0])
    q = dict(q_type=kind, d=f(layer.d_quant_wt), q_m=f(layer.q_m_wt),
             t=f(layer.t_quant_wt) if kind == O.NONLINEAR else 1.0)
    w = layer.weight.detach().cpu().reshape(layer.weight.shape[0], -1)
    return O.quant_codes(w, q["q_type"], q["d"], q["q_m"], q["t"]), q


def codes_tie_stats(w: torch.Tensor, got: torch.Tensor, own: torch.Tensor, q: dict) -> dict:
    from oracle.ties import tie_check
    return tie_check(w, got.cpu().reshape(own.shape), own, q["q_type"], q["d"], q["q_m"], q["t"])


def codes_proven(st: dict) -> bool:
    """oracle.ties.tie_check's verdict on a set of codes: every code that differs from the oracle's is a proven
    rounding tie, and at most TIE_SHARE_CAP of the codes differ."""
    return st["non_ties"] == 0 and st["flips"] <= TIE_SHARE_CAP * st["total"]


def assert_codes_match_oracle(layer, got: torch.Tensor) -> dict:
    own, q = oracle_weight_codes(layer)
    w = layer.weight.detach().cpu().reshape(own.shape)
    st = codes_tie_stats(w, got, own, q)
    assert codes_proven(st), st
    return st


def _act_values64(layer, x: torch.Tensor) -> torch.Tensor:
    """float64 d_act * codes of the layer's activation quantizer on x: the device's own codes (qvit_fake_quant_f32,
    the quant_code every route shares), each checked against the oracle's like the weight codes: a differing code
    must be a proven rounding tie, at most TIE_SHARE_CAP of them (oracle.ties adopts the device's code the same way)."""
    from oracle import quant_oracle as O
    kind = O.NONLINEAR if hasattr(layer, "t_quant_act") else O.LINEAR
    f = lambda p: float(p.detach().cpu().reshape(-1)[0])
    d, qm = f(layer.d_quant_act), f(layer.q_m_act)
    t = f(layer.t_quant_act) if kind == O.NONLINEAR else 1.0
    with torch.no_grad():
        got = (layer.quantize_act(x.float()) / layer.d_quant_act.detach()).round().cpu()
    xc = x.detach().cpu()
    own = O.quant_codes(xc, kind, d, qm, t)
    st = codes_tie_stats(xc, got, own, dict(q_type=kind, d=d, q_m=qm, t=t))
    assert codes_proven(st), st
    return float(np.float32(d)) * got.double().reshape(x.shape)


def forward_ref64(layer, x: torch.Tensor, weight_codes: torch.Tensor) -> torch.Tensor:
    """The float64 restatement of the layer's forward on the CPU: F.linear / F.conv2d of d_a k_a and d_w k_w, the
    codes being the ones already proven equal to the oracle's or rounding ties of them (on inputs that are not
    tie-free, float64 and float32 quantizers round a tie apart, which says nothing about the contraction)."""
    import torch.nn.functional as F
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizeConv2d
    d_w = float(layer.d_quant_wt.detach().cpu().reshape(-1)[0])
    w = (d_w * weight_codes.cpu().double()).reshape(layer.weight.shape)
    xq = x.detach().cpu().double()
    if layer.quant_mode == QuantizationMode.WEIGHT_AND_ACTIVATION:
        xq = _act_values64(layer, x)
    b = layer.bias.detach().cpu().double()
    if isinstance(layer, QuantizeConv2d):
        return F.conv2d(xq, w, b, layer.stride, layer.padding, layer.dilation, layer.groups)
    return F.linear(xq, w, b)


def assert_twin_pinned(twin, x: torch.Tensor, routes: Dict[str, torch.Tensor]) -> None:
    """The twin against its independent references (module docstring): codes, w_fakequant, forward."""
    assert_codes_match_oracle(twin, routes["weight_codes"])
    d = twin.d_quant_wt.detach().reshape(1).float()
    assert torch.equal(routes["w_fakequant"], d * routes["weight_codes"])
    ref = forward_ref64(twin, x, routes["weight_codes"])
    assert torch.allclose(routes["forward"].cpu().double(), ref, rtol=FORWARD_RTOL, atol=FORWARD_ATOL)
