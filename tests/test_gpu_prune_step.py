"""The pruning stages of QuantAwareOptimizer on the device against tests/prune_step_ref.py: the saliency sums and
scores, a joint pruning and quantization step with every branch of compute_gamma_d, the whole schedule on a two-block
ViT with a mid-period checkpoint, the constructor's rejections, and compress_pruned_mlp on the integer path.

Shapes: three groups of 8, 33 and 70 rows, member widths 48 and 130 (no multiple of 4: the scalar path) plus the
biases (width 1); l2.weight starts 4 bytes into its storage (the 16-byte path must fall back).

Tolerances. The row sums are double accumulations of fp32 inputs: N 2^-53 sum|terms| against float64 (N the row's
element count) for all three sums in every variant; the fp32 gradient variant they are taken over is rebuilt bit for
bit from the moments the boundary step stored (device_grad_variant). gamma, d and the redundant rows: 4 x the
largest difference between the reference's fp32 torch form and its float64 form on the same inputs (neither is the
code under test), never below 1 fp32 ulp of the value, as tests/test_gpu_qat_step.py does."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import prune_step_ref as R
from prune_step_ref import Group, PruneF64, PruneHyper, PruneTorch

pytestmark = pytest.mark.gpu
ROWS, WIDTHS = (8, 33, 70), (48, 130, 48)
U24 = 2.0 ** -24


class Net(nn.Module):
    def __init__(self, nonlinear=True):
        super().__init__()
        from quantized_vit_amd import QuantizationMode as M, QuantizationType as T, QuantizeLinear
        qt = T.SYMMETRIC_NONLINEAR if nonlinear else T.SYMMETRIC_LINEAR
        for i, (r, w) in enumerate(zip(ROWS, WIDTHS)):
            setattr(self, f"l{i}", QuantizeLinear(w, r, bias=True, quant_type=qt, quant_mode=M.WEIGHT_AND_ACTIVATION))
        self.other = nn.Parameter(torch.zeros(5, 7))


def make_net(dev, seed=0, nonlinear=True):
    g = torch.Generator().manual_seed(seed)
    net = Net(nonlinear).to(dev)
    net.l2.weight = nn.Parameter(torch.zeros(ROWS[2] * WIDTHS[2] + 1, device=dev)[1:].view(ROWS[2], WIDTHS[2]))
    assert net.l2.weight.data_ptr() % 16 == 4 and net.l2.weight.is_contiguous()
    with torch.no_grad():
        for name, p in net.named_parameters():
            leaf = name.split(".")[-1]
            if leaf.startswith("q_m"):
                v = 0.9 + 0.2 * torch.rand(1, generator=g)
            elif leaf.startswith("t_quant"):
                v = 0.95 + 0.1 * torch.rand(1, generator=g)
            elif leaf.startswith("d_quant"):
                v = (1.0 + 0.1 * torch.rand(1, generator=g)) / 127.0
            else:
                v = torch.randn(p.shape, generator=g) * 0.3
            p.copy_(v.to(dev))
    return net


def host_params(net):
    return {n: p.detach().cpu().clone() for n, p in net.named_parameters()}


def make_grads(params, seed, scale=0.05):
    g = torch.Generator().manual_seed(1000 + seed)
    return {k: torch.randn(v.shape, generator=g) * scale for k, v in params.items()}


def set_grads(net, grads, dev):
    for name, p in net.named_parameters():
        p.grad = grads[name].to(dev)


def dev_groups(net):
    from quantized_vit_amd import PruneGroup
    return [PruneGroup(f"g{i}", getattr(net, f"l{i}"), [getattr(net, f"l{i}").weight, getattr(net, f"l{i}").bias])
            for i in range(3)]


def ref_groups():
    return [Group(f"g{i}", f"l{i}", [f"l{i}.weight", f"l{i}.bias"]) for i in range(3)]


def make_opt(net, **kw):
    from quantized_vit_amd import QuantAwareOptimizer
    return QuantAwareOptimizer(net, prune_groups=dev_groups(net), **kw)


VARIANTS = {
    "sgd_plain": dict(variant="sgd"),
    "sgd": dict(variant="sgd", first_momentum=0.9, dampening=0.1, weight_decay=1e-2),
    "adam": dict(variant="adam", first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2),
    "adamw": dict(variant="adamw", first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2),
}
BASE = dict(lr=1e-2, lr_quant=1e-3, start_projection_step=0, projection_steps=2, min_bit_wt=4, max_bit_wt=16)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


# ---- scores -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("later", [False, True], ids=["first_step", "later_step"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_scores_against_float64(dev, variant, later):
    # first-step moments: the boundary falls on step 1 (period 1: (1 - 1 - 1) % 1 == 0); later: on step 2
    sched = dict(start_pruning_step=1, pruning_steps=3 if later else 1, pruning_periods=1)
    kw = dict(BASE, **VARIANTS[variant], **sched)
    net = make_net(dev, 1)
    start = host_params(net)
    opt = make_opt(net, **kw)
    ref = PruneTorch(start, PruneHyper(**kw), ref_groups())
    f64 = PruneF64({k: v.numpy() for k, v in start.items()}, PruneHyper(**kw), ref_groups())
    for s in range(2 if later else 1):
        if s == (1 if later else 0):
            before = host_params(net)   # the device's own parameters as the boundary step finds them
        g = make_grads(start, s)
        set_grads(net, g, dev)
        opt.step()
        ref.step(g)
        f64.step({k: v.numpy() for k, v in g.items()})
    assert ref.curr_period == 1 and opt._prune.curr_period == 1
    sums = opt._prune._sums.cpu().numpy()
    scores = opt._prune._scores.cpu().numpy().astype(np.float64)
    gv_dev = device_grad_variant(opt, variant, g)
    row0, per_group, tols = 0, [], []
    for gr in ref.groups:
        n = sum(before[m][0].numel() for m in gr.members)
        p = torch.cat([before[m].reshape(gr.num_groups, -1) for m in gr.members], dim=1).double().numpy()
        gv = np.concatenate([gv_dev[m].reshape(gr.num_groups, -1) for m in gr.members], axis=1).astype(np.float64)
        want = np.stack([(p * p).sum(1), (gv * gv).sum(1), (p * gv).sum(1)], axis=1)
        absum = np.stack([(p * p).sum(1), (gv * gv).sum(1), np.abs(p * gv).sum(1)], axis=1)
        tol = n * 2.0 ** -53 * absum
        got = sums[row0:row0 + gr.num_groups]
        err = np.abs(got - want)
        print(f"{gr.name}: sums max err/tol {np.max(err / np.maximum(tol, 1e-300)):.3f}")
        assert (err <= tol).all(), (gr.name, float(np.max(err / tol)))
        per_group.append(R.criteria_f64(want[:, 0], want[:, 1], want[:, 2], n))
        # a criterion's relative error is at most twice that of the sum it is made of; sum p g's is the bound
        # times its condition sum|p g| / |sum p g|
        tols.append(2 * n * 2.0 ** -53 * np.maximum(1.0, absum[:, 2] / np.maximum(np.abs(want[:, 2]), 1e-300)))
        row0 += gr.num_groups
    want_scores = np.concatenate(R.overall_scores(per_group, R.DEFAULT_CRITERIA))
    # five terms and their normalisers on top of the criteria (x 4), and the rounding of the result to fp32
    score_tol = 4 * np.concatenate(tols) + U24
    rel = np.abs(scores[:row0] - want_scores) / np.abs(want_scores)
    print(f"scores: max rel err {rel.max():.3e}, tol {score_tol.min():.3e} .. {score_tol.max():.3e}")
    assert (rel <= score_tol).all()
    assert [sorted(x.active) for x in opt._prune.groups] == [sorted(x.active) for x in f64.groups]


def device_grad_variant(opt, variant, grads):
    """The gradient variant the boundary step's kernels formed, rebuilt bit for bit from what that step stored: the
    same per-element function runs in the scores kernel and in the member update, which leaves m' and v' in the
    optimizer's moment buffers. sgd with momentum: m'. adam, adamw: (m' / bc1) / (sqrt(v' / bc2) + 1e-8), five
    correctly rounded fp32 operations, which NumPy's float32 repeats. Plain sgd: the gradient itself."""
    f = np.float32
    out = {}
    for di in opt._prune.member_dense:
        name = opt._dense[di][0]
        if variant == "sgd_plain":
            out[name] = grads[name].numpy()
            continue
        m = opt._m[di].cpu().numpy()
        if variant == "sgd":
            out[name] = m
            continue
        v = opt._v[di].cpu().numpy()
        hp = opt.param_groups[0]
        bc1 = f(1.0 - hp["first_momentum"] ** opt.num_steps)
        bc2 = f(1.0 - hp["second_momentum"] ** opt.num_steps)
        out[name] = (m / bc1) / (np.sqrt(v / bc2) + f(1e-8))
        assert out[name].dtype == np.float32
    return out


# ---- the joint step ---------------------------------------------------------------------------------------------
REDUNDANT = {"single": ([3], [17], [40]), "scattered": ([0, 2, 7], [1, 5, 8, 13, 32], [0, 9, 33, 34, 69]),
             "all_but_divisible": (list(range(7)), list(range(32)), list(range(69)))}
PRUNED = ([], [30], [2, 68])


COEFF = {"pos": (0.3, -0.3), "neg": (-0.3, -0.3), "mean": (0.3, -0.3), "zero": (0.0, 0.0), "res_pos": (0.3, 0.3),
         "loop": (2e-4, -2e-4), "min": (3.0, -0.3)}


def joint_grads(start, redundant, kind, seed):
    """Gradients that steer compute_gamma_d: on a group's redundant rows g = a_c u + a_r res, u a masked copy of
    clip made orthogonal to res over those rows (so <res, g> = a_r |res|^2 exactly and cos_res has the sign of a_r),
    the biases a_c bias; everywhere else small noise. Built from the float64 helpers, not from the code under test."""
    grads = make_grads(start, seed, scale=0.01)
    a_c, a_r = COEFF[kind]
    gen = torch.Generator().manual_seed(77 + seed)
    for i, rows in enumerate(redundant):
        w = start[f"l{i}.weight"].double().numpy()
        d, q = float(start[f"l{i}.d_quant_wt"]), float(start[f"l{i}.q_m_wt"])
        t = float(start[f"l{i}.t_quant_wt"]) if f"l{i}.t_quant_wt" in start else None
        clip, res, _ = R.clip_res_quant_f64(w, d, q, t)
        mask = (torch.rand(w.shape, generator=gen) < 0.5).double().numpy()
        u, r = (clip * mask)[rows], res[rows]
        u = u - (np.sum(u * r) / np.sum(r * r)) * r
        grads[f"l{i}.weight"][rows] = torch.from_numpy(a_c * u + a_r * r).float()
        grads[f"l{i}.bias"][rows] = (a_c * start[f"l{i}.bias"][rows]).float()
    return grads


def steer_signs(net, redundant, kind):
    """The reference tests the SIGNED mean of clip over the redundant rows (geta.py:387), which random weights put
    below 1e-8 half of the time: positive rows for every kind but "mean", negative ones for it."""
    with torch.no_grad():
        for i, rows in enumerate(redundant):
            ly = getattr(net, f"l{i}")
            sign = -1.0 if kind == "mean" else 1.0
            ly.weight[rows] = sign * ly.weight[rows].abs()
            ly.bias[rows] = sign * ly.bias[rows].abs()


JOINT_KW = dict(BASE, start_pruning_step=1, pruning_steps=4, pruning_periods=1)


def _install(groups, redundant):
    """The redundant and pruned sets by hand; the caller has put curr_pruning_period past the last period, so no
    boundary fires and the next step (number 2) is a joint step at t = 1 of a period of 4."""
    for g, a, p in zip(groups, redundant, PRUNED):
        g.active, g.pruned = list(a), [r for r in p if r not in a]
        g.important = [i for i in range(g.num_groups) if i not in g.active and i not in g.pruned]


def _joint_ref(sets, kind, seed=3, variant="sgd_plain", nonlinear=True):
    """Parameters, gradients and both reference forms after the joint step, all on the CPU."""
    kw = dict(JOINT_KW, **VARIANTS[variant])
    net = make_net(torch.device("cpu"), seed, nonlinear)
    steer_signs(net, REDUNDANT[sets], kind)
    start = host_params(net)
    grads = joint_grads(start, REDUNDANT[sets], kind, seed)
    forms = [PruneF64({k: v.numpy() for k, v in start.items()}, PruneHyper(**kw), ref_groups()),
             PruneTorch(start, PruneHyper(**kw), ref_groups())]
    for o in forms:
        o.curr_period, o.num_steps = 1, 1
        _install(o.groups, REDUNDANT[sets])
    forms[0].step({k: v.numpy() for k, v in grads.items()})
    forms[1].step(grads)
    return start, grads, forms, kw


def _joint_device(dev, start, sets, kw, nonlinear=True):
    net = make_net(dev, 0, nonlinear)
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.copy_(start[name].to(dev))
    opt = make_opt(net, **kw)
    opt.num_steps = 1
    opt._prune.curr_period = 1
    _install(opt._prune.groups, REDUNDANT[sets])
    opt._prune._tables()
    return net, opt


KINDS = {"pos": R.SCHEDULE, "neg": R.NEGATIVE, "mean": R.MEAN_ZERO, "zero": R.NON_FINITE, "res_pos": R.SCHEDULE,
         "loop": R.SCHEDULE, "min": R.SCHEDULE}


# every redundant set with every branch kind on the nonlinear quantizer, and the linear one (t NULL on the device,
# pw = |x| where the reference forms exp(1.0 * log|x|)) on the kinds that run clip, res and quantize to the end
JOINT_CASES = [(s, k, True) for s in REDUNDANT for k in KINDS] + \
              [("scattered", k, False) for k in ("pos", "neg", "loop")]


@pytest.fixture(scope="module")
def joint_refs():
    """Every case's reference run, and the tolerance the issue asks to be measured: the largest relative difference
    between the fp32 torch form and the float64 form over ALL these inputs, per quantity (a single case can agree
    by luck to the last bit, which says nothing about fp32's reach). Rows: relative to the largest entry."""
    runs, rel = {}, {"gamma": 0.0, "d": 0.0, "rows": 0.0}
    for sets, kind, nonlinear in JOINT_CASES:
        if True:
            runs[sets, kind, nonlinear] = start, grads, (f64, th), kw = _joint_ref(sets, kind, nonlinear=nonlinear)
            for g in f64.groups:
                (ga, da, _), (gb, db, _) = f64.last[g.name], th.last[g.name]
                if ga:
                    rel["gamma"] = max(rel["gamma"], abs(ga - gb) / abs(ga))
                rel["d"] = max(rel["d"], abs(da - db) / abs(da))
                for m in g.members:
                    a, b = f64.p[m][g.active], th.p[m][g.active].double().numpy()
                    rel["rows"] = max(rel["rows"], float(np.abs(a - b).max() / np.abs(a).max()))
    print("measured (b)-(a), relative:", {k: f"{v:.3e}" for k, v in rel.items()})
    return runs, rel


@pytest.mark.parametrize("sets,kind,nonlinear", JOINT_CASES,
                         ids=[f"{s}-{k}{'' if n else '-linear'}" for s, k, n in JOINT_CASES])
def test_joint_step(dev, joint_refs, sets, kind, nonlinear):
    runs, rel = joint_refs
    start, grads, (f64, th), kw = runs[sets, kind, nonlinear]
    net, opt = _joint_device(dev, start, sets, kw, nonlinear)
    set_grads(net, grads, dev)
    opt.step()
    got = host_params(net)
    gamma, info = opt._prune.gamma.cpu().numpy().astype(np.float64), opt._prune.info.cpu().numpy()
    seen = set()
    for i, g in enumerate(f64.groups):
        ga, da, ia = f64.last[g.name]
        ib = th.last[g.name][2]
        sums, count = f64.last_six[g.name]
        if kind != "zero":
            assert R.margins(*sums, count) >= 1e-3, (g.name, R.margins(*sums, count))   # a condition on the inputs
        assert ia == ib == int(info[i]), (g.name, ia, ib, int(info[i]))
        assert ia & 7 == KINDS[kind]
        seen.add(ia)
        for what, a, dv in (("gamma", ga, gamma[i]), ("d", da, float(got[f"l{i}.d_quant_wt"]))):
            tol = max(4 * rel[what] * abs(a), float(_ulp32(a)))
            print(f"{g.name} {what}: device {dv:.9e} f64 {a:.9e} err {abs(dv - a):.2e} tol {tol:.2e}")
            assert abs(dv - a) <= tol, (g.name, what)
        for m in g.members:
            a, dv = f64.p[m][g.active], got[m][g.active].double().numpy()
            tol = np.maximum(4 * rel["rows"] * np.abs(a).max(), _ulp32(a))
            err = np.abs(dv - a)
            print(f"{m} redundant rows: max err {err.max():.2e}, tol {tol.min():.2e}")
            assert (err <= tol).all(), m
            if g.pruned:
                assert not got[m][g.pruned].any(), m
    if kind == "res_pos":
        assert all(i & R.D_UPPER for i in seen)
    if kind == "loop":
        assert all(i & R.LOOPED for i in seen)
    if kind == "min":
        assert all(i & R.MIN_UPPER for i in seen)
    if kind in ("pos", "neg"):
        assert not any(i & R.D_UPPER for i in seen)


def test_rows_outside_the_redundant_set_take_the_dense_step_without_decay(dev):
    from quantized_vit_amd import QuantAwareOptimizer
    redundant = REDUNDANT["scattered"]
    start, grads, _, kw = _joint_ref("scattered", "pos", seed=4, variant="adamw")
    net, opt = _joint_device(dev, start, "scattered", kw)
    plain = make_net(dev, 0)
    with torch.no_grad():
        for name, p in plain.named_parameters():
            p.copy_(start[name].to(dev))
    kw2 = {k: v for k, v in kw.items() if k not in ("start_pruning_step", "pruning_steps", "pruning_periods")}
    dense = QuantAwareOptimizer(plain, **dict(kw2, weight_decay=None, fix_after_step=5))
    dense.num_steps = 1
    for _ in range(2):   # the second step reads the moments the first one left
        set_grads(net, grads, dev)
        set_grads(plain, grads, dev)
        opt.step()
        dense.step()
    a, b = host_params(net), host_params(plain)
    for i, (act, pr) in enumerate(zip(redundant, PRUNED)):
        keep = [r for r in range(ROWS[i]) if r not in act and r not in pr]
        for leaf in ("weight", "bias"):
            assert torch.equal(a[f"l{i}.{leaf}"][keep], b[f"l{i}.{leaf}"][keep]), (i, leaf)
            assert not a[f"l{i}.{leaf}"][[r for r in pr if r not in act]].any()
    sa, sb = opt.state_dict(), dense.state_dict()
    for u, v in zip(sa["first_moments"] + sa["second_moments"], sb["first_moments"] + sb["second_moments"]):
        assert torch.equal(u, v)   # the moments move as the dense step moves them, on every row


FINISH = [   # cg, cc, gg, rg, rr, csum per row -> the branches no honest tensor reaches, and the loop cap
    ((3.0, 4.0, 1.0, 0.1, 1.0, 5.0), R.CLAMP_POS | R.D_UPPER),
    ((-3.0, 4.0, 1.0, 0.1, 1.0, 5.0), R.CLAMP_NEG | R.D_UPPER),
    ((-3.0, 4.0, 1.0, -0.5, 1.0, 5.0), R.CLAMP_NEG | R.MIN_UPPER),
    ((1e-150, 4.0, 1e-300, -5e-151, 1.0, 5.0), R.SCHEDULE | R.LOOPED | R.CAPPED),
    ((1e-4, 4.0, 1e-8, -5e-5, 1.0, 5.0), R.SCHEDULE | R.LOOPED),
]


def test_finish_kernel_branches_from_given_sums(dev):
    """qvit_prune_joint_finish on hand-made partials: |cos| > 1 cannot come from real tensors, nor can the cut loop
    without a denormal gradient norm. Three rows per group, folded in index order."""
    from quantized_vit_amd import _lib
    ng = len(FINISH)
    scal = torch.tensor([[1.0 / 127, 1.0, 1.0]] * ng, dtype=torch.float32, device=dev)
    table = np.zeros(ng, dtype=_lib.PRUNE_GROUP_DTYPE)
    partials = np.zeros((3 * ng, 6))
    for i, (s, _) in enumerate(FINISH):
        base = scal.data_ptr() + 12 * i
        G = table[i]
        G["d"], G["qm"], G["t"] = base, base + 4, base + 8
        G["rows"], G["joint"], G["red_begin"], G["red_count"], G["elems"] = 10, 1, 3 * i, 3, 5
        partials[3 * i:3 * i + 3] = np.asarray(s) * np.array([[0.5], [0.25], [0.25]])
    gamma = torch.zeros(ng, dtype=torch.float32, device=dev)
    info = torch.zeros(ng, dtype=torch.int32, device=dev)
    _lib.prune_joint_finish(torch.from_numpy(table.view(np.int64)).to(dev), ng, torch.from_numpy(partials).to(dev),
                            3 * ng, 1e-2, 4, 1, 4, 16, gamma, info)
    gamma, info, d = gamma.cpu().numpy(), info.cpu().numpy(), scal[:, 0].cpu().numpy()
    for i, (s, want) in enumerate(FINISH):
        ga, da, ia = R.gamma_d_scalar(*s, count=15, lr=1e-2, period=4, t=1, q_m=1.0, t_quant=1.0, min_bit=4,
                                      max_bit=16)
        assert ia == want == int(info[i]), (i, ia, want, int(info[i]))
        assert abs(gamma[i] - ga) <= _ulp32(ga) and abs(d[i] - da) <= _ulp32(da), (i, gamma[i], ga, d[i], da)


# ---- rejections ---------------------------------------------------------------------------------------------------
def test_constructor_rejections(dev):
    from quantized_vit_amd import PruneGroup, QuantAwareOptimizer
    net = make_net(dev, 0)
    net.plain = nn.Linear(4, 6).to(dev)
    net.h16 = nn.Parameter(torch.zeros(8, 3, device=dev, dtype=torch.float16))
    net.strided = nn.Parameter(torch.zeros(3, 8, device=dev).t())
    assert not net.strided.is_contiguous()
    ok = dict(BASE, variant="sgd")

    def build(groups, **kw):
        return QuantAwareOptimizer(net, prune_groups=groups, **dict(ok, **kw))
    with pytest.raises(ValueError, match="QuantizeLinear"):
        build([PruneGroup("g", net.plain, [net.plain.weight])])
    with pytest.raises(ValueError, match="float32"):
        build([PruneGroup("g", net.l0, [net.l0.weight, net.h16])])
    with pytest.raises(ValueError, match="contiguous"):
        build([PruneGroup("g", net.l0, [net.l0.weight, net.strided])])
    del net.h16, net.strided
    with pytest.raises(ValueError, match="two groups"):
        build([PruneGroup("a", net.l0, [net.l0.weight]), PruneGroup("b", net.l0, [net.l0.weight])])
    with pytest.raises(ValueError, match="shape"):
        build([PruneGroup("g", net.l0, [net.l0.weight, net.l1.bias])])
    with pytest.raises(ValueError, match="fix_after_step"):
        build(dev_groups(net), start_pruning_step=2, pruning_steps=4, fix_after_step=5)
    assert build(dev_groups(net), start_pruning_step=2, pruning_steps=4, fix_after_step=6).fix_after_step == 6


# ---- the schedule, end to end ---------------------------------------------------------------------------------------
def small_vit(dev, seed=0):
    """Two blocks, dim 64, hidden 96, 4 heads, 16 x 16 patches on 32 x 32: W4A8, calibrated as build_quantized_vit
    calibrates."""
    from quantized_vit_amd import QuantizationMode, QuantizationType, collect_input_absmax, model_to_quantize_model, \
        set_activation_quant
    from quantized_vit_amd.calibrate import redraw_init_artifacts, synthetic_images
    from quantized_vit_amd.vit_model import VisionTransformer
    torch.manual_seed(seed)
    model = VisionTransformer(img_size=32, patch_size=16, num_classes=10, embed_dim=64, depth=2, num_heads=4,
                              mlp_ratio=1.5, representation_size=None)
    redraw_init_artifacts(model)
    model = model.to(dev).eval()
    absmax = collect_input_absmax(model, synthetic_images(2, 32, seed=1, device=dev))
    model = model_to_quantize_model(model, num_bits=4, quant_type=QuantizationType.SYMMETRIC_NONLINEAR,
                                    quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    set_activation_quant(model, absmax, bits=8, t=1.0)
    return model.eval()


SCHEDULE = dict(variant="adamw", lr=1e-3, lr_quant=1e-4, first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2,
                start_projection_step=0, projection_steps=2, min_bit_wt=4, max_bit_wt=16, min_bit_act=4,
                max_bit_act=16, start_pruning_step=2, pruning_steps=6, pruning_periods=2, target_group_sparsity=0.5)
NSTEPS = 10


def _vit_groups():
    return [Group(f"blocks.{i}.mlp", f"blocks.{i}.mlp.fc1", [f"blocks.{i}.mlp.fc1.weight", f"blocks.{i}.mlp.fc1.bias"])
            for i in range(2)]


def _vit_grads(start, s):
    g = torch.Generator().manual_seed(500 + s)
    return {k: torch.randn(v.shape, generator=g) * (0.002 if v.numel() == 1 else 0.02) for k, v in start.items()}


@pytest.fixture(scope="module")
def schedule_run(dev):
    """The run every schedule test reads: the model after NSTEPS steps, the reference's sets per step, a checkpoint
    inside the second period and the device's sets per step."""
    from quantized_vit_amd import QuantAwareOptimizer, vit_mlp_prune_groups
    model = small_vit(dev)
    start = host_params(model)
    opt = QuantAwareOptimizer(model, prune_groups=vit_mlp_prune_groups(model), **SCHEDULE)
    ref = PruneF64({k: v.numpy() for k, v in start.items()}, PruneHyper(**SCHEDULE), _vit_groups())
    rows_dev, rows_ref, ckpt, synced = [], [], None, []
    for s in range(NSTEPS):
        g = _vit_grads(start, s)
        set_grads(model, g, dev)
        boundary = opt._prune._boundary(s + 1)
        nred = opt._prune._nred   # rows in the joint stage as the step begins (a boundary step selects its own)
        if not boundary:
            torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        synced.append((s + 1, boundary, nred))
        ref.step({k: v.numpy() for k, v in g.items()})
        rows_dev.append((opt.pruned_rows(), [sorted(x.active) for x in opt._prune.groups]))
        rows_ref.append((ref.pruned_rows(), [sorted(x.active) for x in ref.groups]))
        if s + 1 == 6:   # the first step of the second period: its rows are selected and not yet committed
            ckpt = (copy.deepcopy(opt.state_dict()), {k: v.clone() for k, v in model.state_dict().items()})
    return dict(model=model, opt=opt, ref=ref, start=start, rows_dev=rows_dev, rows_ref=rows_ref, ckpt=ckpt,
                synced=synced)


def test_schedule_selects_the_reference_sets_and_reaches_the_target(schedule_run):
    r = schedule_run
    assert r["rows_dev"] == r["rows_ref"]
    assert [b for _, b, _ in r["synced"]] == [n in (3, 6) for n in range(1, NSTEPS + 1)]
    assert any(nred for _, b, nred in r["synced"] if not b), "no joint step ran under the sync check"
    final = r["opt"].pruned_rows()
    assert sum(len(v) for v in final.values()) == 96
    m, mr = r["opt"].prune_metrics(), r["ref"].prune_metrics()
    assert m["num_zero_groups"] == 96 and abs(m["group_sparsity"] - 0.5) < 1e-9
    assert m["num_important_groups"] == mr["num_important_groups"] == 96
    assert m["num_redundant_groups"] == mr["num_redundant_groups"] == 96
    assert r["opt"].fixed and r["opt"].stage() == 2
    for i, blk in enumerate(r["model"].blocks):
        rows = final[f"blocks.{i}.mlp"]
        assert not blk.mlp.fc1.weight[rows].any() and not blk.mlp.fc1.bias[rows].any()
        keep = [x for x in range(96) if x not in rows]
        assert blk.mlp.fc1.weight[keep].abs().sum(dim=1).min() > 0


def test_a_mid_period_checkpoint_continues_identically(dev, schedule_run):
    from quantized_vit_amd import QuantAwareOptimizer, vit_mlp_prune_groups
    state, params = schedule_run["ckpt"]
    for key in ("pruned_idxes", "active_redundant_idxes", "curr_pruning_period", "target_num_redundant_groups"):
        assert key in state["pruning"]
    assert any(state["pruning"]["active_redundant_idxes"])   # really inside a period
    model = small_vit(dev)
    model.load_state_dict(params)
    opt = QuantAwareOptimizer(model, prune_groups=vit_mlp_prune_groups(model), **SCHEDULE)
    opt.load_state_dict(state)
    for s in range(6, NSTEPS):
        set_grads(model, _vit_grads(schedule_run["start"], s), dev)
        opt.step()
    a, b = host_params(model), host_params(schedule_run["model"])
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert opt.pruned_rows() == schedule_run["opt"].pruned_rows()


PLAIN = {k: v for k, v in SCHEDULE.items() if not k.startswith(("pruning", "start_pruning", "target"))}
IDENTITY = {
    # the untouched default path (fix_after_step left alone: 2) against declared groups that never prune
    # (pruning_steps = 0: no period, the fix stage after start_pruning_step = 2)
    "default_fix_after_step": (dict(PLAIN), dict(PLAIN, start_pruning_step=2, pruning_steps=0)),
    # the pruning schedule's stages (fix after 2 + 6) with a target of 0: boundaries and selections run and take no
    # row. projection_steps = 100 keeps the bit schedule still in both, since it ends at fix_after_step without
    # groups and at start_pruning_step with them
    "target_zero": (dict(PLAIN, projection_steps=100, fix_after_step=8),
                    dict(SCHEDULE, projection_steps=100, target_group_sparsity=0.0)),
}


@pytest.mark.parametrize("case", list(IDENTITY))
def test_members_through_the_apply_kernel_leave_the_bits_of_the_run_without_groups(dev, schedule_run, case):
    """prune_groups=None is the code path of before, run here untouched. With groups declared the members leave the
    dense launch for qvit_prune_joint_apply in every stage; when nothing is pruned that must give the same bits
    everywhere: parameters, moments, quantizer moments and the fixed bit widths."""
    from quantized_vit_amd import QuantAwareOptimizer, vit_mlp_prune_groups
    kw_plain, kw_groups = IDENTITY[case]
    runs = []
    for kw in (kw_plain, kw_groups):
        model = small_vit(dev)
        groups = vit_mlp_prune_groups(model) if kw is kw_groups else None
        opt = QuantAwareOptimizer(model, prune_groups=groups, **kw)
        for s in range(NSTEPS):
            set_grads(model, _vit_grads(schedule_run["start"], s), dev)
            opt.step()
        runs.append((host_params(model), opt.state_dict(), opt))
    (pa, sa, oa), (pb, sb, ob) = runs
    assert oa.fix_after_step == ob.fix_after_step == (2 if case == "default_fix_after_step" else 8)
    assert oa.fixed and ob.fixed and (oa.max_bit_wt, oa.max_bit_act) == (ob.max_bit_wt, ob.max_bit_act)
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    for key in ("first_moments", "second_moments"):
        assert all(torch.equal(u, v) for u, v in zip(sa[key], sb[key]))
    assert torch.equal(sa["quant_moments"], sb["quant_moments"]) and torch.equal(sa["fixed_bits"], sb["fixed_bits"])
    assert "pruning" not in sa and sb["pruning"]["pruned_idxes"] == [[], []]


# ---- compression ----------------------------------------------------------------------------------------------------
def test_compressed_model_gives_the_same_logits(dev, schedule_run):
    from quantized_vit_amd import _lib, compress_pruned_mlp
    from quantized_vit_amd.calibrate import synthetic_images
    img = synthetic_images(2, 32, seed=9, device=dev)
    # the schedule run's own sets on a freshly calibrated W4A8 model: the trained scalars of that run have left the
    # int8 range (16-bit start), and the statement is about the integer path
    pruned, by_hand = small_vit(dev), small_vit(dev, seed=2)
    keep = 37
    assert keep % _lib.TILE_K != 0 and keep % 16 != 0 and keep % 4 != 0
    chosen = list(schedule_run["opt"].pruned_rows().values())
    with torch.no_grad():
        for model, sets in ((pruned, chosen), (by_hand, [torch.randperm(96, generator=torch.Generator().manual_seed(i))
                                                         [:96 - keep].tolist() for i in range(2)])):
            for blk, rows in zip(model.blocks, sets):
                blk.mlp.fc1.weight[rows] = 0
                blk.mlp.fc1.bias[rows] = 0
                blk.mlp.fc1.invalidate()
    left = [96 - len(rows) for rows in schedule_run["opt"].pruned_rows().values()]
    assert sum(left) == 96 and all(h % _lib.TILE_K for h in left)   # the K padding of fc2 is exercised
    for model, hidden in ((pruned, left), (by_hand, [keep, keep])):
        with torch.no_grad():
            for m in model.modules():
                if callable(getattr(m, "invalidate", None)):
                    m.invalidate()
            want = model(img).clone()
            small = compress_pruned_mlp(model)
            assert [b.mlp.fc1.out_features for b in small.blocks] == hidden == \
                [b.mlp.fc2.in_features for b in small.blocks]
            assert all(b.mlp.fc1.quant_plan().int_path and b.mlp.fc2.quant_plan().int_path for b in small.blocks)
            got = small(img)
        assert torch.isfinite(want).all() and torch.equal(got, want)
