"""The group-lasso penalty of QuantAwareOptimizer (group_lasso_lambda; qvit_group_lasso, qvit_group_lasso_scale)
against tests/group_lasso_ref.py.

Shapes: the groups of test_gpu_prune_step.py (8, 33 and 70 rows, widths 48 and 130, the scalar path, plus bias;
l2.weight 4 bytes off alignment); `fit`, whose row with its bias fills the register budget exactly, `over4` and
`over3`, 4 and 3 elements past it (the 16-byte and the scalar streaming path); `head`, 3 units of sections = 3,
unit_rows = 5; `small`, 2 rows, not prunable under group_divisible = 2. One unit of l0, over4 and head is zero and
l1.bias has no gradient.

Bounds. sumsq: a double accumulation, N 2^-53 sum p^2. loss: 1 fp32 ulp plus the sumsq bound through the square
root. Gradient: 2^-22 |term| + ulp32(g + term) for one rounding each of coef, the product and the add. gl_scale: 1
fp32 ulp of the float64 form. Everything else is bit for bit."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import group_lasso_ref as R
from quantized_vit_amd import PruneGroup, QuantAwareOptimizer, QuantizeLinear, _lib

BUDGET = _lib.GROUP_LASSO_SLOTS * _lib.GROUP_LASSO_SLOT_ELEMS
# name: rows, width, sections, unit_rows
SHAPES = {"l0": (8, 48, 1, 1), "l1": (33, 130, 1, 1), "l2": (70, 48, 1, 1), "fit": (3, BUDGET - 256, 1, 1),
          "over4": (5, BUDGET - 252, 1, 1), "over3": (6, BUDGET - 253, 1, 1), "head": (45, 20, 3, 5),
          "small": (2, 8, 1, 1)}
PRUNABLE = [n for n in SHAPES if n != "small"]
ZEROED = {"l0": [3], "over4": [2], "head": [(s * 3 + 1) * 5 + j for s in range(3) for j in range(5)]}   # head: unit 1
ADAMW = dict(variant="adamw", first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2)
SCHED = dict(lr=1e-2, lr_quant=1e-3, start_projection_step=0, projection_steps=2, start_pruning_step=1, pruning_steps=4,
             pruning_periods=2, group_divisible=2, grad_clip=(-0.02, 0.02),   # a boundary at step 2
             # scores of a size at which sqrt(elems) / score lies inside (0.1, 10) for some units and outside for others
             # (the default weights sum to 1 and clamp every unit at 10: every scale 1)
             importance_score_criteria={"magnitude": 40.0, "taylor_first_order": 10.0})


def make_net(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    net = nn.Module()
    for name, (rows, width, _, _) in SHAPES.items():
        setattr(net, name, QuantizeLinear(width, rows, bias=True))
    net = net.to(dev)
    net.l2.weight = nn.Parameter(torch.zeros(70 * 48 + 1, device=dev)[1:].view(70, 48))
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(("weight", "bias")):
                v = torch.randn(p.shape, generator=g) * 0.3
            else:   # d_quant, q_m
                v = (0.9 + 0.2 * torch.rand(1, generator=g)) / (127.0 if "d_quant" in name else 1.0)
            p.copy_(v.to(dev))
        for name, rows in ZEROED.items():
            getattr(net, name).weight[rows] = 0.0
            getattr(net, name).bias[rows] = 0.0
    return net


def groups_of(net, names=SHAPES):
    return [PruneGroup(n, getattr(net, n), [getattr(net, n).weight, getattr(net, n).bias], SHAPES[n][2], SHAPES[n][3])
            for n in names]


def ref_groups(net):
    return [(g.members, g.sections, g.unit_rows) for g in groups_of(net, PRUNABLE)]


def set_grads(net, seed, dev, skip=()):
    g = torch.Generator().manual_seed(1000 + seed)
    for name, p in net.named_parameters():
        v = torch.randn(p.shape, generator=g) * 0.05
        p.grad = None if name in skip else v.to(dev)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def check_grads(net, before, terms):
    """Every member's gradient against before + term within the bound; bit for bit where the term is 0."""
    for n, ts in zip(PRUNABLE, terms):
        for p, t, leaf in zip((getattr(net, n).weight, getattr(net, n).bias), ts, ("weight", "bias")):
            g0 = before[f"{n}.{leaf}"]
            if g0 is None:
                assert p.grad is None
                continue
            got, g0 = p.grad.cpu().numpy(), g0.numpy()
            want = g0.astype(np.float64) + t
            err, tol = np.abs(got - want), 2.0 ** -22 * np.abs(t) + ulp32(want)
            assert (err <= tol).all(), (n, leaf)
            assert np.array_equal(got[t == 0].view(np.int32), g0[t == 0].view(np.int32)), (n, leaf)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["unit_scale", "scaled", "lambda0"])
def test_penalty_against_float64(dev, case):
    net = make_net(dev)
    opt = QuantAwareOptimizer(net, prune_groups=groups_of(net), group_lasso_lambda=0.0, **ADAMW, **SCHED)
    nu, scale, lam = opt._prune.total_num_groups, None, 0.0 if case == "lambda0" else 0.05
    if case == "scaled":   # as a checkpoint taken after a boundary brings it
        st = opt.state_dict()
        st["pruning"]["gl_scale"] = torch.rand(nu, generator=torch.Generator().manual_seed(5)) * 9.9 + 0.1
        opt.load_state_dict(st)
        scale = st["pruning"]["gl_scale"].double().numpy()
    set_grads(net, 0, dev, skip=("l1.bias",))
    before = {n: None if p.grad is None else p.grad.cpu().clone() for n, p in net.named_parameters()}
    ptrs = np.array([opt._grad_ptr(n, p) for n, p in opt._dense], dtype=np.int64)
    opt._prune.penalty(lam, ptrs, np.zeros(len(ptrs), dtype=bool))

    sumsq, loss, terms = R.penalty_f64(ref_groups(net), scale, lam)
    elems = np.concatenate([np.full(SHAPES[n][0] // (SHAPES[n][2] * SHAPES[n][3]),
                                    (SHAPES[n][1] + 1) * SHAPES[n][2] * SHAPES[n][3]) for n in PRUNABLE])
    assert nu == len(sumsq) == 128
    got, tol = opt._prune._lasso_sumsq[:nu].cpu().numpy(), elems * 2.0 ** -53 * sumsq
    assert (np.abs(got - sumsq) <= tol).all() and (got[sumsq == 0] == 0).all() and (sumsq == 0).sum() == 3
    sc = np.ones(nu) if scale is None else scale
    loss_tol = ulp32(loss) + (sc * tol / (2 * np.sqrt(np.maximum(sumsq, 1e-300)))).sum()
    got_loss = float(opt.group_lasso_loss().cpu())
    assert abs(got_loss - loss) <= loss_tol
    check_grads(net, before, terms)
    for leaf in ("weight", "bias"):   # a group that is not prunable takes no part
        assert torch.equal(getattr(net.small, leaf).grad.cpu(), before[f"small.{leaf}"])


@pytest.mark.gpu
@pytest.mark.parametrize("nunits", [14, 602])
def test_scale_entry_point(dev, nunits):
    """inv = sqrt(elems) / |score|: 7 / 2 and 12 / 2 ordinary; 0, 1e-12 and 0.5 clamp at 10, 1e12, 100 and inf at 0.1;
    a negative score counts by its size and a NaN gives 1. The mean moves clamped units off their bounds."""
    scores = np.resize(np.array([2.0, 0.0, 1e-12, 1e12, -2.0, np.nan, np.inf, 0.5, 100.0], dtype=np.float32), nunits)
    table = np.zeros(2, dtype=_lib.PRUNE_GROUP_DTYPE)
    table["elems"] = (49, 144)
    units = np.zeros(nunits, dtype=_lib.PRUNE_ITEM_DTYPE)
    units["group"] = np.arange(nunits) >= nunits // 2
    to_dev = lambda a: torch.from_numpy(a.view(np.int64).copy()).to(dev)   # noqa: E731
    out = torch.zeros(nunits, dtype=torch.float32, device=dev)
    _lib.group_lasso_scale(to_dev(table), 2, to_dev(units), nunits, torch.from_numpy(scores).to(dev), out)
    want = R.gl_scale_f64(scores, table["elems"][units["group"]])
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and (np.abs(got - want) <= ulp32(want)).all(), np.max(np.abs(got - want) / ulp32(want))


def state_bits(opt):
    pr = opt._prune
    t = [p.detach() for p in opt.model.parameters()] + [m for m in opt._m + opt._v if m is not None] + \
        [opt._qmom, pr._scores]
    return [x.cpu().numpy().view(np.int32) for x in t], [sorted(g.active) for g in pr.groups], opt.pruned_rows()


def assert_same(a, b, scores=True):
    (ta, *la), (tb, *lb) = state_bits(a), state_bits(b)
    assert la == lb and all(np.array_equal(x, y) for x, y in zip(ta[:None if scores else -1], tb))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [ADAMW, dict(variant="sgd", first_momentum=0.9, dampening=0.1, weight_decay=1e-2)],
                         ids=["adamw", "sgd"])
def test_step_composes_with_the_parent_path(dev, variant):
    """A penalises and steps; B, built without the penalty, steps on A's penalised gradients: the same bits, so the
    penalty comes before the clip, the scores and the update. coef shows which scale a step applied: 1 up to and on
    the boundary step 2, the scale of step 2's scores in step 3."""
    lam, nets = 0.05, [make_net(dev), make_net(dev)]
    A = QuantAwareOptimizer(nets[0], prune_groups=groups_of(nets[0]), group_lasso_lambda=lam, **variant, **SCHED)
    B = QuantAwareOptimizer(nets[1], prune_groups=groups_of(nets[1]), **variant, **SCHED)
    nu = A._prune.total_num_groups
    elems = np.concatenate([np.full(g.num_groups, A._prune._grow["elems"][i]) for i, g in enumerate(A._prune.groups)
                            if g.prunable])
    scale = np.ones(nu)
    for step in range(3):
        set_grads(nets[0], step, dev)
        raw = nets[0].l0.weight.grad.clone()
        norm = np.sqrt(R.penalty_f64(ref_groups(nets[0]), None, lam)[0])
        A.step()
        assert not torch.equal(nets[0].l0.weight.grad, raw)   # the penalty reached the gradient
        for p, q in zip(nets[1].parameters(), nets[0].parameters()):
            p.grad = q.grad.clone()
        B.step()
        assert_same(A, B)
        coef = A._prune._lasso_coef[:nu].cpu().numpy()
        want = np.where(norm > 0, lam * scale / np.maximum(norm, 1e-300), 0)
        assert (np.abs(coef - want) <= 2.0 ** -23 * want).all(), step
        if step == 1:   # the boundary step: its scores make the scale of step 3
            scale = R.gl_scale_f64(A._prune._scores[:nu].cpu().numpy(), elems)
            assert (np.abs(A._prune.gl_scale[:nu].cpu().numpy() - scale) <= ulp32(scale)).all()
            scale = A._prune.gl_scale[:nu].cpu().numpy().astype(np.float64)
    assert A._prune.curr_period == 1 and scale.std() > 0 and any(A.pruned_rows().values())


@pytest.mark.gpu
@pytest.mark.parametrize("lasso", [True, False], ids=["lasso", "none"])
def test_state_round_trip(dev, lasso):
    """A checkpoint after the boundary step continues bit for bit, the scale restored; without the option the
    pruning state has the keys it had, and a penalised optimizer loads such a state as one without a scale."""
    kw = dict(group_lasso_lambda=0.05) if lasso else {}
    net = make_net(dev)
    opt = QuantAwareOptimizer(net, prune_groups=groups_of(net), **kw, **ADAMW, **SCHED)
    for step in range(2):
        set_grads(net, step, dev)
        opt.step()
    st = copy.deepcopy(opt.state_dict())
    keys = {"group_names", "pruned_idxes", "active_redundant_idxes", "important_idxes", "pruned_group_idxes",
            "curr_pruning_period", "target_num_redundant_groups"}
    assert set(st["pruning"]) == keys | ({"gl_scale"} if lasso else set())
    net2 = make_net(dev)
    net2.load_state_dict(net.state_dict())
    opt2 = QuantAwareOptimizer(net2, prune_groups=groups_of(net2), group_lasso_lambda=0.05, **ADAMW, **SCHED)
    opt2.load_state_dict(st)
    assert opt2._prune.has_gl_scale == lasso
    if lasso:
        assert torch.equal(opt2._prune.gl_scale, opt._prune.gl_scale) and float(opt2._prune.gl_scale.std()) > 0
        for o, n in ((opt, net), (opt2, net2)):
            set_grads(n, 2, dev)
            o.step()
        assert_same(opt, opt2, scores=False)   # (the scores are no part of a state)
        assert torch.equal(opt.group_lasso_loss(), opt2.group_lasso_loss()) and float(opt.group_lasso_loss()) > 0


def test_torch_form_is_the_float64_form():
    """The benchmark's fp32 torch baseline against the float64 form, within 4 fp32 roundings of each term (the norm,
    lambda scale, the division, the product); a rounding is 2^-23, as in the gradient bound, where two make 2^-22."""
    net = make_net(torch.device("cpu"), seed=3)
    groups = [g for g, n in zip(ref_groups(net), PRUNABLE) if n in ("l0", "l1", "l2", "head")]
    scale = torch.rand(sum(SHAPES[n][0] // (SHAPES[n][2] * SHAPES[n][3]) for n in ("l0", "l1", "l2", "head")),
                       generator=torch.Generator().manual_seed(9)) * 9.9 + 0.1
    for ms, _, _ in groups:
        for p in ms:
            p.grad = torch.zeros_like(p)
    loss32 = float(R.penalty_torch(groups, scale, 0.05))
    _, loss, terms = R.penalty_f64(groups, scale.double().numpy(), 0.05)
    assert abs(loss32 - loss) <= 4 * 2.0 ** -23 * loss
    for (ms, _, _), ts in zip(groups, terms):
        for p, t in zip(ms, ts):
            assert (np.abs(p.grad.numpy() - t) <= 4 * 2.0 ** -23 * np.abs(t)).all()


@pytest.mark.parametrize("lam", [-1e-6, math.nan, math.inf])
def test_rejections(lam):
    from quantized_vit_amd import build
    build.build()
    net = make_net(torch.device("cpu"))
    with pytest.raises(ValueError, match="needs prune_groups"):
        QuantAwareOptimizer(net, group_lasso_lambda=1e-6)
    with pytest.raises(ValueError, match="finite number >= 0"):
        QuantAwareOptimizer(net, prune_groups=groups_of(net), group_lasso_lambda=lam)
    lib, fake, odd = _lib.load(), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    args = lambda **kw: [kw.get(k, d) for k, d in (("groups", fake), ("ng", 1), ("members", fake), ("nm", 1),   # noqa
                                                   ("units", fake), ("nu", 1), ("rows", None), ("nr", 0),
                                                   ("scale", None), ("lam", 0.0), ("sumsq", fake), ("coef", fake),
                                                   ("loss", fake), ("stream", None))]
    assert lib.qvit_group_lasso(*args(lam=lam)) == -1
    for null in ("groups", "members", "units", "sumsq", "coef", "loss"):
        assert lib.qvit_group_lasso(*args(**{null: None})) == -3
    assert lib.qvit_group_lasso(*args(nr=1)) == -3   # rows are listed, the table is not there
    for off in ("groups", "members", "units", "sumsq"):
        assert lib.qvit_group_lasso(*args(**{off: odd})) == -2
    assert lib.qvit_group_lasso(*args(scale=ctypes.c_void_p(0x1002))) == -2
    assert lib.qvit_group_lasso(*args(nu=-1)) == -1 and lib.qvit_group_lasso(*args(nu=0)) == 0
    for bad, code in ((dict(scores=None), -3), (dict(groups=odd), -2), (dict(nu=-1), -1)):
        a = {**dict(groups=fake, ng=1, units=fake, nu=1, scores=fake, scale=fake, stream=None), **bad}
        assert lib.qvit_group_lasso_scale(*a.values()) == code
