"""tests/prune_step_ref.py against itself: the float64 and the fp32 torch forms agree over a whole schedule, every
branch of compute_gamma_d is reached by a constructed input (and the branch asserted), and the integer bookkeeping
(selection with its setdiff1d ordering, the group_divisible refinement, the period schedule) does what
optimizer/geta.py:132-147, :167-236 do. No GPU."""
import math

import numpy as np
import pytest
import torch

import prune_step_ref as R
from prune_step_ref import Group, PruneF64, PruneHyper, PruneTorch


def net(seed=0, rows=(8, 33), widths=(48, 130), nonlinear=True):
    g = torch.Generator().manual_seed(seed)
    p = {}
    for i, (r, w) in enumerate(zip(rows, widths)):
        p[f"l{i}.weight"] = torch.randn(r, w, generator=g) * 0.3
        p[f"l{i}.bias"] = torch.randn(r, generator=g) * 0.1
        for side in ("wt", "act"):
            p[f"l{i}.d_quant_{side}"] = torch.tensor([1.0 / 127 * 1.07])
            p[f"l{i}.q_m_{side}"] = torch.tensor([1.0 + 0.01 * i])
            if nonlinear:
                p[f"l{i}.t_quant_{side}"] = torch.tensor([0.98])
    p["other"] = torch.randn(5, 7, generator=g)
    return p


def groups(n=2):
    return [Group(f"g{i}", f"l{i}", [f"l{i}.weight", f"l{i}.bias"]) for i in range(n)]


def grads(params, seed, scale=0.05):
    g = torch.Generator().manual_seed(100 + seed)
    return {k: torch.randn(v.shape, generator=g) * scale for k, v in params.items()}


HP = dict(variant="adamw", lr=1e-2, lr_quant=1e-3, first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2,
          start_projection_step=0, projection_steps=2, min_bit_wt=4, max_bit_wt=16, start_pruning_step=1,
          pruning_steps=6, pruning_periods=2, target_group_sparsity=0.5)


@pytest.mark.parametrize("nonlinear", [True, False])
def test_the_two_forms_agree_over_a_schedule(nonlinear):
    start = net(0, nonlinear=nonlinear)
    a = PruneF64({k: v.numpy() for k, v in start.items()}, PruneHyper(**HP), groups())
    b = PruneTorch(start, PruneHyper(**HP), groups())
    for s in range(9):
        g = grads(start, s)
        a.step({k: v.numpy() for k, v in g.items()})
        b.step(g)
        assert a.pruned_rows() == b.pruned_rows() and a.state() == b.state()
        for k in a.p:
            np.testing.assert_allclose(b.p[k].double().numpy(), a.p[k], rtol=2e-4, atol=2e-5, err_msg=f"{k} step {s}")
    assert a.target == 20 and sum(len(v) for v in a.pruned_rows().values()) == 20
    m = a.prune_metrics()
    assert m["num_zero_groups"] == 20 and abs(m["group_sparsity"] - 20 / 41) < 1e-9
    assert b.prune_metrics()["num_zero_groups"] == 20


BRANCHES = [
    # cg, cc, gg, rg, rr, csum -> branch | flags (count 10, lr 1e-2, period 4, t 1, q_m 1, t_quant 1, bits 4..16)
    (dict(cg=1.0, cc=4.0, gg=1.0, rg=0.1, rr=1.0, csum=-1.0), R.MEAN_ZERO | R.D_UPPER),
    (dict(cg=0.0, cc=4.0, gg=0.0, rg=0.0, rr=1.0, csum=5.0), R.NON_FINITE | R.D_UPPER),
    (dict(cg=1.0, cc=4.0, gg=1.0, rg=0.1, rr=1.0, csum=5.0), R.SCHEDULE | R.D_UPPER),
    (dict(cg=1.0, cc=4.0, gg=1.0, rg=-0.5, rr=1.0, csum=5.0), R.SCHEDULE),
    (dict(cg=1.0, cc=4.0, gg=1.0, rg=-1e-3, rr=1.0, csum=5.0), R.SCHEDULE | R.MIN_UPPER),
    (dict(cg=1e-4, cc=4.0, gg=1e-8, rg=-5e-5, rr=1.0, csum=5.0), R.SCHEDULE | R.LOOPED),
    (dict(cg=-1.0, cc=4.0, gg=1.0, rg=-0.5, rr=1.0, csum=5.0), R.NEGATIVE | R.MIN_UPPER),
    (dict(cg=3.0, cc=4.0, gg=1.0, rg=0.1, rr=1.0, csum=5.0), R.CLAMP_POS | R.D_UPPER),
    (dict(cg=-3.0, cc=4.0, gg=1.0, rg=0.1, rr=1.0, csum=5.0), R.CLAMP_NEG | R.D_UPPER),
    (dict(cg=1e-150, cc=4.0, gg=1e-300, rg=-5e-151, rr=1.0, csum=5.0), R.SCHEDULE | R.LOOPED | R.CAPPED),
]


@pytest.mark.parametrize("sums,want", BRANCHES, ids=[str(i) for i in range(len(BRANCHES))])
def test_every_branch_of_compute_gamma_d(sums, want):
    gamma, d, info = R.gamma_d_scalar(**sums, count=10, lr=1e-2, period=4, t=1, q_m=1.0, t_quant=1.0, min_bit=4,
                                      max_bit=16)
    assert info == want, (info, want)
    upper, lower = 1.0 / 7, 1.0 / 32767
    assert lower <= d <= upper
    branch = want & 7
    if branch in (R.MEAN_ZERO, R.NON_FINITE) or want & R.CAPPED:
        assert gamma == 0.0 and d == upper
    elif branch in (R.SCHEDULE, R.CLAMP_POS) and not want & R.LOOPED:
        assert gamma == 1.0 - 2.0 / 3.0
    elif branch == R.NEGATIVE:
        assert gamma == pytest.approx(0.001 * 1e-2 * 1.0 / (0.5 * 2.0))
    elif branch == R.CLAMP_NEG:
        assert gamma == pytest.approx(0.001 * 1e-2 * 1.0 / 2.0)
    if want & R.LOOPED and not want & R.CAPPED:
        assert gamma < 1.0 / 3.0 and d >= lower


def test_the_torch_form_reaches_the_data_branches():
    """compute_gamma_d on tensors: positive and negative cosine, a negative mean, a zero gradient."""
    start = net(1)
    for kind, want in (("pos", R.SCHEDULE), ("neg", R.NEGATIVE), ("mean", R.MEAN_ZERO), ("zero", R.NON_FINITE)):
        p = {k: v.clone() for k, v in start.items()}
        if kind == "mean":
            p["l0.weight"] = -p["l0.weight"].abs()
            p["l0.bias"] = -p["l0.bias"].abs()
        hp = PruneHyper(variant="sgd", lr=1e-2, start_pruning_step=1, pruning_steps=4, min_bit_wt=4, max_bit_wt=16)
        b = PruneTorch(p, hp, groups())
        a = PruneF64({k: v.numpy() for k, v in p.items()}, hp, groups())
        for o in (a, b):
            o.groups[0].active, o.curr_period, o.num_steps = [1, 4, 6], 1, 1
        sign = {"pos": 1.0, "neg": -1.0, "mean": 1.0, "zero": 0.0}[kind]
        gv = {k: sign * v for k, v in p.items()}
        _, _, info = b.compute_gamma_d(b.groups[0], gv, 1)
        assert info & 7 == want, (kind, info)
        sums, count = a.six_sums(a.groups[0], {k: v.numpy().astype(np.float64) for k, v in gv.items()})
        assert R.gamma_d_scalar(*sums, count, hp.lr, 4, 1, 1.0, 0.98, 4, 16)[2] & 7 == want


def test_selection_cuts_a_surplus_by_index_not_by_score():
    scores = np.array([0.9, 0.1, 0.8, 0.2, 0.3, 0.05, 0.7, 0.6])   # no ties
    first = R.select(scores, [], 2)
    assert first == [1, 5]
    # second period: K = 2 + 2 lowest are {5, 1, 3, 4}; minus the taken: [3, 4]
    assert R.select(scores, first, 2) == [3, 4]
    # a taken row that has left the K lowest leaves a surplus: the K = 3 lowest of the new scores are {7, 6, 4},
    # none of them taken, and setdiff1d hands them back sorted by index, so [:2] keeps 4 and 6 and drops 7, the
    # lowest score of all
    scores2 = np.array([0.9, 0.8, 0.7, 0.6, 0.3, 0.95, 0.2, 0.1])
    assert R.select(scores2, [5], 2) == [4, 6]


def test_group_divisible_refinement():
    g = Group("g", "l", [], num_groups=10, important=list(range(10)), active=[0, 2, 4])
    assert R.refine(g, 4) == -1 and g.active == [0, 2] and g.important == [1, 3, 4, 5, 6, 7, 8, 9]   # 7 -> 8 kept
    g = Group("g", "l", [], num_groups=10, important=list(range(10)), active=list(range(10)))
    assert R.refine(g, 4) == -4 and g.active == list(range(6)) and g.important == [6, 7, 8, 9]       # never empty
    g = Group("g", "l", [], num_groups=10, important=list(range(10)), active=[1, 3])
    assert R.refine(g, 4) == 0 and g.active == [1, 3]                                                # 8 is divisible
    g = Group("g", "l", [], num_groups=3, important=[0, 1, 2], active=[1], pruned=[])
    assert R.refine(g, 4) == 0 and g.active == [] and g.important == [0, 1, 2]                       # too small


def test_period_schedule():
    assert R.active_num_redundant_groups(10, 3) == [3, 3, 4]
    assert R.active_num_redundant_groups(96, 2) == [48, 48]
    assert R.active_num_redundant_groups(5, 1) == [5]
    assert sum(R.active_num_redundant_groups(101, 7)) == 101


def test_boundaries_and_commits_fall_where_the_reference_puts_them():
    hp = PruneHyper(**dict(HP, start_pruning_step=3, pruning_steps=6, pruning_periods=2))
    a = PruneF64({k: v.numpy() for k, v in net(2).items()}, hp, groups())
    seen = []
    for s in range(11):
        a.step({k: v.numpy() for k, v in grads(net(2), s).items()})
        seen.append((a.num_steps, a.curr_period, sum(len(g.active) for g in a.groups),
                     sum(len(g.pruned) for g in a.groups)))
    # boundary at (n - 3 - 1) % 3 == 0: n = 4, 7; commit at (n - 3) % 3 == 2: n = 5, 8
    assert [x[1] for x in seen] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2]
    assert [x[2] for x in seen] == [0, 0, 0, 10, 0, 0, 10, 0, 0, 0, 0]
    assert [x[3] for x in seen] == [0, 0, 0, 0, 10, 10, 10, 20, 20, 20, 20]
