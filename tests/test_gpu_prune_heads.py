"""Prune groups whose unit is a set of rows (attention heads) on the device, against tests/prune_step_ref.py through
tests/prune_heads_ref.py's permutation: the folded saliency sums and scores, the joint step with every branch of
compute_gamma_d, the exact zeros of a pruned head, the dense step of an important one, run-to-run bits, and the whole
schedule on a two-block ViT with head and MLP groups.

Shapes (tests/prune_heads_common.py): a head group of H = 3, hd = 4, width 50 (the scalar path), one of H = 2, hd = 64,
width 128 (the 16-byte path), a BASIC group of 33 rows and a head group of H = 2, hd = 4, width 48, the weights of
both starting 4 bytes into their storage.

Tolerances. A unit's sums are double accumulations of fp32 inputs, per row and then over the rows: N 2^-53 sum|terms|
against float64, N the UNIT's element count. gamma, d and the redundant rows: 4 x the largest difference between the
reference's fp32 torch form and its float64 form over all these inputs, never below 1 fp32 ulp of the value, measured
here and not taken from the one-row tests: the units are longer.

Rounding ties. The joint branch subtracts gamma * d * rint(q), q = |w|^t / d. A weight whose q lies within fp32's
reach of k + 1/2 takes the neighbouring code in fp32, a step of gamma * d, a thousand times every other difference.
Such elements are identified from the float64 form alone (near_tie: 1/2 - |rint(q) - q| <= |q| 2^-20, sixteen fp32
ulps of q for the exp, log and division that form it), are left out of the measured figure, and may differ from
float64 by one code step more than the others; every other element is held to the figure measured without them."""
import copy

import numpy as np
import pytest
import torch

import prune_heads_common as C
import prune_heads_ref as P
import prune_step_ref as R
from prune_step_ref import PruneF64, PruneHyper, PruneTorch
from test_gpu_prune_step import (BASE, JOINT_KW, KINDS, NSTEPS, SCHEDULE, U24, VARIANTS, _ulp32, device_grad_variant,
                                 host_params, joint_grads, make_grads, set_grads, steer_signs)

pytestmark = pytest.mark.gpu


def make_opt(net, **kw):
    from quantized_vit_amd import QuantAwareOptimizer
    return QuantAwareOptimizer(net, prune_groups=C.dev_groups(net), **kw)


def np_dict(d):
    return {k: v.numpy() for k, v in d.items()}


def ref_forms(start, kw):
    """Both reference forms on the permuted copy of `start` (torch tensors on the CPU)."""
    hp = PruneHyper(**kw)
    return (PruneF64(P.permute(np_dict(start), C.SPECS), hp, C.ref_groups()),
            PruneTorch(P.permute(start, C.SPECS), PruneHyper(**kw), C.ref_groups()))


# ---- scores -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("later", [False, True], ids=["first_step", "later_step"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_unit_scores_against_float64(dev, variant, later):
    sched = dict(start_pruning_step=1, pruning_steps=3 if later else 1, pruning_periods=1)
    kw = dict(BASE, **VARIANTS[variant], **sched)
    net = C.make_net(dev, 1)
    start = host_params(net)
    opt = make_opt(net, **kw)
    assert opt._prune.folded and opt._prune.total_num_groups == sum(C.UNITS)
    f64, _ = ref_forms(start, kw)
    for s in range(2 if later else 1):
        if s == (1 if later else 0):
            before = host_params(net)
        g = make_grads(start, s)
        set_grads(net, g, dev)
        opt.step()
        f64.step(P.permute(np_dict(g), C.SPECS))
    assert f64.curr_period == 1 and opt._prune.curr_period == 1
    sums = opt._prune._unit_sums.cpu().numpy()
    scores = opt._prune._scores.cpu().numpy().astype(np.float64)
    before_u = P.permute(before, C.SPECS)
    gv_u = P.permute(device_grad_variant(opt, variant, g), C.SPECS)
    row0, per_group, tols = 0, [], []
    for gr in f64.groups:
        p = torch.cat([before_u[m].reshape(gr.num_groups, -1) for m in gr.members], dim=1).double().numpy()
        gv = np.concatenate([gv_u[m].reshape(gr.num_groups, -1) for m in gr.members], axis=1).astype(np.float64)
        n = p.shape[1]
        assert n == int(opt._prune._grow["elems"][int(gr.name[1])])   # elems is the unit's element count
        want = np.stack([(p * p).sum(1), (gv * gv).sum(1), (p * gv).sum(1)], axis=1)
        absum = np.stack([(p * p).sum(1), (gv * gv).sum(1), np.abs(p * gv).sum(1)], axis=1)
        tol = n * 2.0 ** -53 * absum
        got = sums[row0:row0 + gr.num_groups]
        err = np.abs(got - want)
        print(f"{gr.name}: {gr.num_groups} units of {n} elements, sums max err/tol "
              f"{np.max(err / np.maximum(tol, 1e-300)):.3f}")
        assert (err <= tol).all(), (gr.name, float(np.max(err / tol)))
        per_group.append(R.criteria_f64(want[:, 0], want[:, 1], want[:, 2], n))
        tols.append(2 * n * 2.0 ** -53 * np.maximum(1.0, absum[:, 2] / np.maximum(np.abs(want[:, 2]), 1e-300)))
        row0 += gr.num_groups
    assert row0 == sum(C.UNITS)
    want_scores = np.concatenate(R.overall_scores(per_group, R.DEFAULT_CRITERIA))
    score_tol = 4 * np.concatenate(tols) + U24
    rel = np.abs(scores[:row0] - want_scores) / np.abs(want_scores)
    print(f"scores: max rel err {rel.max():.3e}, tol {score_tol.min():.3e} .. {score_tol.max():.3e}")
    assert (rel <= score_tol).all()
    assert [sorted(x.active) for x in opt._prune.groups] == [sorted(x.active) for x in f64.groups]


# ---- the joint step ---------------------------------------------------------------------------------------------
# in units: heads of l0 (3), l1 (2) and l3 (2), rows of l2 (33). "none": a head group beside joint ones has no
# redundant head
REDUNDANT = {"none": ([1], [], [17], [0]), "scattered": ([0, 2], [1], [1, 5, 8, 13, 32], [1]),
             "all": ([0, 1], [0], list(range(32)), [0])}
PRUNED = ([2], [1], [2, 30], [1])
TIE_REACH = 2.0 ** -20


def near_tie(w, d, q_m, t):
    """Elements of the float64 weight w whose code rint(|w|^t / d) fp32 may round the other way."""
    _, res, qw = R.clip_res_quant_f64(w, d, q_m, t)
    return 0.5 - np.abs(res) <= np.abs(qw / d) * TIE_REACH


def _install(groups, redundant, pruned=PRUNED):
    for g, a, p in zip(groups, redundant, pruned):
        g.active, g.pruned = list(a), [r for r in p if r not in a]
        g.important = [i for i in range(g.num_groups) if i not in g.active and i not in g.pruned]


def _joint_ref(units, kind, seed=3, variant="sgd_plain", nonlinear=True, pruned=PRUNED):
    """Parameters, gradients and both reference forms after the joint step with the redundant `units` per layer."""
    kw = dict(JOINT_KW, **VARIANTS[variant])
    net = C.make_net(torch.device("cpu"), seed, nonlinear)
    rows = C.physical_rows(units)
    steer_signs(net, rows, kind)
    start = host_params(net)
    grads = joint_grads(start, rows, kind, seed)
    forms = ref_forms(start, kw)
    for o in forms:
        o.curr_period, o.num_steps = 1, 1
        _install(o.groups, units, pruned)
    forms[0].step(P.permute(np_dict(grads), C.SPECS))
    forms[1].step(P.permute(grads, C.SPECS))
    return start, grads, forms, kw


def _joint_device(dev, start, units, kw, nonlinear=True, pruned=PRUNED):
    net = C.make_net(dev, 0, nonlinear)
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.copy_(start[name].to(dev))
    opt = make_opt(net, **kw)
    opt.num_steps = 1
    opt._prune.curr_period = 1
    _install(opt._prune.groups, units, pruned)
    opt._prune._tables()
    return net, opt


JOINT_CASES = [(s, k, True) for s in REDUNDANT for k in KINDS] + \
              [("scattered", k, False) for k in ("pos", "neg", "loop")]


def _ties(f64, start_u):
    """{member: near_tie mask over the group's active units} for the quantized members of the joint groups."""
    out = {}
    for g in f64.groups:
        if g.active:
            m = f"{g.layer}.weight"
            gamma, d, _ = f64.last[g.name]
            _, q, t = f64._wt_scalars(g.layer)
            out[m] = near_tie(start_u[m][g.active].astype(np.float64), d, q, t)
    return out


@pytest.fixture(scope="module")
def joint_refs():
    """Every case's reference run and the measured reach of fp32: the largest relative difference between the fp32
    torch form and the float64 form over ALL these inputs, per quantity; for the rows, over the elements that are not
    at a rounding tie of the quantizer (module docstring)."""
    runs, rel, nties = {}, {"gamma": 0.0, "d": 0.0, "rows": 0.0, "rows_with_ties": 0.0}, 0
    for sets, kind, nonlinear in JOINT_CASES:
        start, grads, (f64, th), kw = _joint_ref(REDUNDANT[sets], kind, nonlinear=nonlinear)
        ties = _ties(f64, P.permute(np_dict(start), C.SPECS))
        runs[sets, kind, nonlinear] = start, grads, (f64, th), kw, ties
        for g in f64.groups:
            if not g.active:
                continue
            (ga, da, _), (gb, db, _) = f64.last[g.name], th.last[g.name]
            if ga:
                rel["gamma"] = max(rel["gamma"], abs(ga - gb) / abs(ga))
            rel["d"] = max(rel["d"], abs(da - db) / abs(da))
            for m in g.members:
                a, b = f64.p[m][g.active], th.p[m][g.active].double().numpy()
                diff = np.abs(a - b) / np.abs(a).max()
                rel["rows_with_ties"] = max(rel["rows_with_ties"], float(diff.max()))
                if m in ties:
                    nties += int(ties[m].sum())
                    diff = diff[~ties[m]]
                rel["rows"] = max(rel["rows"], float(diff.max()))
    print("measured (b)-(a), relative:", {k: f"{v:.3e}" for k, v in rel.items()}, f"{nties} elements at a tie")
    return runs, rel


@pytest.mark.parametrize("sets,kind,nonlinear", JOINT_CASES,
                         ids=[f"{s}-{k}{'' if n else '-linear'}" for s, k, n in JOINT_CASES])
def test_joint_step(dev, joint_refs, sets, kind, nonlinear):
    runs, rel = joint_refs
    start, grads, (f64, th), kw, ties = runs[sets, kind, nonlinear]
    net, opt = _joint_device(dev, start, REDUNDANT[sets], kw, nonlinear)
    set_grads(net, grads, dev)
    opt.step()
    got_phys = host_params(net)
    got = P.permute(got_phys, C.SPECS)
    gamma, info = opt._prune.gamma.cpu().numpy().astype(np.float64), opt._prune.info.cpu().numpy()
    seen = set()
    for i, g in enumerate(f64.groups):
        if not g.active:
            assert int(info[i]) == -1 and g.name not in f64.last
        else:
            ga, da, ia = f64.last[g.name]
            ib = th.last[g.name][2]
            sums, count = f64.last_six[g.name]
            if kind != "zero":
                assert R.margins(*sums, count) >= 1e-3, (g.name, R.margins(*sums, count))
            assert ia == ib == int(info[i]), (g.name, ia, ib, int(info[i]))
            assert ia & 7 == KINDS[kind]
            seen.add(ia)
            for what, a, dv in (("gamma", ga, gamma[i]), ("d", da, float(got[f"l{i}.d_quant_wt"]))):
                tol = max(4 * rel[what] * abs(a), float(_ulp32(a)))
                print(f"{g.name} {what}: device {dv:.9e} f64 {a:.9e} err {abs(dv - a):.2e} tol {tol:.2e}")
                assert abs(dv - a) <= tol, (g.name, what)
        for m in g.members:
            if g.active:
                a, dv = f64.p[m][g.active], got[m][g.active].double().numpy()
                tol = np.maximum(4 * rel["rows"] * np.abs(a).max(), _ulp32(a))
                if m in ties:   # one code step more where fp32 may take the neighbouring code
                    tol = tol + ties[m] * abs(f64.last[g.name][0] * f64.last[g.name][1])
                err = np.abs(dv - a)
                print(f"{m} redundant units: max err {err.max():.2e}, tol {tol.min():.2e} .. {tol.max():.2e}")
                assert (err <= tol).all(), m
            if g.pruned:
                assert not got[m][g.pruned].any(), m
                assert not got_phys[m][C.physical_rows([x.pruned for x in f64.groups])[i]].any(), m
    if kind == "res_pos":
        assert all(i & R.D_UPPER for i in seen)
    if kind == "loop":
        assert all(i & R.LOOPED for i in seen)
    if kind == "min":
        assert all(i & R.MIN_UPPER for i in seen)
    if kind in ("pos", "neg"):
        assert not any(i & R.D_UPPER for i in seen)


def test_important_heads_take_the_dense_step_without_decay_and_pruned_heads_are_zeros(dev):
    """Against the dense launch of an optimizer without groups on the same rows, bitwise, over two steps."""
    from quantized_vit_amd import QuantAwareOptimizer
    units = ([0], [1], [1, 5, 8, 13, 32], [0])       # redundant, every group joint
    pruned_units = ([2], [], [2, 30], [])            # beside them: head 2 of l0, rows 2 and 30 of l2
    start, grads, _, kw = _joint_ref(units, "pos", seed=4, variant="adamw", pruned=pruned_units)
    net, opt = _joint_device(dev, start, units, kw, pruned=pruned_units)
    plain = C.make_net(dev, 0)
    with torch.no_grad():
        for name, p in plain.named_parameters():
            p.copy_(start[name].to(dev))
    kw2 = {k: v for k, v in kw.items() if k not in ("start_pruning_step", "pruning_steps", "pruning_periods")}
    dense = QuantAwareOptimizer(plain, **dict(kw2, weight_decay=None, fix_after_step=5))
    dense.num_steps = 1
    for _ in range(2):
        set_grads(net, grads, dev)
        set_grads(plain, grads, dev)
        opt.step()
        dense.step()
    a, b = host_params(net), host_params(plain)
    red_rows, pruned_rows = C.physical_rows(units), C.physical_rows(pruned_units)
    assert pruned_rows[0] and red_rows[1] and len(pruned_rows[0]) == 3 * 4
    for i in range(C.NGROUPS):
        keep = [r for r in range(C.ROWS[i]) if r not in red_rows[i] and r not in pruned_rows[i]]
        assert keep
        for leaf in ("weight", "bias"):
            assert torch.equal(a[f"l{i}.{leaf}"][keep], b[f"l{i}.{leaf}"][keep]), (i, leaf)
            z = a[f"l{i}.{leaf}"][pruned_rows[i]]
            assert z.numel() == 0 or (not z.any() and not torch.signbit(z).any()), (i, leaf)
    sa, sb = opt.state_dict(), dense.state_dict()
    for u, v in zip(sa["first_moments"] + sa["second_moments"], sb["first_moments"] + sb["second_moments"]):
        assert torch.equal(u, v)


def test_two_runs_give_the_same_bits(dev):
    """Plain step, boundary step (scores, fold, selection, joint), joint step: twice, from the same inputs."""
    kw = dict(BASE, **VARIANTS["adamw"], start_pruning_step=1, pruning_steps=4, pruning_periods=1)
    runs = []
    for _ in range(2):
        net = C.make_net(dev, 5)
        start = host_params(net)
        opt = make_opt(net, **kw)
        for s in range(3):
            set_grads(net, make_grads(start, s), dev)
            opt.step()
        pr = opt._prune
        assert pr.curr_period == 1 and pr._nred > 0
        runs.append((host_params(net), pr._scores.cpu(), pr._unit_sums.cpu(), pr._sums.cpu(), pr.gamma.cpu(),
                     pr.info.cpu(), [list(g.active) for g in pr.groups], opt.state_dict()))
    a, b = runs
    assert all(torch.equal(a[0][k], b[0][k]) for k in a[0])
    for x, y in zip(a[1:6], b[1:6]):
        assert torch.equal(x, y)
    assert a[6] == b[6]
    for key in ("first_moments", "second_moments"):
        assert all(torch.equal(u, v) for u, v in zip(a[7][key], b[7][key]))


def test_the_fold_gives_zeros_to_a_unit_whose_row_items_disagree(dev):
    """qvit_prune_scores_fold compares every row item it reads with the unit that names it. One row item each with a
    wrong group, a wrong row and a wrong link: the three units they belong to get zero sums, every other unit the
    bits of the fold over the untouched tables."""
    from quantized_vit_amd import _lib
    kw = dict(BASE, **VARIANTS["sgd_plain"], start_pruning_step=1, pruning_steps=1, pruning_periods=1)
    net = C.make_net(dev, 6)
    opt = make_opt(net, **kw)
    set_grads(net, make_grads(host_params(net), 0), dev)
    opt.step()                                   # a boundary step: row sums and tables are on the device
    pr = opt._prune
    assert pr.curr_period == 1 and pr.order == [0, 1, 2, 3]
    good = pr._unit_sums.clone()
    assert (good[:, 0] > 0).all()
    items = pr._items.copy()
    base = np.cumsum([0] + list(C.ROWS))         # a group's row 0 in the items
    unit0 = np.cumsum([0] + list(C.UNITS))       # a group's unit 0 in the units
    r = base[0] + 1 * 4 + 2                      # l0: head 1, section 0, j = 2 -> names group 2
    items["group"][r] = 2
    r = base[1] + (1 * 2 + 0) * 64 + 7           # l1: head 0, section 1, j = 7 -> names the row after it
    items["row"][r] += 1
    r = base[3] + (2 * 2 + 1) * 4 + 3            # l3: head 1, section 2, j = 3 -> carries unit 0
    items["link"][r] = 0
    bad = {unit0[0] + 1, unit0[1] + 0, unit0[3] + 1}
    table = torch.from_numpy(items.view(np.int64)).to(dev)
    out = torch.full_like(good, -1.0)
    lib = _lib.load()
    st = lib.qvit_prune_scores_fold(_lib._ptr(pr._gtable.dev), len(pr.groups), _lib._ptr(table), pr.nprunable_rows,
                                    _lib._ptr(pr._sums), _lib._ptr(pr._utable.dev), pr.total_num_groups,
                                    _lib._ptr(out), _lib._stream(dev))
    assert st == 0
    out = out.cpu()
    for u in range(pr.total_num_groups):
        if u in bad:
            assert not out[u].any(), u
        else:
            assert torch.equal(out[u], good[u].cpu()), u


# ---- the schedule, end to end ---------------------------------------------------------------------------------------
def _criteria_kw(criteria):
    return {} if criteria is None else dict(importance_score_criteria=criteria)


def _vit_opt(model, criteria):
    from quantized_vit_amd import QuantAwareOptimizer, vit_head_prune_groups, vit_mlp_prune_groups
    return QuantAwareOptimizer(model, prune_groups=vit_head_prune_groups(model) + vit_mlp_prune_groups(model),
                               **SCHEDULE, **_criteria_kw(criteria))


@pytest.fixture(scope="module", params=["cosine", "default"])
def schedule_run(request, dev):
    """NSTEPS steps with head and MLP groups in one ranking. "default": the reference's default criteria, under which no
    head of this model is ever taken (tests/test_prune_heads_cpu.py); "cosine": the cosine criterion alone, under which
    three heads of each block go."""
    criteria = C.COSINE if request.param == "cosine" else None
    model = C.head_vit(dev)
    start = host_params(model)
    opt = _vit_opt(model, criteria)
    ref = PruneF64(P.permute(np_dict(start), C.VIT_SPECS), PruneHyper(**SCHEDULE, criteria=criteria),
                   C.vit_ref_groups())
    rows_dev, rows_ref, ckpt, synced = [], [], None, []
    for s in range(NSTEPS):
        g = C.vit_grads(start, s)
        set_grads(model, g, dev)
        boundary = opt._prune._boundary(s + 1)
        nred = opt._prune._nred
        if not boundary:
            torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        synced.append((s + 1, boundary, nred))
        ref.step(P.permute(np_dict(g), C.VIT_SPECS))
        rows_dev.append((opt.pruned_rows(), [sorted(x.active) for x in opt._prune.groups]))
        rows_ref.append((ref.pruned_rows(), [sorted(x.active) for x in ref.groups]))
        if s + 1 == 6:
            ckpt = (copy.deepcopy(opt.state_dict()), {k: v.clone() for k, v in model.state_dict().items()})
    return dict(model=model, opt=opt, ref=ref, start=start, rows_dev=rows_dev, rows_ref=rows_ref, ckpt=ckpt,
                synced=synced, criteria=criteria)


def test_schedule_selects_the_reference_sets_and_reaches_the_target_in_units(schedule_run):
    r = schedule_run
    assert r["rows_dev"] == r["rows_ref"]
    assert [b for _, b, _ in r["synced"]] == [n in (3, 6) for n in range(1, NSTEPS + 1)]
    assert any(nred for _, b, nred in r["synced"] if not b), "no joint step ran under the sync check"
    opt, ref = r["opt"], r["ref"]
    final = opt.pruned_rows()
    assert opt._prune.total_num_groups == 2 * C.VIT_HEADS + 2 * C.VIT_HIDDEN
    assert sum(len(v) for v in final.values()) == ref.target == opt._prune.target
    m, mr = opt.prune_metrics(), ref.prune_metrics()
    assert m["num_zero_groups"] == mr["num_zero_groups"] == ref.target
    assert m["num_important_groups"] == mr["num_important_groups"]
    assert m["num_redundant_groups"] == mr["num_redundant_groups"] == ref.target
    assert opt.fixed and opt.stage() == 2
    heads = [final[f"blocks.{i}.attn"] for i in range(2)]
    if r["criteria"] is not None:
        assert any(heads) and all(len(h) < C.VIT_HEADS for h in heads)
    for i, blk in enumerate(r["model"].blocks):
        w, b = blk.attn.qkv.weight, blk.attn.qkv.bias
        dead = P.rows_of_units(heads[i], C.VIT_HEADS, C.VIT_HD)
        assert not w[dead].any() and not b[dead].any()
        live = [x for x in range(3 * C.VIT_HEADS * C.VIT_HD) if x not in dead]
        assert w[live].abs().sum(dim=1).min() > 0
        rows = final[f"blocks.{i}.mlp"]
        assert not blk.mlp.fc1.weight[rows].any() and not blk.mlp.fc1.bias[rows].any()


def test_a_mid_period_checkpoint_continues_identically(dev, schedule_run):
    state, params = schedule_run["ckpt"]
    assert any(state["pruning"]["active_redundant_idxes"])
    if schedule_run["criteria"] is not None:
        assert any(state["pruning"]["active_redundant_idxes"][:2]), "no head was redundant at the checkpoint"
    model = C.head_vit(dev)
    model.load_state_dict(params)
    opt = _vit_opt(model, schedule_run["criteria"])
    opt.load_state_dict(state)
    for s in range(6, NSTEPS):
        set_grads(model, C.vit_grads(schedule_run["start"], s), dev)
        opt.step()
    a, b = host_params(model), host_params(schedule_run["model"])
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert opt.pruned_rows() == schedule_run["opt"].pruned_rows()


def test_groups_that_prune_nothing_leave_the_bits_of_the_run_without_groups(dev):
    """Head and MLP members go through qvit_prune_joint_apply, boundaries and the fold run (target 0): parameters,
    moments, quantizer moments and fixed bit widths equal those of the optimizer without groups."""
    from quantized_vit_amd import QuantAwareOptimizer, vit_head_prune_groups, vit_mlp_prune_groups
    plain = {k: v for k, v in SCHEDULE.items() if not k.startswith(("pruning", "start_pruning", "target"))}
    kws = (dict(plain, projection_steps=100, fix_after_step=8),
           dict(SCHEDULE, projection_steps=100, target_group_sparsity=0.0))
    runs, start = [], None
    for kw in kws:
        model = C.head_vit(dev)
        start = host_params(model) if start is None else start
        groups = vit_head_prune_groups(model) + vit_mlp_prune_groups(model) if kw is kws[1] else None
        opt = QuantAwareOptimizer(model, prune_groups=groups, **kw)
        for s in range(NSTEPS):
            set_grads(model, C.vit_grads(start, s), dev)
            opt.step()
        runs.append((host_params(model), opt.state_dict(), opt))
    (pa, sa, oa), (pb, sb, ob) = runs
    assert oa.fixed and ob.fixed and ob._prune.curr_period == 2 and ob._prune.folded
    assert all(torch.equal(pa[k], pb[k]) for k in pa)
    for key in ("first_moments", "second_moments"):
        assert all(torch.equal(u, v) for u, v in zip(sa[key], sb[key]))
    assert torch.equal(sa["quant_moments"], sb["quant_moments"]) and torch.equal(sa["fixed_bits"], sb["fixed_bits"])
    assert sb["pruning"]["pruned_idxes"] == [[], [], [], []]   # two head groups, two MLP groups
