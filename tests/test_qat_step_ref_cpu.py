"""The two restatements of tests/qat_step_ref.py against each other and against the reference's documented quirks;
the optimizer's host-side schedule against theirs. Runs without a GPU."""
import math

import numpy as np
import pytest
import torch

from qat_step_ref import FIX, RANGE, WARMUP, Hyper, StepF64, StepTorch, bit_width, d_of_bits

VARIANTS = {
    "sgd": dict(variant="sgd", first_momentum=0.9, dampening=0.1, weight_decay=1e-2),
    "adam": dict(variant="adam", first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2),
    "adamw": dict(variant="adamw", first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2),
}
STAGES = {
    WARMUP: dict(start_projection_step=10, fix_after_step=20),
    RANGE: dict(start_projection_step=0, projection_steps=2, projection_periods=1, fix_after_step=100),
    FIX: dict(start_projection_step=0, fix_after_step=0),
}


def problem(seed, layers=("l1", "l10")):
    """Two layers whose names are substrings of one another, one nonlinear with activations, one linear."""
    g = torch.Generator().manual_seed(seed)
    p = {"w": torch.randn(301, generator=g) * 0.5, "b": torch.randn(7, generator=g)}
    for i, layer in enumerate(layers):
        sides = ("wt", "act") if i == 0 else ("wt",)
        for side in sides:
            q = 0.8 + 0.4 * torch.rand(1, generator=g)
            p[f"{layer}.d_quant_{side}"] = (1.0 + 0.1 * torch.rand(1, generator=g)) / 127.0
            p[f"{layer}.q_m_{side}"] = q
            if i == 0:
                p[f"{layer}.t_quant_{side}"] = 0.95 + 0.1 * torch.rand(1, generator=g)
    return p


def grads_for(p, seed, steps):
    g = torch.Generator().manual_seed(100 + seed)
    return [{k: torch.randn(v.shape, generator=g) * (0.05 if v.numel() == 1 else 1.0) for k, v in p.items()}
            for _ in range(steps)]


@pytest.mark.parametrize("stage", [WARMUP, RANGE, FIX], ids=["warmup", "range", "fix"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_two_restatements_agree_over_four_steps(variant, stage):
    hp = Hyper(**VARIANTS[variant], **STAGES[stage])
    p = problem(1)
    a, b = StepF64({k: v.numpy() for k, v in p.items()}, hp), StepTorch(p, hp)
    for g in grads_for(p, 1, 4):
        assert a.step({k: v.numpy() for k, v in g.items()}) == stage and b.step(g) == stage
        for k in p:
            ref = a.p[k].reshape(-1)
            err = np.abs(b.p[k].double().numpy().reshape(-1) - ref).max()
            assert err <= 1e-6 * np.abs(ref).max(), (k, err)
        for store_a, store_b in ((a.m, b.m), (a.v, b.v)):
            assert set(store_a) == set(store_b)
            for k in store_a:
                ref = store_a[k].reshape(-1)
                assert np.abs(store_b[k].double().numpy().reshape(-1) - ref).max() <= 1e-6 * np.abs(ref).max(), k
    assert a.bits == b.bits and (stage != FIX or set(a.bits) == {"l1", "l10"})


def test_bit_schedule_goes_16_14_to_6_and_stops():
    from quantized_vit_amd.qat_optim import bit_schedule_step
    hp = Hyper(start_projection_step=2, projection_steps=30, projection_periods=10, fix_after_step=1000, min_bit_wt=2,
               min_bit_act=4)
    m = StepF64({}, hp)
    seen_wt, mine = [m.max_bit_wt], 16
    for n in range(1, 41):
        assert m.advance() == (WARMUP if n <= 2 else RANGE)
        mine = bit_schedule_step(n, 2, 1000, 3, 2, 2, mine)
        assert mine == m.max_bit_wt == m.max_bit_act
        if m.max_bit_wt != seen_wt[-1]:
            seen_wt.append(m.max_bit_wt)
            assert (n - 2 - 1) % 3 == 0
    assert seen_wt == [16, 14, 12, 10, 8, 6]   # the hard floor of 6 although min_bit is 2
    assert bit_schedule_step(1001, 2, 1000, 3, 2, 2, 16) == 16   # no reduction once the fix stage runs


def test_first_step_moments_are_unscaled():
    """base_optimizer.py:20-21, :31-32."""
    p = {"w": torch.tensor([0.5, -1.0])}
    g = {"w": torch.tensor([0.25, 2.0])}
    hp = Hyper(variant="adam", lr=0.1, first_momentum=0.9, second_momentum=0.999, start_projection_step=5)
    b = StepTorch(p, hp)
    b.step(g)
    assert torch.equal(b.m["w"], g["w"]) and torch.equal(b.v["w"], g["w"] ** 2)
    want = p["w"].double() - 0.1 * (g["w"].double() / (1 - 0.9)) / ((g["w"].double() ** 2 / (1 - 0.999)).sqrt() + 1e-8)
    assert torch.allclose(b.p["w"].double(), want, rtol=1e-6, atol=0)
    b.step(g)   # from the second step on the moments are the usual averages
    assert torch.allclose(b.m["w"], g["w"] * 0.9 + g["w"] * 0.1)


def test_range_stage_steps_activation_scalars_twice():
    """geta.py:598-630 then :667-697."""
    p = problem(2)
    g = grads_for(p, 2, 1)[0]
    hp = Hyper(variant="sgd", lr=1e-2, lr_quant=1e-3, **STAGES[RANGE])
    a = StepF64({k: v.numpy() for k, v in p.items()}, hp)
    a.step({k: v.numpy() for k, v in g.items()})
    for name, rate in (("l1.q_m_act", 1e-2 + 1e-3), ("l1.t_quant_act", 1e-2 + 1e-3), ("l1.q_m_wt", 1e-3),
                       ("l10.q_m_wt", 1e-3), ("w", 1e-2)):
        assert np.allclose(a.p[name], p[name].double().numpy() - rate * g[name].double().numpy(), rtol=1e-12), name
    # under adamw the first of the two decays at lr, the second at lr_quant
    hp = Hyper(variant="adamw", lr=1e-2, lr_quant=1e-3, first_momentum=0.9, second_momentum=0.999, weight_decay=0.1,
               **STAGES[RANGE])
    a = StepF64({k: v.numpy() for k, v in p.items()}, hp)
    a.step({k: v.numpy() for k, v in g.items()})
    q0, gq = float(p["l1.q_m_act"]), float(g["l1.q_m_act"])
    gv = (gq / (1 - 0.9)) / (math.sqrt(gq * gq / (1 - 0.999)) + 1e-8)
    q1 = q0 - 1e-2 * 0.1 * q0 - 1e-2 * gv
    assert math.isclose(float(a.p["l1.q_m_act"][0]), q1 - 1e-3 * 0.1 * q1 - 1e-3 * gv, rel_tol=1e-12)


def test_a_layer_takes_its_own_scalars_not_a_substring_match():
    """The reference's `layer_name in p_name` would give "l1" the q_m of "l10" (the later match wins)."""
    p = problem(3)
    p["l10.q_m_wt"] = torch.tensor([5.0])
    hp = Hyper(variant="sgd", **STAGES[RANGE])
    a = StepF64({k: v.numpy() for k, v in p.items()}, hp)
    lo, hi = a.bounds("l1", "wt")
    q, t = float(p["l1.q_m_wt"]), float(p["l1.t_quant_wt"])
    assert lo == d_of_bits(16, q, t) and hi == d_of_bits(4, q, t)
    assert a.bounds("l10", "wt")[1] == d_of_bits(4, 5.0, None)


def test_rint_is_pythons_round_at_the_halves():
    xs = np.arange(-3.5, 9.0, 1.0)
    assert [int(v) for v in np.rint(xs)] == [round(float(v)) for v in xs]
    # a bit width that lands on x.5 exactly: q_m = 1, t = 1, d = 1 / (2^5.5 - 1) gives 6.5 or its neighbour
    d = 1.0 / (2 ** 5.5 - 1)
    b = bit_width(d, 1.0, None)
    assert round(b) == int(np.rint(b))
    assert round(6.5) == 6 and round(7.5) == 8 and np.rint(6.5) == 6 and np.rint(7.5) == 8
