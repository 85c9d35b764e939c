"""tests/quant_error_ref.py against hand-computed cases, and the conditions the GPU tests rely on: every seeded data
set of the selection test has a best candidate that beats the runner-up by a relative gap of at least 1e-6 (far above
the summation-order and power-rounding differences the device may show), so the device argmin is well defined. A seed
that fails this is replaced in quant_error_ref.SELECTION_SETS; the GPU test is not loosened."""
import numpy as np
import pytest
import torch

import quant_error_ref as R


def test_three_elements_two_candidates_linear():
    x = torch.tensor([0.3, -1.0, 2.5], dtype=torch.float32)
    # candidate 0: d = 0.5, q_m = 2 (saturation code rne(2 / 0.5) = 4, value 2); candidate 1: d = 1, q_m = 3
    err, nclip = R.quant_error(x, 0, [0.5, 1.0], [2.0, 3.0])
    f = lambda v: float(np.float32(v))
    # c0: 0.3 -> 0.5 rne(0.6) = 0.5; -1 -> -1; 2.5 >= 2 -> 2.    c1: 0.3 -> 0; -1 -> -1; 2.5 -> rne(2.5) = 2 (half to even)
    want0 = (f(0.3) - 0.5) ** 2 + 0.0 + 0.5 ** 2
    want1 = f(0.3) ** 2 + 0.0 + 0.5 ** 2
    assert err.dtype == torch.float64 and nclip.dtype == torch.int64
    assert err.tolist() == [want0, want1]
    assert nclip.tolist() == [1, 0]


def test_clip_count_boundary():
    q_m = np.float32(1.7)
    below = np.nextafter(q_m, np.float32(0), dtype=np.float32)
    x = torch.tensor([q_m, -q_m, below, -below, 0.0], dtype=torch.float32)
    for qtype, t in ((0, 1.0), (1, 0.9)):
        _, nclip = R.quant_error(x, qtype, [0.1], [float(q_m)], t)
        assert nclip.tolist() == [2], (qtype, nclip)


def test_nonlinear_target_is_the_unrounded_power():
    x = torch.tensor([0.5, -0.25, 0.0], dtype=torch.float32)
    t = 1.25
    p = R.target(x, 1, t)
    want = torch.sign(x) * torch.exp(torch.tensor([t]) * torch.log(x.abs()))
    assert torch.equal(p, want) and p[2] == 0 and p[1] < 0
    # one element, by hand: p = 0.5^1.25, d = 0.1 -> code rne(p / 0.1) = 4, fq = 0.4
    err, _ = R.quant_error(x[:1], 1, [0.1], [10.0], t)
    assert err.item() == (float(p[0]) - float(np.float32(0.1) * np.float32(4.0))) ** 2


def test_nan_and_inf_are_not_masked():
    x = torch.tensor([0.5, float("nan"), 1.0], dtype=torch.float32)
    for qtype in (0, 1):
        err, nclip = R.quant_error(x, qtype, [0.1, 0.2], [0.8, 2.0], 0.9)
        assert torch.isnan(err).all() and nclip.tolist() == [1, 0]
    err, nclip = R.quant_error(torch.tensor([float("inf")]), 0, [0.1], [0.8])
    assert not torch.isfinite(err).any() and nclip.tolist() == [1]


def test_last_candidate_is_the_absmax_choice():
    q_m, d = R.candidates(3.0, 8, 1.0, 32)
    assert q_m[-1].item() == 3.0 and d[-1].item() == float(np.float32(3.0 / 127))
    assert q_m[0].item() == float(np.float32(3.0 * 0.2)) and bool((q_m[1:] > q_m[:-1]).all())


def test_argmin_ties_go_to_the_larger_q_m():
    assert R.argmin_larger_qm(torch.tensor([3.0, 1.0, 2.0, 1.0, 5.0])) == 3


@pytest.mark.parametrize("kind,bits,seed", R.SELECTION_SETS)
@pytest.mark.parametrize("qtype,t", [(0, 1.0), (1, 0.9)])
def test_selection_sets_have_a_clear_winner(kind, bits, seed, qtype, t):
    x, q_m, d = R.selection_case(kind, bits, seed, qtype, t)
    err, _ = R.quant_error(x, qtype, d, q_m, t)
    e = np.sort(err.numpy())
    gap = (e[1] - e[0]) / e[0]
    best = R.argmin_larger_qm(err)
    print(kind, bits, seed, qtype, "best", best, "gap", gap)
    assert gap >= 1e-6, (kind, seed, gap)
    assert 0 < best < len(e) - 1, "the minimum should be interior: a clip that pays"
