"""The CPU restatement of ultra_bn_fuse.hip (tests/ultra_bn_fuse_ref.py) against float64 autograd of
F.batch_norm(training=True) -> clamp(0, 1) -> straight-through round -> F.max_pool2d and against nn.BatchNorm2d's
buffers, and the conditions on the GPU tests' inputs, checked on the reference alone."""
import pytest
import torch
import torch.nn as nn

import ultra_bn_fuse_ref as R

EPS = 1e-5
SHAPES = [(2, 3, 5, 7), (2, 4, 6, 8), (1, 2, 9, 9)]   # odd H and W, even, odd single image


def _restated(x, gamma, beta, levels, pool, g, dtype=torch.float64):
    mean, var, invstd, _, _ = R.stats(x, EPS, dtype=dtype)
    codes, flags, _ = R.forward(x, mean, invstd, gamma, beta, levels, pool)
    dx, dgamma, dbeta = R.backward(x, g, flags, mean, invstd, gamma, pool, dtype=dtype)
    return codes, flags, dx, dgamma, dbeta


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("a_bit", [2, 4, 7])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("tied", [False, True])
def test_restatement_equals_float64_autograd(shape, a_bit, pool, affine, tied):
    levels = 2 ** a_bit - 1
    full = (*shape, pool)
    x, gamma, beta = R.gen_case(full, levels, affine, seed=a_bit * 17 + int(pool))
    if tied:
        x = R.gen_tied(full, seed=a_bit)
    g = R.gen_grad(full, seed=5)
    out, dx, dgamma, dbeta = R.autograd_truth(x, gamma, beta, EPS, levels, pool, g)
    codes, flags, rdx, rdgamma, rdbeta = _restated(x, gamma, beta, levels, pool, g)
    assert torch.equal(torch.round(out * levels).to(torch.int64), codes)
    assert R.rel(codes.double() / levels, out) <= 2.0 ** -50
    if tied and pool and levels == 3:   # the tie rule is exercised: windows whose maximum occurs more than once
        kw = R._windows(R.forward(x, *R.stats(x, EPS)[0:3:2], gamma, beta, levels, False)[0])
        assert int(((kw == kw.amax(-1, keepdim=True)).sum(-1) > 1).sum()) > 0
    assert R.rel(rdx, dx) <= 1e-10
    if affine:
        assert R.rel(rdgamma, dgamma) <= 1e-10 and R.rel(rdbeta, dbeta) <= 1e-10


def test_all_equal_window_sends_the_gradient_top_left():
    x = torch.zeros(2, 1, 2, 2)
    x[1] = 1.0   # image 0: one window of four equal values below the mean, image 1: above
    g = torch.tensor([[[[3.0]]], [[[5.0]]]])
    mean, var, invstd, _, _ = R.stats(x, EPS)
    codes, flags, _ = R.forward(x, mean, invstd, torch.tensor([0.25]), torch.tensor([0.5]), 15, True)
    assert flags.flatten().tolist() == [1, 1]   # winner 0, passing
    gy = R.grad_y(g.double(), flags, x.shape, True)
    assert gy[:, 0].flatten().tolist() == [3.0, 0, 0, 0, 5.0, 0, 0, 0]
    out, dx, _, _ = R.autograd_truth(x, torch.tensor([0.25]), torch.tensor([0.5]), EPS, 15, True, g)
    rdx = R.backward(x, g, flags, mean, invstd, torch.tensor([0.25]), True)[0]
    assert R.rel(rdx, dx) <= 1e-10


@pytest.mark.parametrize("momentum", [0.1, 0.37, None])
@pytest.mark.parametrize("affine", [True, False])
def test_running_statistics_equal_batchnorm2d(momentum, affine):
    bn = nn.BatchNorm2d(3, eps=EPS, momentum=momentum, affine=affine).double().train()
    rm, rv, nbt = bn.running_mean.clone(), bn.running_var.clone(), 0
    for step in range(3):
        x = R.gen_case((2, 3, 5, 7, False), 15, seed=step)[0].double()
        bn(x)
        nbt += 1
        factor = 1.0 / nbt if momentum is None else momentum
        _, _, _, rm, rv = R.stats(x, EPS, factor, rm, rv)
        assert int(bn.num_batches_tracked) == nbt
        assert R.rel(rm, bn.running_mean) <= 1e-12 and R.rel(rv, bn.running_var) <= 1e-12


def _case_reference(shape, levels, seed_shape=None, affine=True):
    x, gamma, beta = R.gen_case(shape, levels, affine,
                                seed=None if seed_shape is None else R.case_seed(seed_shape, levels))
    mean, var, invstd, _, _ = R.stats(x, EPS)
    # the GPU test feeds the device's fp32 statistics: round them as the device does
    return x, R.forward(x, mean.float(), invstd.float(), gamma, beta, levels, shape[4])


@pytest.mark.parametrize("shape,levels", R.CASES)
def test_gpu_cases_are_nearly_tie_free(shape, levels):
    """At most TIE_CAP of each GPU parametrisation lies inside the possible-tie / clamp-edge margin (derived in
    ultra_bn_fuse_ref.py), so the tie-proven comparison is not vacuous. Every quantizer code 0..levels (before the
    pool, which keeps the larger ones) occurs in every case with at least 32 elements per code; smaller cases cannot
    hold them all and are covered by the union below."""
    for affine in (True, False):   # the forward test runs both forms
        x, (codes, flags, tie) = _case_reference(shape, levels, affine=affine)
        share = float(tie.double().mean())
        print(f"{shape} levels {levels} affine {affine}: possible ties {share:.3e}")
        assert share <= R.TIE_CAP
    if x.numel() >= 32 * (levels + 1):
        assert torch.unique(_case_reference(shape[:4] + (False,), levels, shape)[1][0]).tolist() == \
            list(range(levels + 1))


@pytest.mark.parametrize("levels", R.LEVELS)
def test_gpu_cases_reach_every_code(levels):
    seen = set()
    for shape in R.SHAPES:
        seen |= set(_case_reference(shape[:4] + (False,), levels, shape)[1][0].flatten().tolist())
    assert seen == set(range(levels + 1))


def test_margin_covers_an_fp32_evaluation():
    """The derived margin against an actual fp32 evaluation of fmaf(x - mean, a, beta) * levels (torch float32, no
    fused multiply-add: one rounding more than the kernel): every code that differs from float64's is flagged."""
    for shape, levels in R.CASES:
        x, gamma, beta = R.gen_case(shape, levels)
        mean, var, invstd, _, _ = R.stats(x, EPS)
        mean, invstd = mean.float(), invstd.float()
        codes, flags, tie = R.forward(x, mean, invstd, gamma, beta, levels, False)
        y32 = (x - mean.view(1, -1, 1, 1)) * (gamma * invstd).view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
        k32 = torch.round(y32.clamp(0, 1) * float(levels)).to(torch.int64)
        p32 = ((y32 >= 0) & (y32 <= 1)).to(torch.uint8)
        assert not bool(((k32 != codes) & ~tie).any()) and not bool(((p32 != flags) & ~tie).any())
