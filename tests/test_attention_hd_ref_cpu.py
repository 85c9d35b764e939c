"""attention_hd_ref.py (the attention reference with the head width as a parameter) pinned to the width-64 helper it
generalises, and its closed-form gradients pinned to float64 autograd at width 80."""
import pytest
import torch

import attention_backward_ref as R64
import attention_hd_ref as R


@pytest.mark.parametrize("B,N,H", [(1, 5, 2), (2, 33, 2)])
def test_width_64_is_the_existing_helper(B, N, H):
    scale = 64 ** -0.5
    qkv, dO = R.make_inputs(B, N, H, 64, 3, 1.5, 0.5, 2.0)
    qkv0, dO0 = R64.make_inputs(B, N, H, 3, 1.5, 0.5, 2.0)
    assert torch.equal(qkv, qkv0) and torch.equal(dO, dO0)
    assert torch.equal(R.attention(qkv, B, N, H, scale, 64), R64.attention(qkv, B, N, H, scale))
    for dt in (torch.float64, torch.float32):
        assert torch.equal(R.grads(qkv, dO, B, N, H, scale, 64, dt), R64.grads(qkv, dO, B, N, H, scale, dt))
    for a, b in zip(R.closed_form(qkv, dO, B, N, H, scale, 64), R64.closed_form(qkv, dO, B, N, H, scale)):
        assert torch.equal(a, b)
    g64 = R.grads(qkv, dO, B, N, H, scale, 64, torch.float64)
    g32 = R.grads(qkv, dO, B, N, H, scale, 64, torch.float32)
    assert R.section_errs(g32, g64, H, 64) == R64.section_errs(g32, g64, H)
    assert R.cancel_scales(qkv, dO, B, N, H, scale, 64) == R64.cancel_scales(qkv, dO, B, N, H, scale)


@pytest.mark.parametrize("B,N,H", [(1, 1, 1), (1, 5, 2), (3, 33, 2)])
def test_closed_form_is_float64_autograd_at_width_80(B, N, H):
    qkv, dO, o64, o32, g64, g32 = R.case(B, N, H, 80)
    assert o64.shape == (B * N, H * 80) and g64.shape == (B * N, 3 * H * 80)
    d, dP, dS = R.closed_form(qkv, dO, B, N, H, 80 ** -0.5, 80)
    assert dP.shape == (B, H, N, N) and dS.shape == (B, H, N, N)
    den = float(g64.abs().max())
    if N == 1:   # dq = dk = 0 by cancellation; the value gradient is dO itself
        assert float(g64[:, :2 * H * 80].abs().max()) == 0.0
    assert float((d - g64).abs().max()) <= 1e-13 * den
    # the fp32 evaluation is an fp32-class answer to the same question
    assert R.rel_err(o32, o64) <= 64 * R.EPS32
    assert max(R.section_errs(g32, g64, H, 80, R.cancel_scales(qkv, dO, B, N, H, 80 ** -0.5, 80) + (None,)
                              if N == 1 else None)) <= 64 * R.EPS32
