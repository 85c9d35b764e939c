"""qvit_gemm_skinny (64 x 64 tiles, split-K reduced inside the launch) against three oracles, none of them the code
under test: the int64 product from numpy (EPI_I32, exact), the float64 value d_act d_wt acc + bias (EPI_F32, within
the fp32 roundings of the epilogue), and the bytes of qvit_gemm on the same inputs (all five epilogues).

Shapes: M below, at and above one 64-row tile and at one image's 197 tokens; N short of one 64-column tile and
ragged at 1000 (npad 256 / 1024: the unused quarters of a 256-row weight tile, and tile_n > 0); K of one k-tile
(no split), three (one per slice), five split 3 + 2 (a ragged split) and 24 on the automatic split."""
import functools

import numpy as np
import pytest
import torch

from quantized_vit_amd import _lib
from quantized_vit_amd.quant_layers import epilogue_table_geometry, saturation_level
from test_gpu_kernels import _p, _round_up, act_buffer, pack_codes

pytestmark = pytest.mark.gpu

D_ACT, D_WT = 0.0031, 0.0017
MMAX = 197


@functools.lru_cache(maxsize=None)
def _problem(N, K, wfmt, extreme=False):
    """Codes over the full range (or all at the extreme), the bias and the exact int64 product, once per shape:
    the cases at smaller M take the first M rows."""
    g = np.random.default_rng(N * 5 + K * 7 + wfmt)
    lo = -8 if wfmt == _lib.W4R else -127
    a = np.full((MMAX, K), 127) if extreme else g.integers(-127, 128, (MMAX, K))
    w = np.full((N, K), -8) if extreme else g.integers(lo, -lo + (wfmt == _lib.W8), (N, K))
    bias = (g.standard_normal(N) * 0.3).astype(np.float32)
    return a, w, bias, a.astype(np.int64) @ w.astype(np.int64).T


def _device_problem(dev, M, N, K, wfmt, extreme=False):
    a, w, bias, acc = _problem(N, K, wfmt, extreme)
    packed, npad, kpad = pack_codes(torch.from_numpy(w), _lib.W4 if wfmt == _lib.W4R else _lib.W8, dev)
    wimg = _lib.pack_weight_w4r(packed, npad, kpad) if wfmt == _lib.W4R else packed
    A = act_buffer(torch.from_numpy(a[:M]), kpad, dev)
    bias_pad = _lib.pad_bias(torch.from_numpy(bias).to(dev), N, npad, dev)
    return A, wimg, npad, kpad, bias_pad, bias, acc[:M]


def _out(dev, M, N, epi, base):
    if epi == _lib.EPI_I32:
        return torch.full((M, _round_up(N, 4)), -7, dtype=torch.int32, device=dev)
    if epi in (_lib.EPI_I8, _lib.EPI_I8_GELU):
        return torch.full((M, _round_up(N, 16)), 99, dtype=torch.int8, device=dev)
    return base.clone()


def _check_all(dev, M, N, K, wfmt, splits, extreme=False):
    A, wimg, npad, kpad, bias_pad, bias, acc = _device_problem(dev, M, N, K, wfmt, extreme)
    base = torch.randn(M, _round_up(N, 4), generator=torch.Generator().manual_seed(M + N)).to(dev)
    qt, dn, qmn, t = _lib.QT_NONLINEAR, 1.2 / 127, 1.2, 1.0
    q = dict(out_qtype=qt, out_d=_p(dn, dev), out_qm=_p(qmn, dev), out_t=_p(t, dev))
    geo = epilogue_table_geometry(qt, dn, qmn, t, saturation_level(qt, dn, qmn, t), True)
    # the code table on the GELU epilogue, the per-element quantizer on the plain one
    table = _lib.epi_table_build(_lib.EPI_I8_GELU, qt, q["out_d"], q["out_qm"], q["out_t"], 0, *geo, dev)
    for epi in (_lib.EPI_I32, _lib.EPI_F32, _lib.EPI_F32_RESID, _lib.EPI_I8, _lib.EPI_I8_GELU):
        kw = dict(q, epi_table=table if epi == _lib.EPI_I8_GELU else None) if epi in (_lib.EPI_I8, _lib.EPI_I8_GELU) else {}
        args = (A, M, kpad, wimg, wfmt, N, npad, _p(D_ACT, dev), _p(D_WT, dev), bias_pad, epi)
        want = _lib.gemm(*args, _out(dev, M, N, epi, base), **kw)
        got = _lib.gemm_skinny(*args, _out(dev, M, N, epi, base), splits=splits, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"epilogue {epi}: differs from qvit_gemm"
        if epi == _lib.EPI_I32:
            assert np.array_equal(got[:, :N].cpu().numpy().astype(np.int64), acc)
            assert bool((got[:, N:] == -7).all())
        if epi == _lib.EPI_F32:
            # two roundings in alpha, one in (float)acc, one in the fma, and the store
            prod = float(np.float32(D_ACT)) * float(np.float32(D_WT)) * acc.astype(np.float64)
            ref = prod + bias.astype(np.float64)
            err = np.abs(got[:, :N].cpu().numpy().astype(np.float64) - ref)
            bound = 2.0 ** -21 * (np.abs(prod) + np.abs(bias.astype(np.float64)))
            print(f"EPI_F32 max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert bool((err <= bound).all())


@pytest.mark.parametrize("wfmt", [_lib.W4R, _lib.W8])
@pytest.mark.parametrize("K,splits", [(128, 1), (384, 3), (640, 2), (3072, 0)])
@pytest.mark.parametrize("N", [40, 1000])
@pytest.mark.parametrize("M", [1, 63, 65, 197])
def test_skinny_matches_oracles(dev, M, N, K, splits, wfmt):
    _check_all(dev, M, N, K, wfmt, splits)


@pytest.mark.parametrize("wfmt", [_lib.W4R, _lib.W8])
def test_skinny_all_extreme_codes(dev, wfmt):
    _check_all(dev, 65, 40, 3072, wfmt, 0, extreme=True)


def test_workspace_reused_across_calls(dev):
    """Two calls on one workspace, different inputs, forced split: a counter that is not reset or a stale partial
    of the first call shows in the second result."""
    M, N, K = 65, 1000, 640
    ws = torch.zeros(_lib.gemm_skinny_workspace_bytes(M, K, 1024, 3), dtype=torch.uint8, device=dev)
    for wfmt in (_lib.W8, _lib.W4R):   # (two shapes' worth of different inputs; the second call is the one checked)
        A, wimg, npad, kpad, _, _, acc = _device_problem(dev, M, N, K, wfmt)
        C = torch.full((M, N), -7, dtype=torch.int32, device=dev)
        _lib.gemm_skinny(A, M, kpad, wimg, wfmt, N, npad, None, None, None, _lib.EPI_I32, C, splits=3, workspace=ws)
        torch.cuda.synchronize()
    assert np.array_equal(C.cpu().numpy().astype(np.int64), acc)
    assert int(ws[:65536].view(torch.int32).abs().sum()) == 0   # the arrival counters are left zero
