"""qvit_quantize_act_i4 and qvit_gemm_a4 (packed 4-bit activation codes, QVIT_ACT_P4). The quantizer against the bytes
of qvit_quantize_act_i8, unpacked on the host with plain torch ops; the GEMM against the bytes of qvit_gemm on the same
codes (all five epilogues) and, at the accumulator's worst case, against an int64 matmul on the CPU."""
import functools

import numpy as np
import pytest
import torch

from quantized_vit_amd import _lib
from quantized_vit_amd.quant_layers import epilogue_table_geometry, saturation_level
from test_gpu_kernels import _p, _round_up, act_buffer, pack_codes

pytestmark = pytest.mark.gpu

D_ACT, D_WT = 0.0031, 0.0017
MMAX = 300


def pack_p4(codes: torch.Tensor) -> torch.Tensor:
    """[M, kpad] codes in [-7, 7] -> QVIT_ACT_P4 bytes [M, kpad / 2], written from the format's definition."""
    t = codes.to(torch.int16).reshape(codes.shape[0], -1, 2, 64) & 15      # [row, k-tile, half, byte]
    return (t[:, :, 0] | (t[:, :, 1] << 4)).to(torch.uint8).reshape(codes.shape[0], -1)


@pytest.mark.parametrize("pad", [0, 4, 3])            # ldx == cols; ldx > cols on the 16-byte loads; on the scalar loads
@pytest.mark.parametrize("cols", [128, 200, 768])     # kpad 128, 256 (padding nibbles), 768
@pytest.mark.parametrize("rows", [1, 67])
@pytest.mark.parametrize("qtype,t", [(_lib.QT_LINEAR, 1.0), (_lib.QT_NONLINEAR, 0.9)])
def test_quantizer_matches_int8_codes(dev, qtype, t, rows, cols, pad):
    qm = 1.5
    d = qm ** t / 7                                   # saturation code 7
    x = torch.randn(rows, cols + pad, generator=torch.Generator().manual_seed(rows + cols)) * qm   # a third saturates
    x[-1, :7] = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1e-38, -1e-38])
    x = x.to(dev)[:, :cols]
    kpad = _round_up(cols, 128)
    q = (qtype, _p(d, dev), _p(qm, dev), _p(t, dev), 0)
    want = _lib.quantize_act_i8(x, *q, torch.full((rows, kpad), 99, dtype=torch.int8, device=dev), kpad)
    buf = torch.full((rows, kpad // 2 + 16), 0x5A, dtype=torch.uint8, device=dev)
    _lib.quantize_act_i4(x, *q, buf, kpad)
    got = _lib.unpack_act_p4(buf, kpad)
    assert int(want.abs().max()) == 7 and want[-1, :7].tolist() == [0, 7, -7, 0, 0, 0, 0]
    assert torch.equal(got, want) and bool((got[:, cols:] == 0).all())
    assert bool((buf[:, kpad // 2:] == 0x5A).all())   # bytes past kpad / 2 are never touched
    assert torch.equal(pack_p4(want), buf[:, :kpad // 2])


@functools.lru_cache(maxsize=None)
def _problem(N, K, wfmt):
    """Activation codes over [-7, 7], weight codes over the format's range, the bias and the exact int64 product,
    once per shape: the cases at smaller M take the first M rows."""
    g = np.random.default_rng(N * 5 + K * 7 + wfmt)
    a = g.integers(-7, 8, (MMAX, K))
    w = g.integers(-8, 8, (N, K)) if wfmt == _lib.W4R else g.integers(-127, 128, (N, K))
    bias = (g.standard_normal(N) * 0.3).astype(np.float32)
    return a, w, bias, a.astype(np.int64) @ w.astype(np.int64).T


def _device_weights(w, wfmt, dev):
    packed, npad, kpad = pack_codes(torch.from_numpy(w), _lib.W4 if wfmt == _lib.W4R else _lib.W8, dev)
    return (_lib.pack_weight_w4r(packed, npad, kpad) if wfmt == _lib.W4R else packed), npad, kpad


def _out(dev, M, N, epi, base):
    if epi == _lib.EPI_I32:
        return torch.full((M, _round_up(N, 4)), -7, dtype=torch.int32, device=dev)
    if epi in (_lib.EPI_I8, _lib.EPI_I8_GELU):
        return torch.full((M, _round_up(N, 16)), 99, dtype=torch.int8, device=dev)
    return base.clone()


@pytest.mark.parametrize("wfmt", [_lib.W4R, _lib.W8])
@pytest.mark.parametrize("K", [128, 384, 1024])       # one k-tile (shorter than the ring), odd and even counts
@pytest.mark.parametrize("N", [200, 768])             # npad 256 (ragged) / 768 (three weight tiles)
@pytest.mark.parametrize("M", [1, 129, 300])
def test_gemm_matches_qvit_gemm(dev, M, N, K, wfmt):
    a, w, bias, acc = _problem(N, K, wfmt)
    wimg, npad, kpad = _device_weights(w, wfmt, dev)
    A8 = act_buffer(torch.from_numpy(a[:M]), kpad, dev)
    A4 = pack_p4(A8)
    bias_pad = _lib.pad_bias(torch.from_numpy(bias).to(dev), N, npad, dev)
    base = torch.randn(M, _round_up(N, 4), generator=torch.Generator().manual_seed(M + N)).to(dev)
    qt, dn, qmn, t = _lib.QT_NONLINEAR, 1.2 / 127, 1.2, 1.0
    q = dict(out_qtype=qt, out_d=_p(dn, dev), out_qm=_p(qmn, dev), out_t=_p(t, dev))
    geo = epilogue_table_geometry(qt, dn, qmn, t, saturation_level(qt, dn, qmn, t), True)
    # the code table on the GELU epilogue, the per-element quantizer on the plain one
    table = _lib.epi_table_build(_lib.EPI_I8_GELU, qt, q["out_d"], q["out_qm"], q["out_t"], 0, *geo, dev)
    for epi in (_lib.EPI_I32, _lib.EPI_F32, _lib.EPI_F32_RESID, _lib.EPI_I8, _lib.EPI_I8_GELU):
        kw = dict(q, epi_table=table if epi == _lib.EPI_I8_GELU else None) if epi in (_lib.EPI_I8, _lib.EPI_I8_GELU) else {}
        tail = (kpad, wimg, wfmt, N, npad, _p(D_ACT, dev), _p(D_WT, dev), bias_pad, epi)
        want = _lib.gemm(A8, M, *tail, _out(dev, M, N, epi, base), **kw)
        got = _lib.gemm_a4(A4, M, *tail, _out(dev, M, N, epi, base), **kw)
        again = _lib.gemm_a4(A4, M, *tail, _out(dev, M, N, epi, base), **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"epilogue {epi}: differs from qvit_gemm"
        assert torch.equal(got, again), f"epilogue {epi}: two calls differ"
        if epi == _lib.EPI_I32:
            assert np.array_equal(got[:, :N].cpu().numpy().astype(np.int64), acc[:M])
            assert bool((got[:, N:] == -7).all())


@pytest.mark.parametrize("wfmt", [_lib.W4R, _lib.W8])
def test_accumulator_worst_case_against_int64(dev, wfmt):
    """K = 65536, every activation +-7, every weight -8 or 7; row 0 x column 0 is all (-7)(-8): 65536 * 56 = 3670016,
    256 times that in the QVIT_W4R accumulator (9.4e8 < 2^31)."""
    M, N, K = 16, 256, 65536
    g = np.random.default_rng(wfmt)
    a = g.choice([-7, 7], (M, K))
    w = g.choice([-8, 7], (N, K))
    a[0], w[0] = -7, -8
    wimg, npad, kpad = _device_weights(w, wfmt, dev)
    A4 = pack_p4(torch.from_numpy(a).to(dev))
    C = torch.zeros((M, N), dtype=torch.int32, device=dev)
    _lib.gemm_a4(A4, M, kpad, wimg, wfmt, N, npad, None, None, None, _lib.EPI_I32, C)
    want = a.astype(np.int64) @ w.astype(np.int64).T
    assert want[0, 0] == 3670016
    assert np.array_equal(C.cpu().numpy().astype(np.int64), want)
