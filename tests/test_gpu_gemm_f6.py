"""qvit_quantize_act_f6, qvit_pack_weight_f6 and qvit_gemm_f6 (W4A4 on the FP6 matrix instruction). The quantizer
against the bytes of qvit_quantize_act_i8 packed on the host from the format's definition; the GEMM against the bytes of
qvit_gemm on the same codes (all five epilogues) and against an int64 matmul on the CPU, up to the accumulator's worst
case, which is the proof that the fp32 accumulator adds these integers exactly."""
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
E2M3 = torch.tensor([0x00, 0x08, 0x10, 0x14, 0x18, 0x1A, 0x1C, 0x1E])


def pack_f6(codes: torch.Tensor) -> torch.Tensor:
    """[M, kpad] codes in [-7, 7] -> QVIT_ACT_F6 bytes [M, 3 kpad / 4], written from the format's definition: column j
    of a 32-column group at bits [6 j, 6 j + 6) of its 24 bytes; per k-tile the four 16-byte heads, then the tails."""
    c = codes.cpu().to(torch.int64)
    f = E2M3[c.abs()] | ((c < 0).to(torch.int64) << 5)
    w = (f.reshape(c.shape[0], -1, 4) << torch.tensor([0, 6, 12, 18])).sum(-1)           # 4 fields = 3 bytes
    by = ((w.unsqueeze(-1) >> torch.tensor([0, 8, 16])) & 255).reshape(c.shape[0], -1, 4, 24)   # [row, k-tile, q, 24]
    out = torch.cat((by[..., :16].flatten(2), by[..., 16:].flatten(2)), dim=2)
    return out.to(torch.uint8).reshape(c.shape[0], -1).to(codes.device)


@pytest.mark.parametrize("pad", [0, 4, 3])            # ldx == cols; ldx > cols on the 16-byte loads; on the scalar loads
@pytest.mark.parametrize("cols", [128, 200, 768])     # kpad 128, 256 (padding fields), 768
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
    buf = torch.full((rows, kpad // 4 * 3 + 16), 0x5A, dtype=torch.uint8, device=dev)
    _lib.quantize_act_f6(x, *q, buf, kpad)
    assert int(want.abs().max()) == 7 and want[-1, :7].tolist() == [0, 7, -7, 0, 0, 0, 0]
    assert torch.equal(buf[:, :kpad // 4 * 3], pack_f6(want))
    got = _lib.unpack_act_f6(buf, kpad)
    assert torch.equal(got, want) and bool((got[:, cols:] == 0).all())
    assert bool((buf[:, kpad // 4 * 3:] == 0x5A).all())   # bytes past the row's length are never touched


@functools.lru_cache(maxsize=None)
def _problem(N, K):
    """Codes of both operands over [-7, 7], the bias and the exact int64 product, once per shape: the cases at smaller
    M take the first M rows."""
    g = np.random.default_rng(N * 5 + K * 7)
    a, w = g.integers(-7, 8, (MMAX, K)), g.integers(-7, 8, (N, K))
    return a, w, (g.standard_normal(N) * 0.3).astype(np.float32), a.astype(np.int64) @ w.astype(np.int64).T


def _out(dev, M, N, epi, base):
    if epi == _lib.EPI_I32:
        return torch.full((M, _round_up(N, 4)), -7, dtype=torch.int32, device=dev)
    if epi in (_lib.EPI_I8, _lib.EPI_I8_GELU):
        return torch.full((M, _round_up(N, 16)), 99, dtype=torch.int8, device=dev)
    return base.clone()


@pytest.mark.parametrize("K", [128, 384, 1024])       # one k-tile (shorter than the ring), odd and even counts
@pytest.mark.parametrize("N", [200, 768])             # npad 256 (ragged) / 768 (three weight tiles)
@pytest.mark.parametrize("M", [1, 129, 300])
def test_gemm_matches_qvit_gemm(dev, M, N, K):
    a, w, bias, acc = _problem(N, K)
    packed, npad, kpad = pack_codes(torch.from_numpy(w), _lib.W4, dev)
    w4r, w6f = _lib.pack_weight_w4r(packed, npad, kpad), _lib.pack_weight_f6(packed, npad, kpad)
    A8 = act_buffer(torch.from_numpy(a[:M]), kpad, dev)
    A6 = pack_f6(A8)
    bias_pad = _lib.pad_bias(torch.from_numpy(bias).to(dev), N, npad, dev)
    base = torch.randn(M, _round_up(N, 4), generator=torch.Generator().manual_seed(M + N)).to(dev)
    qt, dn, qmn, t = _lib.QT_NONLINEAR, 1.2 / 127, 1.2, 1.0
    q = dict(out_qtype=qt, out_d=_p(dn, dev), out_qm=_p(qmn, dev), out_t=_p(t, dev))
    geo = epilogue_table_geometry(qt, dn, qmn, t, saturation_level(qt, dn, qmn, t), True)
    # the code table on the GELU epilogue, the per-element quantizer on the plain one
    table = _lib.epi_table_build(_lib.EPI_I8_GELU, qt, q["out_d"], q["out_qm"], q["out_t"], 0, *geo, dev)
    for epi in (_lib.EPI_I32, _lib.EPI_F32, _lib.EPI_F32_RESID, _lib.EPI_I8, _lib.EPI_I8_GELU):
        kw = dict(q, epi_table=table if epi == _lib.EPI_I8_GELU else None) if epi in (_lib.EPI_I8, _lib.EPI_I8_GELU) else {}
        tail = (N, npad, _p(D_ACT, dev), _p(D_WT, dev), bias_pad, epi)
        want = _lib.gemm(A8, M, kpad, w4r, _lib.W4R, *tail, _out(dev, M, N, epi, base), **kw)
        got = _lib.gemm_f6(A6, M, kpad, w6f, *tail, _out(dev, M, N, epi, base), **kw)
        again = _lib.gemm_f6(A6, M, kpad, w6f, *tail, _out(dev, M, N, epi, base), **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"epilogue {epi}: differs from qvit_gemm"
        assert torch.equal(got, again), f"epilogue {epi}: two calls differ"
        if epi == _lib.EPI_I32:
            assert np.array_equal(got[:, :N].cpu().numpy().astype(np.int64), acc[:M])
            assert bool((got[:, N:] == -7).all())


def test_accumulator_worst_case_against_int64(dev):
    """K = 65536, every code +-7; row 0 x column 0 is all (-7)(-7): 65536 * 49 = 3211264 < 2^24, the largest sum an
    fp32 accumulator has to hold exactly."""
    M, N, K = 16, 256, 65536
    g = np.random.default_rng(6)
    a, w = g.choice([-7, 7], (M, K)), g.choice([-7, 7], (N, K))
    a[0], w[0] = -7, -7
    packed, npad, kpad = pack_codes(torch.from_numpy(w), _lib.W4, dev)
    C = torch.zeros((M, N), dtype=torch.int32, device=dev)
    _lib.gemm_f6(pack_f6(torch.from_numpy(a).to(dev)), M, kpad, _lib.pack_weight_f6(packed, npad, kpad), N, npad, None,
                 None, None, _lib.EPI_I32, C)
    want = a.astype(np.int64) @ w.astype(np.int64).T
    assert want[0, 0] == 3211264
    assert np.array_equal(C.cpu().numpy().astype(np.int64), want)


def test_pack_rejects_minus_eight(dev):
    w = torch.zeros(256, 128, dtype=torch.int64)
    w[77, 45] = -8
    packed, npad, kpad = pack_codes(w, _lib.W4, dev)
    with pytest.raises(_lib.QvitError, match="-8"):
        _lib.pack_weight_f6(packed, npad, kpad)
