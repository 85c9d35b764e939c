"""C-ABI of the FP6 W4A4 path (qvit_quantize_act_f6, qvit_pack_weight_f6, qvit_gemm_f6, qvit_gemm_f6_fits): exported
symbols, the documented limits and the documented order of the argument rejections. No kernel is launched."""
import ctypes

import pytest

from quantized_vit_amd import _lib, build, quant_layers

ENULL, EALIGN, EINVAL = -3, -2, -1
p = lambda v: None if v is None else ctypes.c_void_p(v)   # never dereferenced


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _gemm(lib, A=0x1000, M=70, K=384, ldp=288, Wp=0x2000, N=200, npad=256, d_act=0x3000, d_wt=0x3100, bias=0x4000,
          epi=_lib.EPI_F32, C=0x6000, ldc=200):
    return lib.qvit_gemm_f6(p(A), M, K, ldp, p(Wp), N, npad, p(d_act), p(d_wt), p(bias), epi, p(C), ldc, 0, None, None,
                            None, 0, None, None)


def _quant(lib, x=0x1000, out=0x3000, ldp=96, kpad=128, rows=4, qtype=0):
    return lib.qvit_quantize_act_f6(p(x), rows, 100, 100, qtype, p(0x2000), p(0x2100), None, 0, p(out), ldp, kpad, None)


def test_symbols_and_switch(lib):
    for name in ("qvit_quantize_act_f6", "qvit_pack_weight_f6", "qvit_gemm_f6", "qvit_gemm_f6_fits"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "gemm_f6.hip" in build.SOURCES and build.source_flags("gemm_f6.hip") == build.source_flags("gemm_a4.hip")
    assert quant_layers.F6_GEMM is False   # off unless QVIT_F6_GEMM=1


@pytest.mark.parametrize("kw", [dict(K=100, ldp=96), dict(K=65536 + 128, ldp=49248), dict(npad=200), dict(N=257),
                                dict(M=-1)])
def test_gemm_rejects_sizes(lib, kw):
    assert lib.qvit_gemm_f6_fits(kw.get("M", 70), kw.get("K", 384), kw.get("N", 200), kw.get("npad", 256),
                                 _lib.EPI_F32) == 0
    assert _gemm(lib, A=0x1004, **kw) == EINVAL   # sizes before alignment


def test_gemm_fits_and_check_order(lib):
    assert all(lib.qvit_gemm_f6_fits(70, K, 200, 256, e) == 1 for K in (128, 65536)
               for e in range(_lib.EPI_F32, _lib.EPI_I32 + 1))
    assert lib.qvit_gemm_f6_fits(70, 384, 200, 256, 5) == 0 and _gemm(lib, epi=5) == EINVAL
    assert _lib.gemm_f6_fits(70, 384, 200, 256, _lib.EPI_I32) is True
    for name in ("A", "Wp", "C"):
        assert _gemm(lib, **{name: None}, K=100) == ENULL, name             # null before sizes and alignment
    assert _gemm(lib, d_act=None) == ENULL and _gemm(lib, d_wt=None) == ENULL
    assert _gemm(lib, M=0, d_act=None, d_wt=None, epi=_lib.EPI_I32) == 0    # EPI_I32 reads no scale
    assert _gemm(lib, ldp=272) == EINVAL                                    # ldp < 3 K / 4
    for kw in (dict(ldp=296), dict(A=0x1008), dict(Wp=0x2004), dict(C=0x6004), dict(ldc=202), dict(bias=0x4008)):
        assert _gemm(lib, **kw) == EALIGN, kw
    assert _gemm(lib, M=0) == 0 and _gemm(lib, M=0, bias=None) == 0         # nothing to do


def test_quantizer_checks(lib):
    assert _quant(lib, x=None, qtype=7) == ENULL and _quant(lib, out=None) == ENULL
    for kw in (dict(qtype=7), dict(rows=-1), dict(kpad=192, ldp=144), dict(kpad=64), dict(ldp=80),
               dict(kpad=256, ldp=176)):
        assert _quant(lib, out=0x3004, **kw) == EINVAL, kw
    assert _quant(lib, ldp=104) == EALIGN and _quant(lib, out=0x3008) == EALIGN and _quant(lib, rows=0) == 0
