"""C-ABI of the 16-bit activation path (qvit_quantize_act_i16, qvit_weight_code_sums, qvit_gemm_a16,
qvit_gemm_a16_fits): exported symbols, the documented limits and the documented order of the argument checks. No kernel
is launched (runs without a GPU): every call here is rejected before a launch, or has nothing to do."""
import ctypes

import pytest

from quantized_vit_amd import _lib, build, quant_layers

ENULL, EALIGN, EINVAL = -3, -2, -1
p = lambda v: None if v is None else ctypes.c_void_p(v)   # never dereferenced


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _gemm(lib, A=0x1000, M=70, K=384, lda=384, Wp=0x2000, wfmt=_lib.W16, N=300, npad=512, d_act=0x3000, d_wt=0x3100,
          bias=0x4000, wsum=0x5000, Y=0x6000, ldy=300):
    return lib.qvit_gemm_a16(p(A), M, K, lda, p(Wp), wfmt, N, npad, p(d_act), p(d_wt), p(bias), p(wsum), p(Y), ldy,
                             None)


def test_symbols_and_switch(lib):
    for name in ("qvit_quantize_act_i16", "qvit_weight_code_sums", "qvit_gemm_a16", "qvit_gemm_a16_fits"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "gemm_a16.hip" in build.SOURCES and build.source_flags("gemm_a16.hip") == build._NO_PACKED_FP32
    assert quant_layers.A16_GEMM is False   # off unless QVIT_A16_GEMM=1


def test_fits_limits(lib):
    fits = lambda M=70, K=384, wfmt=_lib.W16, N=300, npad=512: lib.qvit_gemm_a16_fits(M, K, wfmt, N, npad)
    assert all(fits(wfmt=f) == 1 for f in (_lib.W4, _lib.W8, _lib.W16, _lib.W24))
    assert fits(K=_lib.A16_MAX_K) == 1 and fits(M=0) == 1 and fits(M=1 << 24) == 1 and _lib.A16_MAX_K >= 16384
    for kw in (dict(K=_lib.A16_MAX_K + 128), dict(K=100), dict(K=0), dict(wfmt=_lib.W4R), dict(wfmt=5), dict(M=-1),
               dict(M=(1 << 24) + 1), dict(N=0), dict(N=513), dict(npad=500), dict(npad=(1 << 24) + 256, N=8)):
        assert fits(**kw) == 0, kw
        assert _gemm(lib, **kw) == EINVAL, kw
    assert _lib.gemm_a16_fits(70, 384, _lib.W16, 300, 512) is True


def test_gemm_check_order(lib):
    for name in ("A", "Wp", "Y", "d_act", "d_wt", "wsum"):
        assert _gemm(lib, **{name: None}, K=100, lda=8) == ENULL, name      # null before sizes and alignment
    for kw in (dict(lda=256), dict(ldy=296), dict(K=100, lda=100)):
        assert _gemm(lib, A=0x1004, **kw) == EINVAL, kw                     # sizes before alignment
    for kw in (dict(lda=392), dict(ldy=302), dict(A=0x1008), dict(Wp=0x2004), dict(Y=0x6004), dict(bias=0x4008),
               dict(wsum=0x5004)):
        assert _gemm(lib, **kw) == EALIGN, kw
    assert _gemm(lib, M=0) == 0 and _gemm(lib, M=0, bias=None) == 0         # nothing to do


def test_quantizer_and_sums_checks(lib):
    quant = lambda x=0x1000, qtype=0, planes=0x3000, ldc=128, kpad=128, rows=4: lib.qvit_quantize_act_i16(
        p(x), rows, 100, 100, qtype, p(0x2000), p(0x2100), None, 0, p(planes), ldc, kpad, None)
    sums = lambda Wp=0x1000, wfmt=_lib.W8, npad=256, K=128, out=0x2000: lib.qvit_weight_code_sums(
        p(Wp), wfmt, npad, K, p(out), None)
    assert quant(x=None, qtype=7) == ENULL and quant(planes=None) == ENULL
    for kw in (dict(qtype=7), dict(rows=-1), dict(kpad=96), dict(kpad=120, ldc=120), dict(ldc=112)):
        assert quant(planes=0x3004, **kw) == EINVAL, kw
    assert quant(ldc=136) == EALIGN and quant(planes=0x3008) == EALIGN and quant(rows=0) == 0
    assert sums(Wp=None, K=100) == ENULL and sums(out=None) == ENULL
    for kw in (dict(wfmt=3), dict(npad=100), dict(K=100), dict(K=_lib.A16_MAX_K + 128)):
        assert sums(out=0x2004, **kw) == EINVAL, kw
    assert sums(Wp=0x1008) == EALIGN and sums(out=0x2004) == EALIGN
