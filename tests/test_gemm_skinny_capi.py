"""C-ABI of the skinny-M split-K GEMM (qvit_gemm_skinny, qvit_gemm_skinny_fits, qvit_gemm_skinny_workspace):
exported symbols, the shapes it takes, and argument validation by the header's status conventions. No kernel is
launched (runs without a GPU): every call here is rejected before a launch."""
import ctypes

import pytest

from quantized_vit_amd import _lib, build

ENULL, EALIGN, EINVAL = -3, -2, -1
W4, W8, W4R, W8R = 4, 8, 40, 80
EPI_QKV_SPLIT = 5


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_symbols_exported(lib):
    for name in ("qvit_gemm_skinny", "qvit_gemm_skinny_fits", "qvit_gemm_skinny_workspace"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name


@pytest.mark.parametrize("args, fits", [
    ((197, 768, W4R, 768, 768, _lib.EPI_F32_RESID), 1),
    ((197, 768, W8, 3072, 3072, _lib.EPI_I8_GELU), 1),
    ((1, 128, W4R, 40, 256, _lib.EPI_I32), 1),
    ((4096, 3072, W8, 1000, 1024, _lib.EPI_I8), 1),
    ((4096, 3072, W4R, 1000, 1024, _lib.EPI_F32), 1),
    ((197, 768, W4, 768, 768, _lib.EPI_F32), 0),       # the LDS-staged image: qvit_gemm
    ((197, 768, W8R, 768, 768, _lib.EPI_F32), 0),      # the int8 register image: qvit_gemm
    ((4097, 768, W4R, 768, 768, _lib.EPI_F32), 0),     # M above the limit
    ((0, 768, W4R, 768, 768, _lib.EPI_F32), 0),
    ((197, 704, W4R, 768, 768, _lib.EPI_F32), 0),      # K % 128
    ((197, 131072, W4R, 768, 768, _lib.EPI_F32), 0),   # the 16x-scaled accumulation bound
    ((197, 131072, W8, 768, 768, _lib.EPI_F32), 1),
    ((197, 768, W4R, 768, 704, _lib.EPI_F32), 0),      # npad < N, npad % 256
    ((197, 768, W4R, 768, 768, EPI_QKV_SPLIT), 0),
    ((4096, 768, W4R, 16640, 16640, _lib.EPI_F32), 0),  # 64 x 260 tiles > 16384 counters
])
def test_fits(lib, args, fits):
    assert lib.qvit_gemm_skinny_fits(*args) == fits
    assert _lib.gemm_skinny_fits(*args) == bool(fits)


def _call(lib, A=0x1000, M=197, K=768, lda=768, Wp=0x2000, wfmt=W4R, N=768, npad=768, d_act=0x3000, d_wt=0x3010,
          bias=0x4000, epi=_lib.EPI_F32, C=0x5000, ldc=768, splits=3, ws=0x10000, ws_bytes=None):
    p = lambda v: None if v is None else ctypes.c_void_p(v)   # never dereferenced: rejected before any launch
    if ws_bytes is None:
        n = ctypes.c_size_t(0)
        lib.qvit_gemm_skinny_workspace(M, K, npad, splits, ctypes.byref(n))
        ws_bytes = n.value
    return lib.qvit_gemm_skinny(p(A), M, K, lda, p(Wp), wfmt, N, npad, p(d_act), p(d_wt), p(bias), epi, p(C), ldc,
                                0, None, None, None, 0, None, splits, p(ws), ws_bytes, None)


@pytest.mark.parametrize("kw, status", [
    (dict(A=None), ENULL), (dict(Wp=None), ENULL), (dict(C=None), ENULL), (dict(d_act=None), ENULL),
    (dict(ws=None), ENULL),
    (dict(K=704, lda=704), EINVAL),                      # K % 128
    (dict(splits=7), EINVAL),                            # > K / 128
    (dict(K=3072, lda=3072, splits=17), EINVAL),         # > 16
    (dict(wfmt=W4), EINVAL), (dict(wfmt=W8R), EINVAL), (dict(wfmt=5), EINVAL),
    (dict(epi=EPI_QKV_SPLIT), EINVAL),
    (dict(M=4097), EINVAL),
    (dict(ws_bytes=65536 + 4 * 12 * 3 * 16384 - 1), EINVAL),   # one byte short of counters + 144 partials
    (dict(A=0x1008), EALIGN), (dict(lda=776), EALIGN), (dict(ws=0x10008), EALIGN),
    (dict(A=0x1008, wfmt=W4), EALIGN),                   # qvit_gemm's order first: alignment before the image rule
    (dict(A=None, K=704), ENULL),
])
def test_rejections(lib, kw, status):
    assert _call(lib, **kw) == status


def test_workspace_query(lib):
    n = ctypes.c_size_t(7)
    q = lambda *a: lib.qvit_gemm_skinny_workspace(*a, ctypes.byref(n))
    assert lib.qvit_gemm_skinny_workspace(197, 768, 768, 0, None) == ENULL
    assert q(197, 704, 768, 0) == EINVAL and q(4097, 768, 768, 0) == EINVAL and q(197, 768, 768, 7) == EINVAL
    assert q(197, 768, 768, 1) == 0 and n.value == 0                         # no split: no workspace
    assert q(197, 768, 768, 3) == 0 and n.value == 65536 + 4 * 12 * 3 * 16384
    assert _lib.gemm_skinny_workspace_bytes(65, 640, 1024, 2) == 65536 + 2 * 16 * 2 * 16384
