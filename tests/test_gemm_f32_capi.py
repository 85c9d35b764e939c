"""C-ABI of the fp32 x fp32 GEMM (qvit_gemm_f32_nt, qvit_gemm_f32_tn, qvit_gemm_f32_tn_workspace_bytes): exported
symbols, argument validation by the header's status conventions and the workspace formula. No kernel is launched
(runs without a GPU): every call here is rejected before a launch."""
import ctypes

import pytest

from quantized_vit_amd import _lib, build

ENULL, EALIGN, EINVAL = -3, -2, -1
p = lambda v: None if v is None else ctypes.c_void_p(v)   # never dereferenced


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _nt(lib, A=0x1000, M=64, K=48, lda=48, B=0x2000, N=40, ldb=48, bias=0x3000, C=0x4000, ldc=40):
    return lib.qvit_gemm_f32_nt(p(A), M, K, lda, p(B), N, ldb, p(bias), p(C), ldc, None)


def _tn(lib, A=0x1000, M=64, I=48, lda=48, B=0x2000, J=40, ldb=40, C=0x4000, ldc=40, ws=0x5000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(0, int(lib.qvit_gemm_f32_tn_workspace_bytes(M, I, J)))
    return lib.qvit_gemm_f32_tn(p(A), M, I, lda, p(B), J, ldb, p(C), ldc, p(ws), ws_bytes, None)


def test_symbols_exported(lib):
    for name in ("qvit_gemm_f32_nt", "qvit_gemm_f32_tn", "qvit_gemm_f32_tn_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name


@pytest.mark.parametrize("call, operands", [(_nt, ("A", "B", "C")), (_tn, ("A", "B", "C", "ws"))])
def test_null_operands(lib, call, operands):
    for name in operands:
        assert call(lib, **{name: None}) == ENULL, name


def test_bad_sizes(lib):
    for kw in (dict(M=-1), dict(K=0), dict(N=0), dict(N=-5), dict(lda=44), dict(ldb=44), dict(ldc=36),
               dict(N=(1 << 24) + 1, ldc=(1 << 24) + 4)):
        assert _nt(lib, **kw) == EINVAL, kw
    for kw in (dict(M=-1), dict(I=0), dict(J=0), dict(lda=44), dict(ldb=36), dict(ldc=36),
               dict(I=(1 << 24) + 1, lda=(1 << 24) + 4)):
        assert _tn(lib, ws_bytes=1 << 20, **kw) == EINVAL, kw
    need = int(lib.qvit_gemm_f32_tn_workspace_bytes(64, 48, 40))
    assert _tn(lib, ws_bytes=need - 1) == EINVAL      # one byte short
    assert _nt(lib, M=0) == 0                          # NT: nothing to do


def test_bad_alignment(lib):
    for kw in (dict(lda=50), dict(ldb=50), dict(ldc=42), dict(A=0x1004), dict(B=0x2008), dict(C=0x4004),
               dict(bias=0x3002)):
        assert _nt(lib, **kw) == EALIGN, kw
    for kw in (dict(lda=50), dict(ldb=42), dict(A=0x1004), dict(B=0x2008), dict(ws=0x5008), dict(C=0x4002)):
        assert _tn(lib, **kw) == EALIGN, kw


def test_workspace_query(lib):
    q = lib.qvit_gemm_f32_tn_workspace_bytes
    assert q(-1, 8, 8) == EINVAL and q(8, 0, 8) == EINVAL and q(8, 8, 0) == EINVAL and q(8, (1 << 24) + 1, 8) == EINVAL
    r128 = lambda v: (v + 127) // 128 * 128
    for I, J in [(1, 1), (48, 64), (10, 100), (257, 130), (1000, 768), (2304, 768), (768, 3072)]:
        tiles = (r128(I) // 128) * (r128(J) // 128)
        for M in (0, 1, 31, 32, 33, 65, 513, 1000, 50432, 1 << 20):
            s = max(1, min(16, (M + 31) // 32, (512 + tiles - 1) // tiles))
            assert int(q(M, I, J)) == s * r128(I) * r128(J) * 4, (M, I, J)
            assert _lib.gemm_f32_tn_splits(M, I, J) == s
