"""C-ABI of the weight-gradient GEMM (qvit_gemm_wgrad, qvit_gemm_wgrad_workspace_bytes): exported symbols,
argument validation by the header's status conventions and the workspace bound. No kernel is launched (runs
without a GPU): every call here is rejected before a launch."""
import ctypes

import pytest

from quantized_vit_amd import _lib, build

ENULL, EALIGN, EINVAL = -3, -2, -1


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _r128(v):
    return (v + 127) // 128 * 128


def test_symbols_exported(lib):
    for name in ("qvit_gemm_wgrad", "qvit_gemm_wgrad_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name


def _call(lib, G=0x1000, M=64, N=48, ldg=48, A=0x2000, K=64, lda=64, d=0x3000, dW=0x4000, ldw=64, ws=0x5000,
          ws_bytes=None):
    p = lambda v: None if v is None else ctypes.c_void_p(v)   # never dereferenced: rejected before any launch
    if ws_bytes is None:
        ws_bytes = max(0, int(lib.qvit_gemm_wgrad_workspace_bytes(M, N, K)))
    return lib.qvit_gemm_wgrad(p(G), M, N, ldg, p(A), K, lda, p(d), p(dW), ldw, p(ws), ws_bytes, None)


def test_null_operands(lib):
    for name in ("G", "A", "d", "dW", "ws"):
        assert _call(lib, **{name: None}) == ENULL, name


def test_bad_sizes(lib):
    assert _call(lib, M=-1, ws_bytes=1 << 20) == EINVAL
    assert _call(lib, N=0, ws_bytes=1 << 20) == EINVAL
    assert _call(lib, K=0, ws_bytes=1 << 20) == EINVAL
    assert _call(lib, N=-5, ws_bytes=1 << 20) == EINVAL
    assert _call(lib, ldg=44) == EINVAL          # ldg < N
    assert _call(lib, lda=48) == EINVAL          # lda < K
    assert _call(lib, ldw=60) == EINVAL          # ldw < K
    assert _call(lib, ws_bytes=16) == EINVAL     # workspace shorter than the query asks for
    assert _call(lib, N=(1 << 24) + 1, ldg=(1 << 24) + 4, ws_bytes=1 << 20) == EINVAL


def test_bad_alignment(lib):
    assert _call(lib, ldg=50) == EALIGN          # ldg % 4
    assert _call(lib, lda=72) == EALIGN          # lda % 16
    assert _call(lib, G=0x1008) == EALIGN
    assert _call(lib, A=0x2004) == EALIGN
    assert _call(lib, ws=0x5008) == EALIGN
    assert _call(lib, dW=0x4002) == EALIGN
    assert _call(lib, dW=0x4004, ldw=67, ws_bytes=0) == EINVAL   # dW needs 4-byte alignment only: size check next


def test_workspace_query(lib):
    q = lib.qvit_gemm_wgrad_workspace_bytes
    assert q(-1, 8, 8) == EINVAL and q(8, 0, 8) == EINVAL and q(8, 8, 0) == EINVAL
    assert q(8, (1 << 24) + 1, 8) == EINVAL
    shapes = [(1, 1), (48, 64), (10, 100), (257, 130), (1000, 768), (768, 768), (2304, 768), (3072, 768), (768, 3072)]
    for N, K in shapes:
        tile_bytes = _r128(N) * _r128(K) * 4
        tiles = (_r128(N) // 128) * (_r128(K) // 128)
        prev = 0
        for M in (0, 1, 31, 32, 33, 64, 65, 129, 513, 1000, 4096, 50432, 1 << 20):
            b = int(q(M, N, K))
            assert b >= tile_bytes and b % tile_bytes == 0, (M, N, K)
            s = b // tile_bytes
            assert s == max(1, min(16, (M + 31) // 32, (512 + tiles - 1) // tiles)), (M, N, K, s)
            assert b >= prev, (M, N, K)                       # non-decreasing in M
            assert b <= 16 * tile_bytes and b <= (tiles + 511) * 65536, (M, N, K)
            assert _lib.gemm_wgrad_splits(M, N, K) == s
            prev = b
    # Mlp.fc1 of ViT-B at b256: a small multiple of the weight
    assert int(q(50432, 3072, 768)) == 4 * 3072 * 768 * 4
