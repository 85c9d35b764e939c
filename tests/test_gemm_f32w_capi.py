"""C-ABI of the frozen-weight fp32 GEMM (qvit_pack_weight_b3_bytes, qvit_pack_weight_b3, qvit_gemm_f32w): header,
binding and exports agree, and rejected arguments return the header's status codes. No kernel is launched (runs
without a GPU): every call here is rejected before a launch."""
import ctypes
import os
import re

import pytest

from quantized_vit_amd import _lib, build

ENULL, EALIGN, EINVAL = -3, -2, -1
NAMES = ("qvit_pack_weight_b3_bytes", "qvit_pack_weight_b3", "qvit_gemm_f32w")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qvit_hip.h")
p = lambda v: None if v is None else ctypes.c_void_p(v)   # never dereferenced


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


_bytes = lambda N, K, planes: (N + 127) // 128 * ((K + 31) // 32) * planes * 8192


def _pack(lib, W=0x1000, N=40, K=48, ldw=48, planes=3, image=0x2000, image_bytes=None):
    nb = _bytes(N, K, planes) if image_bytes is None else image_bytes
    return lib.qvit_pack_weight_b3(p(W), N, K, ldw, planes, p(image), nb, None)


def _gemm(lib, A=0x1000, M=64, K=48, lda=48, Wimg=0x2000, planes=3, image_bytes=None, N=40, terms=6, bias=0x3000,
          epilogue=_lib.EPI_F32, C=0x4000, ldc=40):
    nb = _bytes(N, K, planes) if image_bytes is None else image_bytes
    return lib.qvit_gemm_f32w(p(A), M, K, lda, p(Wimg), planes, nb, N, terms, p(bias), epilogue, p(C), ldc, None)


def test_header_binding_and_exports_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    sigs = {**_lib._SIGNATURES, **_lib.INT64_FUNCS}
    for name in NAMES:
        proto = re.search(rf"\b{name}\s*\(([^)]*)\)", text).group(1)
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert len(proto.split(",")) == len(sigs[name]), name
    assert int(re.search(r"#define\s+QVIT_EPI_F32_GELU\s+(\d+)", open(HEADER).read()).group(1)) == _lib.EPI_F32_GELU
    assert "gemm_f32w.hip" in build.SOURCES and "gemm_f32_common.h" in build.HEADERS
    assert build.source_flags("gemm_f32w.hip") == build.source_flags("gemm_f32.hip")


@pytest.mark.parametrize("call, operands", [(_pack, ("W", "image")), (_gemm, ("A", "Wimg", "C"))])
def test_null_operands(lib, call, operands):
    for name in operands:
        assert call(lib, **{name: None}) == ENULL, name
    assert _gemm(lib, M=0) == 0 and _gemm(lib, M=0, bias=None) == 0    # nothing to do


def test_size_query(lib):
    q = lib.qvit_pack_weight_b3_bytes
    for N, K in [(1, 1), (128, 32), (129, 33), (1000, 768), (768, 3072)]:
        for planes in (2, 3):
            assert int(q(N, K, planes)) == _bytes(N, K, planes), (N, K, planes)
    for args in [(0, 8, 3), (8, 0, 3), (8, 8, 1), (8, 8, 4), ((1 << 24) + 1, 8, 3), (8, (1 << 30) + 1, 2)]:
        assert int(q(*args)) == EINVAL, args


def test_bad_sizes_planes_and_terms(lib):
    for kw in (dict(planes=1), dict(planes=4), dict(N=0), dict(K=0), dict(ldw=44), dict(image_bytes=_bytes(40, 48, 2))):
        assert _pack(lib, **kw) == EINVAL, kw
    for kw in (dict(planes=1), dict(planes=4), dict(terms=6, planes=2), dict(terms=3, planes=3), dict(terms=9),
               dict(terms=0), dict(epilogue=_lib.EPI_I8), dict(epilogue=_lib.EPI_I32), dict(epilogue=7),
               dict(M=-1), dict(N=0), dict(K=0), dict(lda=44), dict(ldc=36), dict(image_bytes=_bytes(40, 48, 3) - 1),
               dict(N=(1 << 24) + 1, ldc=(1 << 24) + 4)):
        assert _gemm(lib, **kw) == EINVAL, kw
    assert _gemm(lib, terms=3, planes=2, M=0) == 0 and _gemm(lib, epilogue=_lib.EPI_F32_GELU, M=0) == 0


def test_bad_alignment(lib):
    for kw in (dict(ldw=50), dict(W=0x1004), dict(image=0x2008)):
        assert _pack(lib, **kw) == EALIGN, kw
    for kw in (dict(lda=50), dict(ldc=42), dict(A=0x1004), dict(Wimg=0x2008), dict(C=0x4004), dict(bias=0x3002)):
        assert _gemm(lib, **kw) == EALIGN, kw
