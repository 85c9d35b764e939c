"""C-ABI of the train-fusion kernels (train_fuse.hip): exported symbols with the declared signatures, the workspace
queries and argument validation by the header's status conventions. No kernel is launched (runs without a GPU):
every call here is rejected before a launch."""
import ctypes

import pytest

from quantized_vit_amd import _lib, build

ENULL, EALIGN, EINVAL = -3, -2, -1
NEW = ("qvit_layernorm_quant_backward", "qvit_gelu_quant_i8", "qvit_gelu_quant_backward")
NEW_I64 = ("qvit_layernorm_quant_backward_workspace_bytes", "qvit_gelu_quant_backward_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_symbols_exported(lib):
    for name in NEW + NEW_I64:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert len(_lib._SIGNATURES["qvit_layernorm_quant_backward"]) == 23
    assert len(_lib._SIGNATURES["qvit_gelu_quant_i8"]) == len(_lib._SIGNATURES["qvit_quantize_act_i8"])
    assert len(_lib._SIGNATURES["qvit_gelu_quant_backward"]) == len(_lib._SIGNATURES["qvit_quant_backward"]) - 1
    for name in NEW_I64:
        assert getattr(lib, name).restype is ctypes.c_int64


def test_declared_in_the_header():
    import os
    with open(os.path.join(os.path.dirname(build.HERE), "include", "qvit_hip.h")) as f:
        text = f.read()
    for name in NEW:
        assert f"int {name}(" in text
    for name in NEW_I64:
        assert f"int64_t {name}(" in text


def test_workspace_queries(lib):
    ln, ge = lib.qvit_layernorm_quant_backward_workspace_bytes, lib.qvit_gelu_quant_backward_workspace_bytes
    assert ln(-1, 8) == EINVAL and ln(8, -1) == EINVAL and ge(-1) == EINVAL
    # one scalar partial (3 doubles) and two column rows per workgroup of 4 rows, at most 1024 workgroups
    for rows, cols in ((0, 8), (1, 4), (5, 64), (4096, 768), (50432, 768), (1 << 20, 2048)):
        grid = max(1, min(1024, (rows + 3) // 4))
        assert ln(rows, cols) == (grid * 24 + 15) // 16 * 16 + grid * 2 * cols * 4, (rows, cols)
    for n in (0, 1, 4099, 1 << 24):
        assert ge(n) == max(1, min(1024, (n // 4 + 255) // 256)) * 24


def _ln(lib, x=0x1000, rows=8, cols=64, ldx=64, gamma=0x2000, beta=0x3000, d=0x4000, qm=0x4010, t=None, qtype=0,
        gy=0x5000, ldg=64, gx=0x6000, ldo=64, gg=0x7000, gb=0x8000, sc=0x9000, ws=0xA000, ws_bytes=None):
    p = lambda v: None if v is None else ctypes.c_void_p(v)   # never dereferenced: rejected before any launch
    if ws_bytes is None:
        ws_bytes = max(0, int(lib.qvit_layernorm_quant_backward_workspace_bytes(rows, cols)))
    return lib.qvit_layernorm_quant_backward(p(x), rows, cols, ldx, p(gamma), p(beta), 1e-6, qtype, p(d), p(qm), p(t),
                                             -2.0, 2.0, p(gy), ldg, p(gx), ldo, p(gg), p(gb), p(sc), p(ws), ws_bytes,
                                             None)


def test_layernorm_backward_rejections(lib):
    for name in ("x", "gamma", "beta", "d", "qm", "gy", "gx", "sc", "ws"):
        assert _ln(lib, **{name: None}) == ENULL, name
    assert _ln(lib, qtype=1) == ENULL                     # nonlinear needs t_quant
    assert _ln(lib, qtype=2) == EINVAL and _ln(lib, qtype=7) == EINVAL
    assert _ln(lib, rows=-1, ws_bytes=1 << 20) == EINVAL and _ln(lib, cols=0, ws_bytes=1 << 20) == EINVAL
    assert _ln(lib, ldx=60) == EINVAL and _ln(lib, ldg=60) == EINVAL and _ln(lib, ldo=60) == EINVAL
    assert _ln(lib, ws_bytes=16) == EINVAL
    # the fast path's rules
    assert _ln(lib, cols=62, ldx=64) == EALIGN
    assert _ln(lib, cols=2052, ldx=2052, ldg=2052, ldo=2052) == EALIGN
    assert _ln(lib, ldx=66) == EALIGN and _ln(lib, ldg=66) == EALIGN and _ln(lib, ldo=66) == EALIGN
    for name, v in (("x", 0x1004), ("gamma", 0x2008), ("beta", 0x3004), ("gy", 0x5008), ("gx", 0x6004), ("ws", 0xA008)):
        assert _ln(lib, **{name: v}) == EALIGN, name


def _ge(lib, h=0x1000, gy=0x2000, n=64, qtype=0, d=0x4000, qm=0x4010, t=None, gh=0x3000, sc=0x5000, ws=0x6000,
        ws_bytes=None):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    if ws_bytes is None:
        ws_bytes = max(0, int(lib.qvit_gelu_quant_backward_workspace_bytes(n)))
    return lib.qvit_gelu_quant_backward(p(h), p(gy), n, qtype, p(d), p(qm), p(t), -2.0, 2.0, p(gh), p(sc), p(ws),
                                        ws_bytes, None)


def test_gelu_rejections(lib):
    for name in ("h", "gy", "d", "qm", "gh", "sc", "ws"):
        assert _ge(lib, **{name: None}) == ENULL, name
    assert _ge(lib, qtype=1) == ENULL and _ge(lib, qtype=2) == EINVAL
    assert _ge(lib, n=-1, ws_bytes=64) == EINVAL and _ge(lib, ws_bytes=8) == EINVAL
    for name, v in (("h", 0x1004), ("gy", 0x2008), ("gh", 0x3004), ("ws", 0x6004)):
        assert _ge(lib, **{name: v}) == EALIGN, name
    p = ctypes.c_void_p
    fwd = lambda **k: lib.qvit_gelu_quant_i8(p(k.get("h", 0x1000)), k.get("rows", 4), k.get("cols", 60),
                                             k.get("ldh", 60), k.get("qtype", 0), p(0x4000), p(0x4010), None, 0,
                                             p(k.get("codes", 0x2000)), k.get("ldc", 64), k.get("kpad", 64), None)
    assert fwd(kpad=48) == EINVAL and fwd(kpad=60) == EINVAL and fwd(ldh=56) == EINVAL and fwd(ldc=48) == EINVAL
    assert fwd(rows=-1) == EINVAL and fwd(qtype=9) == EINVAL
    assert fwd(codes=0x2008) == EALIGN and fwd(ldc=72, kpad=64) == EALIGN
    assert fwd(rows=0) == 0
