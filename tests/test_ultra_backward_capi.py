"""C-ABI of UltraNet's training kernels (ultra_backward.hip): exported symbols with the declared signatures, the
workspace queries and argument validation by the header's status conventions. No kernel is launched (runs without
a GPU): every call here is rejected before a launch."""
import ctypes
import os

import pytest

from quantized_vit_amd import _lib, build

ENULL, EALIGN, EINVAL = -3, -2, -1
NEW = ("qvit_ultra_weight_quant_backward", "qvit_ultra_act_quant_backward", "qvit_conv_wgrad")
NEW_I64 = ("qvit_ultra_weight_quant_backward_workspace_bytes", "qvit_conv_wgrad_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_symbols_exported(lib):
    for name in NEW + NEW_I64:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert len(_lib._SIGNATURES["qvit_ultra_weight_quant_backward"]) == 8
    assert len(_lib._SIGNATURES["qvit_ultra_act_quant_backward"]) == 5
    assert len(_lib._SIGNATURES["qvit_conv_wgrad"]) == 20
    assert len(_lib.INT64_FUNCS["qvit_conv_wgrad_workspace_bytes"]) == 13
    for name in NEW_I64:
        assert getattr(lib, name).restype is ctypes.c_int64
    assert "ultra_backward.hip" in build.SOURCES and "ultra_quant_common.h" in build.HEADERS


def test_declared_in_the_header():
    with open(os.path.join(os.path.dirname(build.HERE), "include", "qvit_hip.h")) as f:
        text = f.read()
    for name in NEW:
        assert f"int {name}(" in text
    for name in NEW_I64:
        assert f"int64_t {name}(" in text
    assert "quant_ultra.py:23-25" in text and "quant_ultra.py:50-55" in text and "quant_ultra.py:85-89" in text


def test_forward_and_backward_share_the_tanh_and_max_routines():
    csrc = os.path.join(build.HERE, "csrc")
    with open(os.path.join(csrc, "ultra_conv.hip")) as f:
        fwd = f.read()
    with open(os.path.join(csrc, "ultra_backward.hip")) as f:
        bwd = f.read()
    for text in (fwd, bwd):
        assert '#include "ultra_quant_common.h"' in text and "tanhf(" not in text
        assert "ultra_tanh(" in text and "ultra_wmax_kernel" in text


def test_workspace_queries(lib):
    wq, cw = lib.qvit_ultra_weight_quant_backward_workspace_bytes, lib.qvit_conv_wgrad_workspace_bytes
    assert wq(-1) == EINVAL
    for n in (0, 1, 255, 1025, 64 * 576, 1 << 24):
        assert wq(n) == 16 + max(1, min(1024, (n + 255) // 256)) * 16
    r64 = lambda v: (v + 63) // 64 * 64
    for (B, C, H, W, N, k, s, p, d) in ((1, 1, 1, 1, 1, 1, 1, 0, 1), (2, 3, 5, 7, 5, 3, 1, 1, 1),
                                        (2, 16, 40, 40, 16, 3, 1, 1, 1), (256, 64, 26, 26, 64, 3, 1, 1, 1),
                                        (1, 4, 11, 13, 8, 3, 2, 1, 1)):
        OH, OW = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
        tiles = (r64(N) // 64) * (r64(C * k * k) // 64)
        splits = max(1, min(256, (B * OH * OW + 31) // 32, (2048 + tiles - 1) // tiles))
        assert cw(B, C, H, W, N, k, k, s, s, p, p, d, d) == splits * r64(N) * r64(C * k * k) * 4
    assert cw(1, 1, 2, 2, 1, 3, 3, 1, 1, 0, 0, 1, 1) == EINVAL       # empty output
    assert cw(1, 0, 2, 2, 1, 1, 1, 1, 1, 0, 0, 1, 1) == EINVAL and cw(1, 1, 2, 2, 1, 1, 1, 0, 1, 0, 0, 1, 1) == EINVAL
    assert cw(1 << 20, 1, 64, 64, 1, 1, 1, 1, 1, 0, 0, 1, 1) == EINVAL   # B OH OW past int32


def _p(v):
    return None if v is None else ctypes.c_void_p(v)   # never dereferenced: rejected before any launch


def test_weight_quant_backward_rejections(lib):
    def call(w=0x1000, g=0x2000, n=64, w_bit=4, gw=0x3000, ws=0x4000, ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = max(0, int(lib.qvit_ultra_weight_quant_backward_workspace_bytes(n)))
        return lib.qvit_ultra_weight_quant_backward(_p(w), _p(g), n, w_bit, _p(gw), _p(ws), ws_bytes, None)
    for name in ("w", "g", "gw", "ws"):
        assert call(**{name: None}) == ENULL, name
    assert call(n=-1, ws_bytes=64) == EINVAL and call(ws_bytes=16) == EINVAL
    assert call(w_bit=1) == EINVAL and call(w_bit=9) == EINVAL and call(w_bit=32) == EINVAL
    for name, v in (("w", 0x1002), ("g", 0x2001), ("gw", 0x3002), ("ws", 0x4004)):
        assert call(**{name: v}) == EALIGN, name
    assert call(n=0) == 0


def test_act_quant_backward_rejections(lib):
    call = lambda x=0x1000, g=0x2000, n=64, gx=0x3000: lib.qvit_ultra_act_quant_backward(_p(x), _p(g), n, _p(gx), None)
    for name in ("x", "g", "gx"):
        assert call(**{name: None}) == ENULL, name
    assert call(n=-1) == EINVAL
    for name, v in (("x", 0x1004), ("g", 0x2008), ("gx", 0x3004)):
        assert call(**{name: v}) == EALIGN, name
    assert call(n=0) == 0


def test_conv_wgrad_rejections(lib):
    def call(G=0x1000, X=0x2000, B=2, C=3, H=5, W=7, N=5, k=3, s=1, p=1, d=1, levels=15, dW=0x3000, ws=0x4000,
             ws_bytes=None):
        if ws_bytes is None:
            ws_bytes = max(0, int(lib.qvit_conv_wgrad_workspace_bytes(B, C, H, W, N, k, k, s, s, p, p, d, d)))
        return lib.qvit_conv_wgrad(_p(G), _p(X), B, C, H, W, N, k, k, s, s, p, p, d, d, levels, _p(dW), _p(ws),
                                   ws_bytes, None)
    for name in ("G", "X", "dW", "ws"):
        assert call(**{name: None}) == ENULL, name
    assert call(levels=0) == EINVAL and call(levels=128) == EINVAL
    assert call(B=-1, ws_bytes=1 << 20) == EINVAL and call(s=0, ws_bytes=1 << 20) == EINVAL
    assert call(p=-1, ws_bytes=1 << 20) == EINVAL and call(H=1, W=1, p=0, ws_bytes=1 << 20) == EINVAL
    assert call(ws_bytes=64) == EINVAL
    for name, v in (("G", 0x1002), ("X", 0x2001), ("dW", 0x3002), ("ws", 0x4008)):
        assert call(**{name: v}) == EALIGN, name
