"""Attention backward without a GPU: the float64 restatement agrees with the closed form the kernel implements,
the binding declares the new exports, and the workspace is O(B H N)."""
import pytest
import torch

import attention_backward_ref as R
from quantized_vit_amd import _lib, build


def test_restatement_matches_closed_form():
    B, N, H = 1, 5, 2
    qkv, dO, g64, _ = R.case(B, N, H)
    d, _, _ = R.closed_form(qkv, dO, B, N, H, R.HD ** -0.5)
    assert float((d - g64).abs().max()) <= 1e-12 * float(g64.abs().max())


def test_binding_declares_the_exports():
    assert "qvit_attention_backward" in _lib.EXPORTED_SYMBOLS
    assert "qvit_attention_backward_workspace_bytes" in _lib.EXPORTED_SYMBOLS
    assert len(_lib._SIGNATURES["qvit_attention_backward"]) == 18
    assert _lib.INT64_FUNCS["qvit_attention_backward_workspace_bytes"] == [_lib._i64] * 3
    assert callable(_lib.attention_backward)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_workspace_is_linear_in_the_sequence(lib):
    ws = lib.qvit_attention_backward_workspace_bytes
    B, N, H = 4, 197, 12
    base = ws(B, N, H)
    assert 0 < base < B * H * N * N * 4
    assert base <= 4 * (B * H * (2 * (N + 31) + 1) + 4)           # two floats per (padded) query, one per head
    assert ws(B + 1, N, H) > base and ws(B, N, H + 1) > base
    prev = 0
    for n in range(1, 700):
        cur = ws(B, n, H)
        assert cur >= prev
        prev = cur
    assert ws(B, 577, H) > base and ws(B, 2 * N, H) <= 2 * base + 4096
    assert ws(1, 0, 1) == -1 and ws(1, 1, 0) == -1 and ws(-1, 1, 1) == -1


def test_argument_validation_without_launch(lib):
    """Host checks only: nothing is dereferenced, nothing launched (runs without a GPU)."""
    import ctypes
    fake = ctypes.c_void_p(0x1000)
    B, N, H = 1, 5, 2
    C = H * 64
    nb = lib.qvit_attention_backward_workspace_bytes(B, N, H)

    def call(qkv=fake, out=fake, go=fake, hd=64, ldq=3 * C, ldo=C, ldgo=C, gq=fake, ldg=3 * C, ws=fake, wsb=nb):
        return lib.qvit_attention_backward(qkv, out, go, B, N, H, hd, ldq, ldo, ldgo, 0.125, 1.0, 1.0, gq, ldg, ws,
                                           wsb, None)
    assert call(hd=32) == -1
    assert call(gq=None) == -3
    assert call(qkv=None) == -3 and call(go=None) == -3 and call(out=None) == -3 and call(ws=None) == -3
    assert call(ldg=3 * C - 4) == -1
    assert call(ldq=3 * C - 4) == -1 and call(ldo=C - 4) == -1
    assert call(wsb=nb - 1) == -1
    assert call(ldq=3 * C + 2) == -2
    assert call(gq=ctypes.c_void_p(0x1008)) == -2
