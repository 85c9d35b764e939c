"""C-ABI of the fused BatchNorm2d -> quantizer -> max pool training kernels (ultra_bn_fuse.hip): exported symbols
with the declared signatures, the workspace queries and argument validation by the header's status conventions. No
kernel is launched (runs without a GPU): every call here is rejected before a launch."""
import ctypes
import os

import pytest

from quantized_vit_amd import _lib, build

ENULL, EALIGN, EINVAL = -3, -2, -1
NEW = ("qvit_bn_stats", "qvit_bn_act_pool_forward", "qvit_bn_act_pool_backward_reduce",
       "qvit_bn_act_pool_backward_dx")
NEW_I64 = ("qvit_bn_stats_workspace_bytes", "qvit_bn_act_pool_backward_workspace_bytes")
BIG = 1 << 20


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_symbols_exported(lib):
    for name in NEW + NEW_I64:
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert len(_lib._SIGNATURES["qvit_bn_stats"]) == 15
    assert len(_lib._SIGNATURES["qvit_bn_act_pool_forward"]) == 14
    assert len(_lib._SIGNATURES["qvit_bn_act_pool_backward_reduce"]) == 14
    assert len(_lib._SIGNATURES["qvit_bn_act_pool_backward_dx"]) == 16
    for name in NEW_I64:
        assert getattr(lib, name).restype is ctypes.c_int64
    assert "ultra_bn_fuse.hip" in build.SOURCES


def test_declared_in_the_header():
    with open(os.path.join(os.path.dirname(build.HERE), "include", "qvit_hip.h")) as f:
        text = f.read()
    for name in NEW:
        assert f"int {name}(" in text
    for name in NEW_I64:
        assert f"int64_t {name}(" in text


def test_the_forward_uses_the_shared_quantizer_routine():
    with open(os.path.join(build.HERE, "csrc", "ultra_bn_fuse.hip")) as f:
        text = f.read()
    assert "quant_code(" in text and "QVIT_QT_ULTRA_ACT" in text and "rintf(" not in text and "atomicAdd" not in text


BAD_SHAPES = [(1, 1, 1, 1),              # M < 2
              (0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, -1),
              (1, 1, 65536, 65536),      # H W past int32
              (1, 1, 46341, 46341),      # H W just past 2^31 - 1 - 8192
              (65536, 65536, 1, 2),      # B C past int32
              (1 << 20, 1 << 10, 128, 128)]   # the grid B C ceil(H W / 8192) past int32


def test_workspace_queries(lib):
    st, bw = lib.qvit_bn_stats_workspace_bytes, lib.qvit_bn_act_pool_backward_workspace_bytes
    for (B, C, H, W) in ((2, 1, 1, 1), (2, 3, 5, 7), (4, 2, 64, 64), (1, 2, 96, 96), (64, 16, 416, 416)):
        slices = (H * W + 8191) // 8192
        assert st(B, C, H, W) == 16 * B * C * slices
        assert bw(B, C, H, W, 0) == 16 * B * C * slices
        if H >= 2 and W >= 2:
            assert bw(B, C, H, W, 1) == 16 * B * C * (((H // 2) * (W // 2) + 2047) // 2048)
    for shape in BAD_SHAPES:
        assert st(*shape) == EINVAL and bw(*shape, 0) == EINVAL, shape
    assert bw(2, 1, 1, 4, 1) == EINVAL and bw(2, 1, 4, 1, 1) == EINVAL   # nothing to pool
    assert bw(2, 1, 4, 4, 2) == EINVAL and bw(2, 1, 4, 4, -1) == EINVAL


def _p(v):
    return None if v is None else ctypes.c_void_p(v)   # never dereferenced: rejected before any launch


def test_stats_rejections(lib):
    def call(x=0x1000, shape=(2, 3, 5, 7), eps=1e-5, rm=0x2000, rv=0x3000, mean=0x4000, var=0x5000, invstd=0x6000,
             ws=0x7000, ws_bytes=BIG):
        return lib.qvit_bn_stats(_p(x), *shape, eps, 0.1, _p(rm), _p(rv), _p(mean), _p(var), _p(invstd), _p(ws),
                                 ws_bytes, None)
    for name in ("x", "mean", "var", "invstd", "ws"):
        assert call(**{name: None}) == ENULL, name
    for shape in BAD_SHAPES:
        assert call(shape=shape) == EINVAL, shape
    assert call(ws_bytes=16 * 6 - 1) == EINVAL and call(eps=-1.0) == EINVAL and call(eps=float("nan")) == EINVAL
    for name, v in (("x", 0x1002), ("rm", 0x2001), ("rv", 0x3002), ("mean", 0x4001), ("var", 0x5002),
                    ("invstd", 0x6003), ("ws", 0x7004)):
        assert call(**{name: v}) == EALIGN, name


def test_forward_rejections(lib):
    def call(x=0x1000, shape=(2, 3, 5, 7), mean=0x2000, invstd=0x3000, gamma=0x4000, beta=0x5000, levels=15, pool=1,
             out=0x6000, flags=0x7000):
        return lib.qvit_bn_act_pool_forward(_p(x), *shape, _p(mean), _p(invstd), _p(gamma), _p(beta), levels, pool,
                                            _p(out), _p(flags), None)
    for name in ("x", "mean", "invstd", "out", "flags"):
        assert call(**{name: None}) == ENULL, name
    for levels in (0, -1, 128, 255):
        assert call(levels=levels) == EINVAL
    for shape in BAD_SHAPES:
        assert call(shape=shape, pool=0) == EINVAL, shape
    assert call(shape=(2, 3, 1, 7)) == EINVAL and call(shape=(2, 3, 5, 1)) == EINVAL and call(pool=2) == EINVAL
    for name, v in (("x", 0x1002), ("mean", 0x2001), ("invstd", 0x3002), ("gamma", 0x4001), ("beta", 0x5002),
                    ("out", 0x6002)):
        assert call(**{name: v}) == EALIGN, name


def test_backward_rejections(lib):
    def reduce(x=0x1000, g=0x2000, flags=0x3000, shape=(2, 3, 5, 7), mean=0x4000, invstd=0x5000, pool=1,
               sums=0x6000, ws=0x7000, ws_bytes=BIG):
        return lib.qvit_bn_act_pool_backward_reduce(_p(x), _p(g), _p(flags), *shape, _p(mean), _p(invstd), pool,
                                                    _p(sums), _p(ws), ws_bytes, None)

    def dx(x=0x1000, g=0x2000, flags=0x3000, shape=(2, 3, 5, 7), mean=0x4000, invstd=0x5000, gamma=0x6000,
           sums=0x7000, pool=1, dx=0x8000, dgamma=0x9000, dbeta=0xa000):
        return lib.qvit_bn_act_pool_backward_dx(_p(x), _p(g), _p(flags), *shape, _p(mean), _p(invstd), _p(gamma),
                                                _p(sums), pool, _p(dx), _p(dgamma), _p(dbeta), None)
    for name in ("x", "g", "flags", "mean", "invstd", "sums", "ws"):
        assert reduce(**{name: None}) == ENULL, name
    for name in ("x", "g", "flags", "mean", "invstd", "sums", "dx"):
        assert dx(**{name: None}) == ENULL, name
    for shape in BAD_SHAPES:
        assert reduce(shape=shape, pool=0) == EINVAL and dx(shape=shape, pool=0) == EINVAL, shape
    assert reduce(shape=(2, 3, 1, 7)) == EINVAL and dx(shape=(2, 3, 5, 1)) == EINVAL
    assert reduce(pool=3) == EINVAL and dx(pool=3) == EINVAL
    assert reduce(ws_bytes=16 * 6 - 1) == EINVAL
    for name, v in (("x", 0x1002), ("g", 0x2001), ("mean", 0x4002), ("invstd", 0x5001), ("sums", 0x6004),
                    ("ws", 0x7004)):
        assert reduce(**{name: v}) == EALIGN, name
    for name, v in (("x", 0x1002), ("g", 0x2001), ("mean", 0x4002), ("invstd", 0x5001), ("gamma", 0x6002),
                    ("sums", 0x7004), ("dx", 0x8002), ("dgamma", 0x9001), ("dbeta", 0xa002)):
        assert dx(**{name: v}) == EALIGN, name


def test_the_flag_is_off_by_default_and_validated(monkeypatch):
    from quantized_vit_amd import quant_ultra as Q
    assert os.environ.get("QVIT_ULTRA_TRAIN_FUSE", "0") != "0" or Q.ULTRA_TRAIN_FUSE == "0"
    for v, want in (("0", False), ("1", True)):
        monkeypatch.setattr(Q, "ULTRA_TRAIN_FUSE", v)
        assert Q.train_fuse_enabled() is want
    monkeypatch.setattr(Q, "ULTRA_TRAIN_FUSE", "yes")
    with pytest.raises(ValueError, match="expected 0 or 1"):
        Q.train_fuse_enabled()
