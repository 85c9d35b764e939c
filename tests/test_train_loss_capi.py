"""C ABI of qvit_train_loss: the exported symbols and every rejection include/qvit_hip.h lists, through fake pointers
that validation never dereferences (nothing is launched: this runs without a GPU), and the module's own refusals."""
import ctypes

import pytest
import torch

from quantized_vit_amd import _lib, build

OK, EINVAL, EALIGN, ENULL = 0, -1, -2, -3
S, T, LA, LB, G, OUT, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def call(lib, logits=S, B=4, C=10, lds=10, teacher=T, ldt=10, la=LA, lb=LB, gamma=0.3, eps=0.1, alpha=0.5, temp=5.0,
         g=G, ldg=10, out=OUT, ws=WS, ws_bytes=None):
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    ws_bytes = max(0, lib.qvit_train_loss_workspace_bytes(B)) if ws_bytes is None else ws_bytes
    return lib.qvit_train_loss(p(logits), B, C, lds, p(teacher), ldt, p(la), p(lb), gamma, eps, alpha, temp, p(g),
                               ldg, p(out), p(ws), ws_bytes, None)


def test_symbols_and_source():
    """Fails without the feature: the symbols do not exist."""
    for name in ("qvit_train_loss", "qvit_train_loss_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert "train_loss.hip" in build.SOURCES


# every row is answered by the host checks alone: a rejection, or B == 0
ROWS = [
    (dict(logits=None), ENULL), (dict(la=None), ENULL), (dict(out=None), ENULL), (dict(ws=None), ENULL),
    (dict(logits=None, B=-1), ENULL),
    (dict(B=-1), EINVAL), (dict(B=(1 << 24) + 1, ws_bytes=1 << 40), EINVAL), (dict(C=0), EINVAL),
    (dict(lds=9), EINVAL), (dict(ldt=9), EINVAL), (dict(ldg=9), EINVAL),
    (dict(temp=0.0), EINVAL), (dict(temp=-1.0), EINVAL), (dict(temp=INF), EINVAL), (dict(temp=NAN), EINVAL),
    (dict(eps=-0.1), EINVAL), (dict(eps=1.5), EINVAL), (dict(eps=NAN), EINVAL),
    (dict(gamma=-0.1), EINVAL), (dict(gamma=1.5), EINVAL), (dict(gamma=NAN), EINVAL),
    (dict(alpha=-0.1), EINVAL), (dict(alpha=1.5), EINVAL), (dict(alpha=NAN), EINVAL),
    (dict(ws_bytes=4 * 32 - 1), EINVAL),
    (dict(logits=S + 2), EALIGN), (dict(teacher=T + 2), EALIGN), (dict(g=G + 2), EALIGN), (dict(la=LA + 4), EALIGN),
    (dict(lb=LB + 4), EALIGN), (dict(ws=WS + 4), EALIGN), (dict(out=OUT + 2), EALIGN),
    # B == 0 returns OK without a launch; the optional pointers may be absent, and then their strides are not read
    (dict(B=0), OK), (dict(B=0, teacher=None, ldt=0, lb=None, g=None, ldg=0), OK),
]


@pytest.mark.parametrize("kw,want", ROWS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in ROWS])
def test_rejections(lib, kw, want):
    assert call(lib, **kw) == want


def test_workspace_query(lib):
    assert lib.qvit_train_loss_workspace_bytes(256) == 256 * 32 and lib.qvit_train_loss_workspace_bytes(0) == 0
    assert lib.qvit_train_loss_workspace_bytes(-1) == EINVAL


def test_module_refuses_what_the_kernel_does_not_take():
    """No CPU fallback, and the refusal names the offending property."""
    from quantized_vit_amd import TrainLoss
    QvitError = _lib.QvitError
    with pytest.raises(QvitError, match="ROCm device"):
        TrainLoss()(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(QvitError, match="kd_temperature"):
        TrainLoss(kd_temperature=0.0)
    with pytest.raises(QvitError, match="gamma"):
        TrainLoss()(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), mix=(torch.zeros(2, dtype=torch.int64), 2))
