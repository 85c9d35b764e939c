"""C ABI of qvit_col2im_quant_backward and its workspace query: exported symbols, documented signatures, and the
order of the host checks (include/qvit_hip.h), pinned the way tests/test_capi_rejections.py pins the other entry
points. Every call is answered by the host checks alone: nothing is dereferenced and nothing is launched, so this runs
without a GPU. A row is (overrides of a valid fused call, status); the rows that expect QVIT_OK use the fold-only
mode (x = NULL) with B = 0, which returns before any launch."""
import ctypes
import re
from pathlib import Path

import pytest

from quantized_vit_amd import _lib, build
from test_capi_rejections import CONV_GEO_BAD, _ax

OK, EINVAL, EALIGN, ENULL = 0, -1, -2, -3
LIN, NONLIN, ULTRA = _lib.QT_LINEAR, _lib.QT_NONLINEAR, _lib.QT_ULTRA_ACT
CAREFUL, STRAY = _lib.QT_FORCE_CAREFUL, 0x200
P0, X0, D0, QM0, T0, GX0, SC0, WS0 = (0x1000 * i for i in range(1, 9))
NAMES = ("qvit_col2im_quant_backward", "qvit_col2im_quant_backward_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)   # never dereferenced


def geo(B=2, C=3, H=8, W=8, k=3, s=1, p=1, dil=1, kh=None, kw=None, sh=None, sw=None, ph=None, pw=None, dh=None,
        dw=None):
    """k, s, p, dil go to both axes; kh .. dw override one axis each."""
    return (B, C, H, W, _ax(kh, k), _ax(kw, k), _ax(sh, s), _ax(sw, s), _ax(ph, p), _ax(pw, p), _ax(dh, dil),
            _ax(dw, dil))


def fold(lib, P=P0, ldp=27, x=X0, qtype=LIN, d=D0, qm=QM0, t=None, gx=GX0, sc=SC0, ws=WS0, wsb=None, **g):
    g = geo(**g)
    if wsb is None:
        wsb = max(0, int(lib.qvit_col2im_quant_backward_workspace_bytes(*g)))
    return lib.qvit_col2im_quant_backward(_p(P), ldp, _p(x), *g, qtype, _p(d), _p(qm), _p(t), -2.0, 2.0, _p(gx),
                                          _p(sc), _p(ws), wsb, None)


def test_symbols_and_signatures(lib):
    """Fails without the feature: the symbols do not exist."""
    header = (Path(build.INCLUDE) / "qvit_hip.h").read_text()
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.search(r"\b(int64_t|int)\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(2).replace("\n", " ").split(",")]
        want = [ctypes.c_void_p if ("*" in a or a.startswith("hipStream_t")) else ctype[a.split()[0]] for a in args]
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want, name
        assert fn.restype is (ctypes.c_int64 if m.group(1) == "int64_t" else ctypes.c_int)


ROWS = [
    # NULL pointers first: P and grad_x always, the quantizer's with x
    (dict(P=None), ENULL), (dict(gx=None), ENULL), (dict(sc=None), ENULL), (dict(d=None), ENULL),
    (dict(qm=None), ENULL), (dict(ws=None), ENULL),
    (dict(P=None, qtype=7), ENULL), (dict(gx=None, s=0), ENULL), (dict(ws=None, P=P0 + 2), ENULL),
    # the quantizer: qtype (EINVAL), then t_quant of the nonlinear one (ENULL), both in front of the geometry
    (dict(qtype=7), EINVAL), (dict(qtype=ULTRA), EINVAL), (dict(qtype=STRAY), EINVAL), (dict(qtype=CAREFUL | 7), EINVAL),
    (dict(qtype=NONLIN), ENULL), (dict(qtype=NONLIN, s=0), ENULL), (dict(qtype=NONLIN, t=T0, s=0), EINVAL),
    (dict(qtype=7, P=P0 + 2), EINVAL),
    # the geometry, then ldp, then the workspace size, then alignment
    *[(g, EINVAL) for g in CONV_GEO_BAD],
    (dict(W=2, pw=0, sw=2, P=P0 + 2), EINVAL), (dict(W=2, pw=0, sw=2, P=None), ENULL),
    (dict(B=-1), EINVAL), (dict(C=0), EINVAL), (dict(B=(1 << 20) + 1), EINVAL), (dict(H=(1 << 16) + 1), EINVAL),
    (dict(kw=1025), EINVAL), (dict(dh=1025), EINVAL), (dict(pw=(1 << 16) + 1), EINVAL),
    (dict(B=1 << 20, C=1 << 20, H=8, W=8, wsb=1 << 20), EINVAL),              # B C H W = 2^46
    (dict(ldp=26), EINVAL), (dict(ldp=(1 << 24) + 4), EINVAL), (dict(ldp=26, wsb=0), EINVAL),
    (dict(wsb=0), EINVAL), (dict(wsb=0, P=P0 + 2), EINVAL), (dict(ldp=26, gx=GX0 + 2), EINVAL),
    (dict(P=P0 + 2), EALIGN), (dict(x=X0 + 1), EALIGN), (dict(gx=GX0 + 2), EALIGN), (dict(ws=WS0 + 4), EALIGN),
    # fold only (x = NULL): the quantizer's arguments and the workspace are not looked at
    (dict(x=None, B=0, qtype=7, d=None, qm=None, sc=None, ws=None, wsb=0), OK),
    (dict(x=None, B=0, P=P0 + 4, gx=GX0 + 8), OK),                          # 4-byte alignment is enough
    (dict(x=None, B=0, P=P0 + 2), EALIGN), (dict(x=None, B=0, gx=None), ENULL), (dict(x=None, B=0, ldp=26), EINVAL),
    (dict(x=None, B=0, s=0), EINVAL),
    # each argument reaches its own axis: valid as given, no output with the pair swapped
    (dict(x=None, B=0, H=3, W=19, kh=1, kw=7, p=0, ldp=21), OK), (dict(x=None, H=3, W=19, kh=7, kw=1, p=0), EINVAL),
    (dict(x=None, B=0, C=1, H=3, W=19, k=5, ph=1, pw=0, ldp=25), OK),
    (dict(x=None, C=1, H=3, W=19, k=5, ph=0, pw=1), EINVAL),
]


def test_rejection_table(lib):
    got = [(kw, fold(lib, **kw)) for kw, _ in ROWS]
    wrong = [(kw, status, want) for (kw, status), (_, want) in zip(got, ROWS) if status != want]
    assert not wrong, "\n".join(f"fold({kw}) returned {s}, expected {w}" for kw, s, w in wrong)


def test_every_row_is_answered_before_a_launch():
    for kw, want in ROWS:
        assert want in (EINVAL, EALIGN, ENULL) or (want == OK and kw.get("x", X0) is None and kw.get("B") == 0), kw


def test_workspace_query(lib):
    q = lib.qvit_col2im_quant_backward_workspace_bytes
    assert int(q(*geo())) == 2 * 24                                     # 384 elements: two workgroups' partials
    assert int(q(*geo(B=0))) == 24
    assert int(q(256, 3, 224, 224, 16, 16, 16, 16, 0, 0, 1, 1)) == 1024 * 24   # the grid cap
    for g in CONV_GEO_BAD:
        assert int(q(*geo(**g))) == EINVAL, g
    for g in (dict(B=-1), dict(C=0), dict(B=(1 << 20) + 1), dict(W=(1 << 16) + 1), dict(kh=1025),
              dict(B=1 << 20, C=1 << 20)):
        assert int(q(*geo(**g))) == EINVAL, g
