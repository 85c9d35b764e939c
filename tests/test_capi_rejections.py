"""Status codes of the C ABI's argument checks, entry point by entry point: which code a rejected call returns and
which check wins when a call breaks two rules at once (QVIT_ENULL, QVIT_EINVAL and QVIT_EALIGN have an order inside
every entry point, and it is part of the ABI). Every call here is answered by the host checks alone: nothing is
dereferenced and nothing is launched, so the table runs without a GPU. A row is (overrides of a valid call, status).
Most rows are rejections; a row that expects QVIT_OK sets to zero the size on which its entry point returns before
its launch (EARLY names that argument per entry point), which shows that the checks in front of it were passed."""
import ctypes

import pytest

from quantized_vit_amd import _lib, build

OK, EINVAL, EALIGN, ENULL = 0, -1, -2, -3
LIN, NONLIN, ULTRA = _lib.QT_LINEAR, _lib.QT_NONLINEAR, _lib.QT_ULTRA_ACT
CAREFUL = _lib.QT_FORCE_CAREFUL   # the one flag bit a qtype may carry
STRAY = 0x200     # any other high bit


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)   # never dereferenced


A0, A1, A2, A3, A4, A5, A6, A7, A8, A9 = (0x1000 * i for i in range(1, 11))


def quantize_act(lib, fn="qvit_quantize_act_i8", x=A0, rows=4, cols=16, ldx=16, qtype=LIN, d=A1, qm=A2, t=None,
                 levels=0, codes=A3, ldc=16, kpad=16):
    return getattr(lib, fn)(_p(x), rows, cols, ldx, qtype, _p(d), _p(qm), _p(t), levels, _p(codes), ldc, kpad, None)


def gelu_quant(lib, **kw):
    return quantize_act(lib, fn="qvit_gelu_quant_i8", **kw)


# the forward quantizer rule (qtype flags, enum, then the scalars the enum needs) in front of a 16-byte code pointer
ROWS_TO_CODES = [
    (dict(x=None), ENULL), (dict(codes=None), ENULL),
    (dict(qtype=7), EINVAL), (dict(qtype=CAREFUL | 7), EINVAL), (dict(qtype=STRAY), EINVAL),
    (dict(d=None), EINVAL), (dict(qm=None), EINVAL),
    (dict(qtype=ULTRA, d=None, qm=None, levels=0), EINVAL), (dict(qtype=ULTRA, d=None, qm=None, levels=128), EINVAL),
    (dict(kpad=12), EINVAL), (dict(ldx=8), EINVAL), (dict(rows=-1), EINVAL), (dict(ldc=8), EINVAL),
    (dict(codes=A3 + 8), EALIGN), (dict(ldc=24), EALIGN),
    (dict(qtype=CAREFUL, codes=A3 + 8), EALIGN),                               # the careful bit is accepted
    (dict(qtype=ULTRA, d=None, qm=None, levels=127, codes=A3 + 8), EALIGN),     # so are 1 and 127 levels
    (dict(qtype=ULTRA, d=None, qm=None, levels=1, codes=A3 + 8), EALIGN),
    (dict(x=None, qtype=7), ENULL), (dict(x=None, kpad=12, codes=A3 + 8), ENULL),   # NULL, then sizes, then alignment
    (dict(qtype=STRAY, codes=A3 + 8), EINVAL), (dict(kpad=12, codes=A3 + 8), EINVAL),
    (dict(rows=0), OK), (dict(rows=0, codes=A3 + 8), EALIGN),
]


def fake_quant(lib, x=A0, n=8, qtype=LIN, d=A1, qm=A2, t=None, levels=0, y=A3):
    return lib.qvit_fake_quant_f32(_p(x), n, qtype, _p(d), _p(qm), _p(t), levels, _p(y), None)


FAKE_QUANT = [
    (dict(x=None), ENULL), (dict(y=None), ENULL), (dict(x=None, qtype=7), ENULL),
    (dict(qtype=7), EINVAL), (dict(qtype=STRAY, n=0), EINVAL), (dict(qtype=CAREFUL, n=0), OK),
    (dict(d=None), EINVAL), (dict(qtype=ULTRA, levels=0, n=0), EINVAL), (dict(qtype=ULTRA, levels=128, n=0), EINVAL),
    (dict(qtype=ULTRA, levels=15, n=0), OK), (dict(n=-1), EINVAL),
]


def pack_weight(lib, w=A0, n=256, k=128, ldw=128, qtype=LIN, d=A1, qm=A2, t=None, wfmt=_lib.W4, packed=A3, npad=256,
                kpad=128, overflow=None):
    return lib.qvit_pack_weight(_p(w), n, k, ldw, qtype, _p(d), _p(qm), _p(t), wfmt, _p(packed), npad, kpad,
                                _p(overflow), None)


PACK_WEIGHT = [
    (dict(w=None), ENULL), (dict(packed=None), ENULL), (dict(w=None, qtype=7, npad=100), ENULL),
    (dict(qtype=7), EINVAL), (dict(qtype=ULTRA), EINVAL), (dict(qtype=STRAY), EINVAL), (dict(d=None), EINVAL),
    (dict(wfmt=5), EINVAL), (dict(npad=100), EINVAL), (dict(n=0), EINVAL), (dict(kpad=100), EINVAL),
    (dict(packed=A3 + 8), EALIGN), (dict(qtype=CAREFUL, packed=A3 + 8), EALIGN),
    (dict(npad=100, packed=A3 + 8), EINVAL), (dict(qtype=STRAY, packed=A3 + 8), EINVAL),
]


def _ax(one, both):
    return both if one is None else one


# Geometries that every entry point with (kh .. dw) arguments rejects with QVIT_EINVAL, as overrides of a valid call
# with a 3 x 3 kernel, stride 1, padding 1 on an image of at least 5 x 5: the extent H + 2 ph - dh (kh - 1) - 1 of one
# axis is -1 at a stride of 2 (a division that truncates toward zero would make one output of it), or one argument of
# one axis is out of range while the other axis is valid.
CONV_GEO_BAD = [
    dict(W=2, pw=0, sw=2), dict(H=2, ph=0, sh=2),                    # a kernel one past the image, stride 2
    dict(W=4, pw=0, sw=2, dw=2), dict(H=4, ph=0, sh=2, dh=2),        # the image holds the kernel, not the dilated one
    dict(kh=0), dict(kw=0), dict(sh=0), dict(sw=0), dict(dh=0), dict(dw=0), dict(ph=-1), dict(pw=-1),
]


def im2col(lib, x=A0, B=1, C=3, H=8, W=8, k=3, s=1, p=1, dil=1, qtype=LIN, d=A1, qm=A2, t=None, levels=0, codes=A3,
           ldc=32, kpad=32, kh=None, kw=None, sh=None, sw=None, ph=None, pw=None, dh=None, dw=None):
    """k, s, p, dil go to both axes; kh .. dw override one axis each."""
    return lib.qvit_im2col_quant_i8(_p(x), B, C, H, W, _ax(kh, k), _ax(kw, k), _ax(sh, s), _ax(sw, s), _ax(ph, p),
                                    _ax(pw, p), _ax(dh, dil), _ax(dw, dil), qtype, _p(d), _p(qm), _p(t), levels, _p(codes), ldc, kpad,
                                    None)


IM2COL = [
    (dict(x=None), ENULL), (dict(codes=None), ENULL), (dict(x=None, s=0), ENULL),
    (dict(qtype=7), EINVAL), (dict(qtype=STRAY, B=0), EINVAL), (dict(qtype=CAREFUL, B=0), OK),
    (dict(qtype=ULTRA, levels=0, B=0), EINVAL), (dict(qtype=ULTRA, levels=128, B=0), EINVAL),
    (dict(qtype=ULTRA, levels=15, B=0), OK), (dict(qm=None), EINVAL),
    (dict(s=0), EINVAL), (dict(kpad=16), EINVAL), (dict(H=1, W=1, p=0), EINVAL),
    (dict(codes=A3 + 4), EALIGN), (dict(ldc=40), EALIGN), (dict(kpad=16, codes=A3 + 4), EINVAL),
    (dict(qtype=7, codes=A3 + 4), EINVAL),
    # one axis bad, the other valid
    (dict(kh=0), EINVAL), (dict(kw=0), EINVAL), (dict(sh=0), EINVAL), (dict(sw=0), EINVAL),
    (dict(ph=-1), EINVAL), (dict(pw=-1), EINVAL), (dict(dh=0), EINVAL), (dict(dw=0), EINVAL),
    (dict(W=1, pw=0), EINVAL), (dict(H=1, ph=0), EINVAL),                  # OH > 0, OW <= 0 and the reverse
    (dict(W=2, pw=0, sw=2), EINVAL), (dict(H=2, ph=0, sh=2), EINVAL),      # a kernel one past the image, stride 2
    # each argument reaches its own axis: valid as given, no output with the pair swapped
    (dict(B=0, H=3, W=19, kh=1, kw=7, p=0), OK), (dict(H=3, W=19, kh=7, kw=1, p=0), EINVAL),
    (dict(B=0, H=3, W=19, kh=1, kw=3, p=0, dw=9), OK), (dict(H=3, W=19, kh=3, kw=1, p=0, dh=9), EINVAL),
    (dict(B=0, C=1, H=3, W=19, k=5, ph=1, pw=0), OK), (dict(C=1, H=3, W=19, k=5, ph=0, pw=1), EINVAL),
    (dict(B=0, C=1, H=13, W=22, kh=2, kw=5, sh=2, sw=3, ph=3, pw=1, dh=3, dw=2), OK),
]


def ln_quant(lib, x=A0, rows=4, cols=16, ldx=16, gamma=A1, beta=A2, qtype=LIN, d=A3, qm=A4, t=None, levels=0, codes=A5,
             ldc=16, kpad=16, table=None):
    return lib.qvit_layernorm_quant_i8(_p(x), rows, cols, ldx, _p(gamma), _p(beta), 1e-5, qtype, _p(d), _p(qm), _p(t),
                                       levels, _p(codes), ldc, kpad, _p(table), None)


LN_QUANT = [
    (dict(x=None), ENULL), (dict(codes=None), ENULL), (dict(x=None, table=A6 + 8), ENULL),
    (dict(table=A6 + 8), EALIGN), (dict(table=A6 + 8, qtype=7), EALIGN),     # the table's alignment comes first
    (dict(qtype=7), EINVAL), (dict(qtype=STRAY, rows=0), EINVAL), (dict(qtype=CAREFUL, rows=0), OK),
    (dict(qtype=ULTRA, levels=0, rows=0), EINVAL), (dict(qtype=ULTRA, levels=128, rows=0), EINVAL),
    (dict(qtype=ULTRA, levels=127, rows=0), OK), (dict(d=None), EINVAL),
    (dict(cols=0), EINVAL), (dict(ldx=8), EINVAL), (dict(kpad=8), EINVAL),
    (dict(codes=A5 + 2), EALIGN), (dict(ldc=18), EALIGN), (dict(cols=0, codes=A5 + 2), EINVAL),
]


def ln_quant_t32(lib, x=A0, rows=4, cols=64, ldx=64, gamma=A1, beta=A2, qtype=LIN, d=A3, qm=A4, t=None, levels=0,
                 codes=A5, kpad=64, table=None):
    return lib.qvit_layernorm_quant_i8_t32(_p(x), rows, cols, ldx, _p(gamma), _p(beta), 1e-5, qtype, _p(d), _p(qm),
                                           _p(t), levels, _p(codes), kpad, _p(table), None)


LN_QUANT_T32 = [
    (dict(x=None), ENULL), (dict(codes=None), ENULL), (dict(table=A6 + 8), EALIGN), (dict(table=A6 + 8, cols=6), EALIGN),
    (dict(qtype=7), EINVAL), (dict(qtype=STRAY, rows=0), EINVAL), (dict(qtype=CAREFUL, rows=0), OK),
    (dict(qtype=ULTRA, levels=0, rows=0), EINVAL), (dict(qtype=ULTRA, levels=128, rows=0), EINVAL),
    (dict(cols=1028, ldx=1028, kpad=1088), EINVAL), (dict(cols=6), EINVAL), (dict(kpad=80), EINVAL),
    (dict(ldx=66), EALIGN), (dict(x=A0 + 4), EALIGN), (dict(gamma=A1 + 4), EALIGN), (dict(beta=A2 + 8), EALIGN),
    (dict(codes=A5 + 4), EALIGN), (dict(cols=6, x=A0 + 4), EINVAL), (dict(qtype=7, x=A0 + 4), EINVAL),
]


def quant_backward(lib, x=A0, g=A1, n=4099, qtype=LIN, d=A2, qm=A3, t=None, k=0.0, gx=A4, sc=A5, ws=A6, wsb=None):
    if wsb is None:
        wsb = max(0, int(lib.qvit_quant_backward_workspace_bytes(n)))
    return lib.qvit_quant_backward(_p(x), _p(g), n, qtype, _p(d), _p(qm), _p(t), -2.0, 2.0, k, _p(gx), _p(sc), _p(ws),
                                   wsb, None)


def gelu_quant_backward(lib, x=A0, g=A1, n=4099, qtype=LIN, d=A2, qm=A3, t=None, gx=A4, sc=A5, ws=A6, wsb=None):
    if wsb is None:
        wsb = max(0, int(lib.qvit_gelu_quant_backward_workspace_bytes(n)))
    return lib.qvit_gelu_quant_backward(_p(x), _p(g), n, qtype, _p(d), _p(qm), _p(t), -2.0, 2.0, _p(gx), _p(sc),
                                        _p(ws), wsb, None)


# the backward rule: flags, then LINEAR / NONLINEAR only; NONLINEAR needs t (ENULL) before any size is looked at
STREAM_BACKWARD = [
    (dict(x=None), ENULL), (dict(g=None), ENULL), (dict(gx=None), ENULL), (dict(sc=None), ENULL), (dict(d=None), ENULL),
    (dict(qm=None), ENULL), (dict(ws=None), ENULL), (dict(x=None, qtype=7), ENULL),
    (dict(qtype=7), EINVAL), (dict(qtype=ULTRA), EINVAL), (dict(qtype=STRAY), EINVAL), (dict(qtype=CAREFUL | ULTRA), EINVAL),
    (dict(qtype=NONLIN), ENULL), (dict(qtype=NONLIN, n=-1, wsb=64), ENULL), (dict(qtype=STRAY | NONLIN), EINVAL),
    (dict(n=-1, wsb=64), EINVAL), (dict(wsb=0), EINVAL),
    (dict(x=A0 + 8), EALIGN), (dict(g=A1 + 4), EALIGN), (dict(gx=A4 + 8), EALIGN), (dict(ws=A6 + 4), EALIGN),
    (dict(qtype=CAREFUL, x=A0 + 8), EALIGN), (dict(qtype=CAREFUL | NONLIN, t=A7, ws=A6 + 4), EALIGN),
    (dict(n=-1, wsb=64, x=A0 + 8), EINVAL), (dict(wsb=0, x=A0 + 8), EINVAL), (dict(qtype=7, x=A0 + 8), EINVAL),
]
QUANT_BACKWARD_ONLY = [(dict(k=-1.0), EINVAL), (dict(k=-1.0, x=A0 + 8), EINVAL),
                       (dict(qtype=NONLIN, t=A7, k=2.0), EINVAL)]


def ln_quant_backward(lib, x=A0, rows=5, cols=64, ldx=64, gamma=A1, beta=A2, qtype=LIN, d=A3, qm=A4, t=None, gy=A5,
                      ldg=64, gx=A6, ldo=64, gg=None, gb=None, sc=A7, ws=A8, wsb=None):
    if wsb is None:
        wsb = max(0, int(lib.qvit_layernorm_quant_backward_workspace_bytes(rows, cols)))
    return lib.qvit_layernorm_quant_backward(_p(x), rows, cols, ldx, _p(gamma), _p(beta), 1e-5, qtype, _p(d), _p(qm),
                                             _p(t), -2.0, 2.0, _p(gy), ldg, _p(gx), ldo, _p(gg), _p(gb), _p(sc), _p(ws),
                                             wsb, None)


LN_QUANT_BACKWARD = [
    (dict(x=None), ENULL), (dict(gamma=None), ENULL), (dict(gy=None), ENULL), (dict(ws=None), ENULL),
    (dict(x=None, qtype=7, cols=0), ENULL),
    (dict(qtype=7), EINVAL), (dict(qtype=ULTRA), EINVAL), (dict(qtype=STRAY), EINVAL),
    (dict(qtype=NONLIN), ENULL), (dict(qtype=NONLIN, cols=0, wsb=1 << 20), ENULL),
    (dict(cols=0, wsb=1 << 20), EINVAL), (dict(ldx=60), EINVAL), (dict(wsb=8), EINVAL), (dict(rows=-1, wsb=1 << 20), EINVAL),
    (dict(cols=66, ldx=68, ldg=68, ldo=68), EALIGN), (dict(cols=2052, ldx=2052, ldg=2052, ldo=2052), EALIGN),
    (dict(ldg=66), EALIGN), (dict(x=A0 + 8), EALIGN), (dict(ws=A8 + 8), EALIGN), (dict(beta=A2 + 4), EALIGN),
    (dict(gg=A9 + 2), EALIGN), (dict(gb=A9 + 1), EALIGN),
    (dict(qtype=CAREFUL, x=A0 + 8), EALIGN), (dict(cols=0, wsb=1 << 20, x=A0 + 8), EINVAL), (dict(wsb=8, x=A0 + 8), EINVAL),
]


def wq_backward(lib, w=A0, g=A1, n=64, w_bit=4, gw=A2, ws=A3, wsb=None):
    if wsb is None:
        wsb = max(0, int(lib.qvit_ultra_weight_quant_backward_workspace_bytes(n)))
    return lib.qvit_ultra_weight_quant_backward(_p(w), _p(g), n, w_bit, _p(gw), _p(ws), wsb, None)


WQ_BACKWARD = [
    (dict(w=None), ENULL), (dict(ws=None, n=-1), ENULL), (dict(n=-1, wsb=64), EINVAL), (dict(w_bit=1), EINVAL),
    (dict(wsb=16), EINVAL), (dict(w=A0 + 2), EALIGN), (dict(g=A1 + 1), EALIGN), (dict(gw=A2 + 2), EALIGN),
    (dict(ws=A3 + 4), EALIGN), (dict(w_bit=9, w=A0 + 2), EINVAL), (dict(wsb=16, ws=A3 + 4), EINVAL),
    (dict(n=0), OK), (dict(n=0, ws=A3 + 4), EALIGN),
]


def act_backward(lib, x=A0, g=A1, n=64, gx=A2):
    return lib.qvit_ultra_act_quant_backward(_p(x), _p(g), n, _p(gx), None)


ACT_BACKWARD = [
    (dict(x=None), ENULL), (dict(gx=None, n=-1), ENULL), (dict(n=-1), EINVAL), (dict(x=A0 + 4), EALIGN),
    (dict(g=A1 + 8), EALIGN), (dict(gx=A2 + 4), EALIGN), (dict(n=-1, x=A0 + 4), EINVAL), (dict(n=0), OK),
    (dict(n=0, gx=A2 + 4), EALIGN),
]


def conv_wgrad_geo(B=2, C=3, H=5, W=7, N=5, k=3, s=1, p=1, dil=1, kh=None, kw=None, sh=None, sw=None, ph=None, pw=None,
                   dh=None, dw=None):
    """The geometry arguments of qvit_conv_wgrad and its workspace query: k, s, p, dil go to both axes; kh .. dw
    override one axis each."""
    return (B, C, H, W, N, _ax(kh, k), _ax(kw, k), _ax(sh, s), _ax(sw, s), _ax(ph, p), _ax(pw, p), _ax(dh, dil),
            _ax(dw, dil))


def conv_wgrad(lib, G=A0, X=A1, levels=15, dW=A2, ws=A3, wsb=None, **geo):
    geo = conv_wgrad_geo(**geo)
    if wsb is None:
        wsb = max(0, int(lib.qvit_conv_wgrad_workspace_bytes(*geo)))
    return lib.qvit_conv_wgrad(_p(G), _p(X), *geo, levels, _p(dW), _p(ws), wsb, None)


CONV_WGRAD = [
    (dict(G=None), ENULL), (dict(ws=None, s=0), ENULL), (dict(s=0, wsb=1 << 20), EINVAL), (dict(levels=0), EINVAL),
    (dict(levels=128), EINVAL), (dict(G=A0 + 2), EALIGN), (dict(X=A1 + 1), EALIGN), (dict(dW=A2 + 2), EALIGN),
    (dict(ws=A3 + 8), EALIGN), (dict(levels=0, G=A0 + 2), EINVAL), (dict(s=0, wsb=1 << 20, ws=A3 + 8), EINVAL),
    (dict(wsb=64), EINVAL), (dict(wsb=64, ws=A3 + 8), EALIGN),   # here the workspace size is looked at last
    *[(geo, EINVAL) for geo in CONV_GEO_BAD],
    # a bad extent is looked at after the null pointers and before the alignment
    (dict(W=2, pw=0, sw=2, G=A0 + 2), EINVAL), (dict(W=2, pw=0, sw=2, G=None), ENULL),
]


def gemm_wgrad(lib, G=A0, M=64, N=48, ldg=48, A=A1, K=64, lda=64, d=A2, dW=A3, ldw=64, ws=A4, wsb=None):
    if wsb is None:
        wsb = max(0, int(lib.qvit_gemm_wgrad_workspace_bytes(M, N, K)))
    return lib.qvit_gemm_wgrad(_p(G), M, N, ldg, _p(A), K, lda, _p(d), _p(dW), ldw, _p(ws), wsb, None)


GEMM_WGRAD = [
    (dict(G=None), ENULL), (dict(d=None, M=-1, wsb=1 << 20), ENULL), (dict(M=-1, wsb=1 << 20), EINVAL), (dict(ldw=60), EINVAL),
    (dict(ldg=50), EALIGN), (dict(lda=72), EALIGN), (dict(G=A0 + 8), EALIGN), (dict(A=A1 + 8), EALIGN),
    (dict(ws=A4 + 8), EALIGN), (dict(dW=A3 + 2), EALIGN), (dict(N=0, wsb=1 << 20, G=A0 + 8), EINVAL),
    (dict(wsb=64), EINVAL), (dict(wsb=64, G=A0 + 8), EALIGN),   # alignment is looked at before the workspace size
]


def bn_stats(lib, x=A0, B=2, C=3, H=4, W=4, eps=1e-5, rm=A1, rv=A2, mean=A3, var=A4, invstd=A5, ws=A6, wsb=None):
    if wsb is None:
        wsb = max(0, int(lib.qvit_bn_stats_workspace_bytes(B, C, H, W)))
    return lib.qvit_bn_stats(_p(x), B, C, H, W, eps, 0.1, _p(rm), _p(rv), _p(mean), _p(var), _p(invstd), _p(ws), wsb, None)


BN_STATS = [
    (dict(x=None), ENULL), (dict(ws=None, B=0), ENULL), (dict(B=0, wsb=1 << 20), EINVAL), (dict(eps=-1.0), EINVAL),
    (dict(wsb=8), EINVAL), (dict(x=A0 + 2), EALIGN), (dict(rm=A1 + 2), EALIGN), (dict(invstd=A5 + 1), EALIGN),
    (dict(ws=A6 + 4), EALIGN), (dict(wsb=8, x=A0 + 2), EINVAL), (dict(B=0, wsb=1 << 20, ws=A6 + 4), EINVAL),
]


def bn_forward(lib, x=A0, B=2, C=3, H=4, W=4, mean=A1, invstd=A2, gamma=A3, beta=A4, levels=15, pool=0, out=A5, flags=A6):
    return lib.qvit_bn_act_pool_forward(_p(x), B, C, H, W, _p(mean), _p(invstd), _p(gamma), _p(beta), levels, pool,
                                        _p(out), _p(flags), None)


BN_FORWARD = [
    (dict(x=None), ENULL), (dict(flags=None, pool=2), ENULL), (dict(pool=2), EINVAL), (dict(levels=0), EINVAL),
    (dict(levels=128), EINVAL), (dict(x=A0 + 2), EALIGN), (dict(gamma=A3 + 2), EALIGN), (dict(out=A5 + 1), EALIGN),
    (dict(levels=0, x=A0 + 2), EINVAL), (dict(pool=1, H=1, out=A5 + 1), EINVAL),
]


def bn_reduce(lib, x=A0, go=A1, flags=A2, B=2, C=3, H=4, W=4, mean=A3, invstd=A4, pool=0, sums=A5, ws=A6, wsb=None):
    if wsb is None:
        wsb = max(0, int(lib.qvit_bn_act_pool_backward_workspace_bytes(B, C, H, W, pool)))
    return lib.qvit_bn_act_pool_backward_reduce(_p(x), _p(go), _p(flags), B, C, H, W, _p(mean), _p(invstd), pool,
                                                _p(sums), _p(ws), wsb, None)


BN_REDUCE = [
    (dict(go=None), ENULL), (dict(sums=None, pool=2, wsb=64), ENULL), (dict(pool=2, wsb=64), EINVAL), (dict(wsb=8), EINVAL),
    (dict(x=A0 + 2), EALIGN), (dict(sums=A5 + 4), EALIGN), (dict(ws=A6 + 4), EALIGN), (dict(wsb=8, sums=A5 + 4), EINVAL),
]


def bn_dx(lib, x=A0, go=A1, flags=A2, B=2, C=3, H=4, W=4, mean=A3, invstd=A4, gamma=A5, sums=A6, pool=0, dx=A7,
          dgamma=A8, dbeta=A9):
    return lib.qvit_bn_act_pool_backward_dx(_p(x), _p(go), _p(flags), B, C, H, W, _p(mean), _p(invstd), _p(gamma),
                                            _p(sums), pool, _p(dx), _p(dgamma), _p(dbeta), None)


BN_DX = [
    (dict(dx=None), ENULL), (dict(sums=None, C=0), ENULL), (dict(C=0), EINVAL), (dict(go=A1 + 2), EALIGN),
    (dict(sums=A6 + 4), EALIGN), (dict(dbeta=A9 + 2), EALIGN), (dict(C=0, dx=A7 + 2), EINVAL),
]


# ---- the output quantizer of the int8 epilogues: enum and scalars only (the flag bits are not looked at) -------
def gemm_i8(lib, A=A0, M=16, K=128, lda=128, Wp=A1, wfmt=_lib.W4, N=16, npad=256, d_act=A2, d_wt=A3, bias=None,
            epi=_lib.EPI_I8, C=A4, ldc=16, qtype=LIN, d=A5, qm=A6, t=None, levels=0, table=None):
    return lib.qvit_gemm(_p(A), M, K, lda, _p(Wp), wfmt, N, npad, _p(d_act), _p(d_wt), _p(bias), epi, _p(C), ldc, qtype,
                         _p(d), _p(qm), _p(t), levels, _p(table), None)


# a valid quantizer reaches the next check (d_act, ENULL); a bad one stops at EINVAL
GEMM_I8 = [
    (dict(A=None), ENULL), (dict(K=100), EINVAL), (dict(lda=136), EALIGN), (dict(A=None, K=100, lda=136), ENULL),
    (dict(K=100, A=A0 + 8), EINVAL), (dict(C=A4 + 2), EALIGN), (dict(C=A4 + 2, qtype=7), EALIGN),
    (dict(qtype=7), EINVAL), (dict(qtype=7, d_act=None), EINVAL), (dict(d=None), EINVAL), (dict(qm=None, d_act=None), EINVAL),
    (dict(qtype=ULTRA, levels=0), EINVAL), (dict(qtype=ULTRA, levels=128, d_act=None), EINVAL),
    (dict(d_act=None), ENULL), (dict(qtype=CAREFUL, d_act=None), ENULL), (dict(qtype=STRAY | NONLIN, d_act=None), ENULL),
    (dict(qtype=ULTRA, d=None, qm=None, levels=127, d_act=None), ENULL),
    (dict(bias=A7 + 8), EALIGN), (dict(M=0), OK),
]


def gemm_resid_ln(lib, A=A0, M=16, K=128, lda=128, Wp=A1, wfmt=_lib.W4, N=64, npad=256, d_act=A2, d_wt=A3, bias=None,
                  C=A4, ldc=64, gamma=A5, beta=A6, qtype=LIN, d=A7, qm=A8, t=None, levels=0, table=None, codes=A9,
                  ldcodes=64, kpad=64, counters=0xB000):
    return lib.qvit_gemm_resid_ln(_p(A), M, K, lda, _p(Wp), wfmt, N, npad, _p(d_act), _p(d_wt), _p(bias), _p(C), ldc,
                                  _p(gamma), _p(beta), 1e-5, qtype, _p(d), _p(qm), _p(t), levels, _p(table), _p(codes),
                                  ldcodes, kpad, _p(counters), None)


GEMM_RESID_LN = [
    (dict(codes=None), ENULL), (dict(wfmt=_lib.W4R), EINVAL), (dict(N=66), EINVAL), (dict(A=A0 + 8), EALIGN),
    (dict(counters=0xB002), EALIGN), (dict(codes=None, N=66, A=A0 + 8), ENULL), (dict(N=66, A=A0 + 8), EINVAL),
    (dict(qtype=7, M=0), EINVAL), (dict(d=None, M=0), EINVAL), (dict(qtype=ULTRA, levels=0, M=0), EINVAL),
    (dict(qtype=ULTRA, levels=128, M=0), EINVAL), (dict(qtype=ULTRA, levels=15, d=None, qm=None, M=0), OK),
    (dict(qtype=CAREFUL, M=0), OK), (dict(qtype=7, gamma=A5 + 8, M=0), EALIGN),   # alignment before the quantizer
]


def epi_table(lib, epi=_lib.EPI_I8, qtype=LIN, d=A0, qm=A1, t=None, levels=0, v_lo=-1.0, w=0.01, nb=200, table=A2):
    return lib.qvit_epi_table_build(epi, qtype, _p(d), _p(qm), _p(t), levels, v_lo, w, nb, _p(table), None)


EPI_TABLE = [
    (dict(table=None), ENULL), (dict(table=None, nb=0), ENULL), (dict(epi=_lib.EPI_F32), EINVAL), (dict(nb=0), EINVAL),
    (dict(qtype=7), EINVAL), (dict(qm=None), EINVAL), (dict(qtype=ULTRA, levels=0), EINVAL),
    (dict(qtype=ULTRA, levels=128), EINVAL), (dict(table=A2 + 8), EALIGN), (dict(qtype=CAREFUL, table=A2 + 8), EALIGN),
    (dict(qtype=ULTRA, levels=127, d=None, qm=None, table=A2 + 8), EALIGN), (dict(qtype=7, table=A2 + 8), EINVAL),
    (dict(nb=0, table=A2 + 8), EINVAL),
]


def gemm_a32(lib, A=A0, M=64, K=768, Wp=A1, wfmt=_lib.W4, N=3072, npad=3072, d_act=A2, d_wt=A3, bias=None,
             epi=_lib.EPI_I8, C=A4, ldc=3072, qtype=LIN, d=A5, qm=A6, t=None, levels=0, table=None):
    return lib.qvit_gemm_a32(_p(A), M, K, _p(Wp), wfmt, N, npad, _p(d_act), _p(d_wt), _p(bias), epi, _p(C), ldc, qtype,
                             _p(d), _p(qm), _p(t), levels, _p(table), None)


GEMM_A32 = [
    (dict(d_wt=None), ENULL), (dict(d_wt=None, K=512), ENULL), (dict(K=512), EINVAL), (dict(ldc=3000), EINVAL),
    (dict(qtype=7), EINVAL), (dict(d=None), EINVAL), (dict(qtype=ULTRA, levels=0), EINVAL),
    (dict(qtype=ULTRA, levels=128), EINVAL), (dict(A=A0 + 8), EALIGN), (dict(ldc=3080), EALIGN), (dict(bias=A7 + 4), EALIGN),
    (dict(qtype=7, A=A0 + 8), EINVAL), (dict(qtype=CAREFUL, A=A0 + 8), EALIGN),
    (dict(qtype=ULTRA, levels=1, d=None, qm=None, C=A4 + 8), EALIGN), (dict(M=0), OK),
]


def attention(lib, qkv=A0, B=1, N=5, H=2, hd=64, ldq=384, in_scale=1.0, mode=1, out=A1, ldo=128, qtype=LIN, d=A2,
              qm=A3, t=None, levels=0):
    return lib.qvit_attention(_p(qkv), B, N, H, hd, ldq, 0.125, in_scale, mode, _p(out), ldo, qtype, _p(d), _p(qm),
                              _p(t), levels, None)


def attention_split(lib, hi=A0, lo=A4, B=1, N=5, H=2, hd=64, in_scale=1.0, mode=1, out=A1, ldo=128, qtype=LIN, d=A2,
                    qm=A3, t=None, levels=0, table=None):
    return lib.qvit_attention_split(_p(hi), _p(lo), B, N, H, hd, 0.125, in_scale, mode, _p(out), ldo, qtype, _p(d),
                                    _p(qm), _p(t), levels, _p(table), None)


ATT_COMMON = [
    (dict(out=None), ENULL), (dict(out=None, hd=32), ENULL), (dict(hd=32), EINVAL), (dict(ldo=64), EINVAL),
    (dict(mode=2, B=0), EINVAL), (dict(out=A1 + 2), EALIGN), (dict(ldo=130), EALIGN), (dict(out=A1 + 2, qtype=7), EALIGN),
    (dict(hd=32, out=A1 + 2), EINVAL),
    (dict(qtype=7, B=0), EINVAL), (dict(d=None, B=0), EINVAL), (dict(qtype=ULTRA, levels=0, B=0), EINVAL),
    (dict(qtype=ULTRA, levels=128, B=0), EINVAL), (dict(qtype=ULTRA, levels=15, d=None, qm=None, B=0), OK),
    (dict(qtype=CAREFUL | NONLIN, B=0), OK), (dict(out=A1 + 4, B=0), OK), (dict(mode=0, out=A1 + 4, B=0), EALIGN),
]
ATTENTION = ATT_COMMON + [(dict(qkv=A0 + 8), EALIGN), (dict(ldq=386), EALIGN), (dict(ldq=380, qkv=A0 + 8), EINVAL),
                          (dict(hd=80, ldq=480, ldo=160), EINVAL)]
ATTENTION_SPLIT = ATT_COMMON + [(dict(lo=A4 + 8), EALIGN), (dict(table=A5 + 8, hd=32), EALIGN)]


def qkv_attention(lib, fn="qvit_qkv_attention", nq=None, A=A0, B=1, N=5, K=256, lda=256, Wp=A1, wfmt=_lib.W4, npad=512,
                  d_act=A2, d_wt=A3, bias=None, H=2, hd=64, in_scale=1.0, mode=1, out=A4, ldo=128, qtype=LIN, d=A5,
                  qm=A6, t=None, levels=0, table=None):
    head = (_p(A), B, N) + (() if nq is None else (nq,))
    return getattr(lib, fn)(*head, K, lda, _p(Wp), wfmt, npad, _p(d_act), _p(d_wt), _p(bias), H, hd, 0.125, in_scale,
                            mode, _p(out), ldo, qtype, _p(d), _p(qm), _p(t), levels, _p(table), None)


def qkv_attention_q(lib, **kw):
    kw.setdefault("nq", 1)
    return qkv_attention(lib, fn="qvit_qkv_attention_q", **kw)


QKV_ATTENTION = [
    (dict(d_act=None), ENULL), (dict(d_act=None, K=100), ENULL), (dict(K=100), EINVAL), (dict(wfmt=_lib.W8), EINVAL),
    (dict(A=A0 + 8), EALIGN), (dict(table=A7 + 8), EALIGN), (dict(K=100, A=A0 + 8), EINVAL), (dict(out=A4 + 2), EALIGN),
    (dict(out=A4 + 2, qtype=7), EALIGN), (dict(mode=2, B=0), EINVAL),
    (dict(qtype=7, B=0), EINVAL), (dict(qm=None, B=0), EINVAL), (dict(qtype=ULTRA, levels=0, B=0), EINVAL),
    (dict(qtype=ULTRA, levels=128, B=0), EINVAL), (dict(qtype=ULTRA, levels=15, d=None, qm=None, B=0), OK),
    (dict(qtype=CAREFUL, B=0), OK),
]


# ---- entry points without a quantizer argument ------------------------------------------------------------------
def gemm_wonly(lib, X=A0, M=16, K=128, ldx=128, Wp=A1, wfmt=_lib.W4, N=16, npad=256, d_wt=A2, bias=None, Y=A3, ldy=16,
               ws=None, wsb=0):
    return lib.qvit_gemm_wonly(_p(X), M, K, ldx, _p(Wp), wfmt, N, npad, _p(d_wt), _p(bias), _p(Y), ldy, _p(ws), wsb,
                               None)


GEMM_WONLY = [
    (dict(X=None), ENULL), (dict(d_wt=None, K=100), ENULL), (dict(wfmt=5), EINVAL), (dict(K=100), EINVAL),
    (dict(ldy=8), EINVAL), (dict(ldx=130), EALIGN), (dict(ldy=18), EALIGN), (dict(K=100, X=A0 + 8), EINVAL),
    (dict(wfmt=5, Y=A3 + 8), EINVAL), (dict(M=0), OK), (dict(M=0, Y=A3 + 8), EALIGN),
]


def conv_wonly(lib, fused=False, X=A0, B=1, C=3, H=8, W=8, k=3, s=1, p=1, dil=1, Wp=A1, wfmt=_lib.W4, N=16, npad=256,
               K=128, d_wt=A2, bias=None, bn_a=A4, bn_s=A5, levels=15, Y=A3, kh=None, kw=None, sh=None, sw=None, ph=None,
               pw=None, dh=None, dw=None):
    """k, s, p, dil go to both axes; kh .. dw override one axis each."""
    head = (_p(X), B, C, H, W, _ax(kh, k), _ax(kw, k), _ax(sh, s), _ax(sw, s), _ax(ph, p), _ax(pw, p), _ax(dh, dil),
            _ax(dw, dil), _p(Wp), wfmt, N, npad, K, _p(d_wt), _p(bias))
    if fused:
        return lib.qvit_conv_wonly_bn_act(*head, _p(bn_a), _p(bn_s), levels, _p(Y), None)
    return lib.qvit_conv_wonly(*head, _p(Y), None, 0, None)


def conv_wonly_bn_act(lib, **kw):
    return conv_wonly(lib, fused=True, **kw)


CONV_WONLY = [
    (dict(Y=None), ENULL), (dict(X=None, s=0), ENULL), (dict(wfmt=5), EINVAL), (dict(s=0), EINVAL), (dict(K=100), EINVAL),
    (dict(H=1, W=1, p=0), EINVAL), (dict(s=0, Wp=A1 + 8), EINVAL), (dict(K=100, bias=A6 + 8), EINVAL), (dict(B=0), OK),
    (dict(B=0, Wp=A1 + 8), EALIGN),
    *[(geo, EINVAL) for geo in CONV_GEO_BAD],
    # a bad extent is looked at after the null pointers and before the alignment
    (dict(W=2, pw=0, sw=2, Wp=A1 + 8), EINVAL), (dict(W=2, pw=0, sw=2, Y=None), ENULL),
]
CONV_WONLY_BN_ACT = CONV_WONLY + [
    (dict(bn_a=None), ENULL), (dict(bn_s=None, levels=0), ENULL), (dict(bn_a=None, Wp=A1 + 8), EALIGN),
    (dict(bn_a=None, K=100), EINVAL), (dict(levels=0), EINVAL), (dict(levels=128), EINVAL), (dict(N=80), EINVAL),
    (dict(wfmt=_lib.W16), EINVAL),
]


def ultra_conv0(lib, img=A0, B=1, H=8, W=8, wvals=A1, alpha=A2, shift=A3, a_bit=4, out=A4):
    return lib.qvit_ultra_conv0(_p(img), B, H, W, _p(wvals), _p(alpha), _p(shift), a_bit, _p(out), None)


ULTRA_CONV0 = [
    (dict(img=None), ENULL), (dict(out=None, H=1), ENULL), (dict(H=1), EINVAL), (dict(a_bit=8), EINVAL),
    (dict(H=1, out=A4 + 8), EINVAL), (dict(B=0), OK), (dict(B=0, out=A4 + 8), EALIGN),
]


def ultra_conv(lib, x=A0, B=1, H=8, W=8, cin=16, ks=3, wcodes=A1, kpad=144, cout=32, w_bit=4, a_bit=4, alpha=A2,
               shift=A3, mode=_lib.ULTRA_CODES, out=A4, ldo=32):
    return lib.qvit_ultra_conv(_p(x), B, H, W, cin, ks, _p(wcodes), kpad, cout, w_bit, a_bit, _p(alpha), _p(shift),
                               mode, _p(out), ldo, None)


F32 = 2   # QVIT_ULTRA_F32
ULTRA_CONV = [
    (dict(shift=None), ENULL), (dict(x=None, w_bit=1), ENULL), (dict(w_bit=1), EINVAL), (dict(ldo=16), EINVAL),
    (dict(mode=5), EINVAL), (dict(alpha=None), ENULL), (dict(alpha=None, mode=5), EINVAL),
    (dict(alpha=None, mode=F32, B=0), OK), (dict(mode=_lib.ULTRA_CODES_POOL, H=7), EINVAL),
    (dict(kpad=150), EALIGN), (dict(ldo=34), EALIGN), (dict(cout=30), EALIGN), (dict(mode=F32, out=A4 + 2, B=0), OK),
    (dict(w_bit=1, x=A0 + 8), EINVAL), (dict(alpha=None, x=A0 + 8), ENULL),
    (dict(mode=_lib.ULTRA_CODES_POOL, H=7, x=A0 + 8), EINVAL), (dict(cin=5), EINVAL), (dict(B=0), OK),
    (dict(B=0, out=A4 + 2), EALIGN),
]


def ultra_conv0_int(lib, img=A0, B=1, H=8, W=8, wcodes=A1, inc=A2, bias=A3, shift_bits=8, out_bit=4, out=A4):
    return lib.qvit_ultra_conv0_int(_p(img), B, H, W, _p(wcodes), _p(inc), _p(bias), shift_bits, out_bit, _p(out), None)


ULTRA_CONV0_INT = [
    (dict(inc=None), ENULL), (dict(out=None, W=1), ENULL), (dict(W=1), EINVAL), (dict(shift_bits=41), EINVAL),
    (dict(out_bit=0, out=A4 + 8), EINVAL), (dict(B=0), OK), (dict(B=0, out=A4 + 8), EALIGN),
]


def ultra_conv_int(lib, x=A0, B=1, H=8, W=8, cin=16, ks=3, wcodes=A1, kpad=144, cout=32, inc=A2, bias=A3, shift_bits=8,
                   out_bit=4, pool=0, out=A4, ldo=32):
    return lib.qvit_ultra_conv_int(_p(x), B, H, W, cin, ks, _p(wcodes), kpad, cout, _p(inc), _p(bias), shift_bits,
                                   out_bit, pool, _p(out), ldo, None)


ULTRA_CONV_INT = [
    (dict(bias=None), ENULL), (dict(x=None, out_bit=8), ENULL), (dict(out_bit=8), EINVAL), (dict(pool=1, W=7), EINVAL),
    (dict(kpad=150), EALIGN), (dict(ldo=34), EALIGN), (dict(cout=30), EALIGN), (dict(pool=1, W=7, x=A0 + 8), EINVAL),
    (dict(out_bit=8, inc=A2 + 2), EINVAL), (dict(cin=64, ks=1), EINVAL), (dict(B=0), OK), (dict(B=0, inc=A2 + 2), EALIGN),
]


def ultra_tail(lib, x=A0, B=1, H=10, W=10, wl=(A1, A2, A3, A4), kpad=576, al=(A5, A5, A5, A5), sl=(A6, A6, A6, A6),
               table=True, hcodes=A7, hkpad=64, hbias=A8, hout=36, w_bit=4, a_bit=4, out=A9, ldo=36, anchors=None,
               na=0, no=0, stride=0.0, io=None, p=None):
    arr = lambda ps: (ctypes.c_void_p * 4)(*ps)   # host arrays of device pointers: the entry point reads these
    w, a, s = arr(wl), arr(al), arr(sl)
    wp, ap, sp = (ctypes.cast(v, ctypes.c_void_p) if table else None for v in (w, a, s))
    return lib.qvit_ultra_tail(_p(x), B, H, W, wp, kpad, ap, sp, _p(hcodes), hkpad, _p(hbias), hout, w_bit, a_bit,
                               _p(out), ldo, _p(anchors), na, no, stride, _p(io), _p(p), None)


DEC = dict(io=0xB000, p=0xC000, anchors=0xD000, na=3, no=12, stride=16.0)
ULTRA_TAIL = [
    (dict(x=None), ENULL), (dict(table=False), ENULL), (dict(out=None), ENULL), (dict(wl=(A1, A2, None, A4)), ENULL),
    (dict(sl=(A6, None, A6, A6), H=27), ENULL), (dict(H=27), EINVAL), (dict(kpad=500), EINVAL), (dict(hout=49), EINVAL),
    (dict(ldo=32), EINVAL), (dict(kpad=584), EALIGN), (dict(hkpad=72), EALIGN), (dict(wl=(A1, A2, A3, A4 + 8)), EALIGN),
    (dict(H=27, x=A0 + 8), EINVAL), (dict(w_bit=1, hcodes=A7 + 8), EINVAL),
    (dict(DEC, p=None), ENULL), (dict(DEC, stride=0.0), EINVAL), (dict(DEC, no=11), EINVAL),
    (dict(DEC, no=11, wl=(None, A2, A3, A4)), EINVAL), (dict(DEC, out=None, B=0), OK), (dict(B=0), OK),
    (dict(B=0, x=A0 + 8), EALIGN),
]


def attention_backward(lib, qkv=A0, out=A1, go=A2, B=1, N=5, H=2, hd=64, ldq=384, ldo=128, ldgo=128, in_scale=1.0,
                       gq=A3, ldg=384, ws=A4, wsb=None):
    if wsb is None:
        wsb = max(0, int(lib.qvit_attention_backward_workspace_bytes(B, N, H)))
    return lib.qvit_attention_backward(_p(qkv), _p(out), _p(go), B, N, H, hd, ldq, ldo, ldgo, 0.125, in_scale, 1.0,
                                       _p(gq), ldg, _p(ws), wsb, None)


ATTENTION_BACKWARD = [
    (dict(gq=None), ENULL), (dict(qkv=None, hd=32), ENULL), (dict(hd=32), EINVAL), (dict(ldq=380), EINVAL),
    (dict(in_scale=0.0), EINVAL), (dict(ldq=386), EALIGN), (dict(ldgo=130), EALIGN), (dict(hd=32, qkv=A0 + 8), EINVAL),
    (dict(ws=None), ENULL), (dict(ws=None, qkv=A0 + 8), EALIGN),   # the workspace is looked at last
    (dict(wsb=8), EINVAL), (dict(wsb=8, ws=A4 + 8), EINVAL), (dict(B=0), OK), (dict(B=0, ws=None), OK),
    (dict(B=0, go=A2 + 8), EALIGN),
]


def pack_w4r(lib, fn="qvit_pack_weight_w4r", packed=A0, npad=256, kpad=128, out=A1):
    return getattr(lib, fn)(_p(packed), npad, kpad, _p(out), None)


def pack_w8r(lib, **kw):
    return pack_w4r(lib, fn="qvit_pack_weight_w8r", **kw)


PACK_WR = [
    (dict(packed=None), ENULL), (dict(out=None, npad=100), ENULL), (dict(npad=100), EINVAL), (dict(kpad=65536 + 128), EINVAL),
    (dict(npad=100, out=A1 + 8), EINVAL), (dict(out=A0), EINVAL),          # not in place
    (dict(packed=A0 + 8, out=A0 + 8), EALIGN),                             # alignment is looked at before that
]


def gemm_qkv_split(lib, A=A0, M=10, K=128, lda=128, Wp=A1, wfmt=_lib.W4, N=64, npad=256, d_act=A2, d_wt=A3, bias=None,
                   seq=5, in_scale=1.0, hi=A4, lo=A5):
    return lib.qvit_gemm_qkv_split(_p(A), M, K, lda, _p(Wp), wfmt, N, npad, _p(d_act), _p(d_wt), _p(bias), seq, in_scale,
                                   _p(hi), _p(lo), None)


GEMM_QKV_SPLIT = [
    (dict(lo=None), ENULL), (dict(d_act=None, N=66), ENULL), (dict(wfmt=5), EINVAL), (dict(N=66), EINVAL),
    (dict(seq=3), EINVAL), (dict(in_scale=0.0), EINVAL), (dict(lda=136), EALIGN), (dict(seq=3, A=A0 + 8), EINVAL),
    (dict(N=66, hi=A4 + 8), EINVAL), (dict(M=0), OK), (dict(M=0, bias=A6 + 8), EALIGN),
]

TABLE = [
    (quantize_act, ROWS_TO_CODES), (gelu_quant, ROWS_TO_CODES), (fake_quant, FAKE_QUANT), (pack_weight, PACK_WEIGHT),
    (im2col, IM2COL), (ln_quant, LN_QUANT), (ln_quant_t32, LN_QUANT_T32),
    (quant_backward, STREAM_BACKWARD + QUANT_BACKWARD_ONLY), (gelu_quant_backward, STREAM_BACKWARD),
    (ln_quant_backward, LN_QUANT_BACKWARD), (wq_backward, WQ_BACKWARD), (act_backward, ACT_BACKWARD),
    (conv_wgrad, CONV_WGRAD), (gemm_wgrad, GEMM_WGRAD), (bn_stats, BN_STATS), (bn_forward, BN_FORWARD),
    (bn_reduce, BN_REDUCE), (bn_dx, BN_DX), (gemm_i8, GEMM_I8), (gemm_resid_ln, GEMM_RESID_LN), (epi_table, EPI_TABLE),
    (gemm_a32, GEMM_A32), (attention, ATTENTION), (attention_split, ATTENTION_SPLIT), (qkv_attention, QKV_ATTENTION),
    (qkv_attention_q, QKV_ATTENTION + [(dict(nq=0, d_act=None), EINVAL), (dict(nq=6), EINVAL)]),
    (gemm_wonly, GEMM_WONLY), (conv_wonly, CONV_WONLY), (conv_wonly_bn_act, CONV_WONLY_BN_ACT),
    (ultra_conv0, ULTRA_CONV0), (ultra_conv, ULTRA_CONV), (ultra_conv0_int, ULTRA_CONV0_INT),
    (ultra_conv_int, ULTRA_CONV_INT), (ultra_tail, ULTRA_TAIL), (attention_backward, ATTENTION_BACKWARD),
    (pack_w4r, PACK_WR), (pack_w8r, PACK_WR), (gemm_qkv_split, GEMM_QKV_SPLIT),
]
IDS = [c.__name__ for c, _ in TABLE]

# The size argument on which an entry point returns QVIT_OK before any launch (read from its source).
EARLY = {
    quantize_act: "rows", gelu_quant: "rows", fake_quant: "n", im2col: "B", ln_quant: "rows", ln_quant_t32: "rows",
    wq_backward: "n", act_backward: "n", gemm_i8: "M", gemm_resid_ln: "M", gemm_a32: "M", attention: "B",
    attention_split: "B", qkv_attention: "B", qkv_attention_q: "B", gemm_wonly: "M", conv_wonly: "B",
    conv_wonly_bn_act: "B", ultra_conv0: "B", ultra_conv: "B", ultra_conv0_int: "B", ultra_conv_int: "B",
    ultra_tail: "B", attention_backward: "B", gemm_qkv_split: "M",
}

# Every pointer argument with an alignment rule: {argument: (address in the valid call, required alignment)}.
# Off by half the alignment it must give QVIT_EALIGN, so a pointer dropped from a check is noticed.
ALIGNED = {
    quantize_act: dict(codes=(A3, 16)), gelu_quant: dict(codes=(A3, 16)), pack_weight: dict(packed=(A3, 16)),
    im2col: dict(codes=(A3, 16)), ln_quant: dict(table=(A6, 16), codes=(A5, 4)),
    ln_quant_t32: dict(x=(A0, 16), gamma=(A1, 16), beta=(A2, 16), codes=(A5, 16), table=(A6, 16)),
    quant_backward: dict(x=(A0, 16), g=(A1, 16), gx=(A4, 16), ws=(A6, 8)),
    gelu_quant_backward: dict(x=(A0, 16), g=(A1, 16), gx=(A4, 16), ws=(A6, 8)),
    ln_quant_backward: dict(x=(A0, 16), gamma=(A1, 16), beta=(A2, 16), gy=(A5, 16), gx=(A6, 16), ws=(A8, 16),
                            gg=(A9, 4), gb=(A9, 4)),
    wq_backward: dict(w=(A0, 4), g=(A1, 4), gw=(A2, 4), ws=(A3, 8)),
    act_backward: dict(x=(A0, 16), g=(A1, 16), gx=(A2, 16)),
    conv_wgrad: dict(G=(A0, 4), X=(A1, 4), dW=(A2, 4), ws=(A3, 16)),
    gemm_wgrad: dict(G=(A0, 16), A=(A1, 16), ws=(A4, 16), dW=(A3, 4)),
    bn_stats: dict(x=(A0, 4), rm=(A1, 4), rv=(A2, 4), mean=(A3, 4), var=(A4, 4), invstd=(A5, 4), ws=(A6, 8)),
    bn_forward: dict(x=(A0, 4), mean=(A1, 4), invstd=(A2, 4), gamma=(A3, 4), beta=(A4, 4), out=(A5, 4)),
    bn_reduce: dict(x=(A0, 4), go=(A1, 4), mean=(A3, 4), invstd=(A4, 4), sums=(A5, 8), ws=(A6, 8)),
    bn_dx: dict(x=(A0, 4), go=(A1, 4), mean=(A3, 4), invstd=(A4, 4), gamma=(A5, 4), sums=(A6, 8), dx=(A7, 4),
                dgamma=(A8, 4), dbeta=(A9, 4)),
    gemm_i8: dict(A=(A0, 16), Wp=(A1, 16), C=(A4, 4), bias=(A7, 16), table=(A8, 16)),
    gemm_resid_ln: dict(A=(A0, 16), Wp=(A1, 16), C=(A4, 16), codes=(A9, 4), counters=(0xB000, 4), bias=(0xC000, 16),
                        gamma=(A5, 16), beta=(A6, 16), table=(0xD000, 16)),
    epi_table: dict(table=(A2, 16)),
    gemm_a32: dict(A=(A0, 16), Wp=(A1, 16), C=(A4, 16), bias=(A7, 16), table=(A8, 16)),
    attention: dict(qkv=(A0, 16), out=(A1, 4)),
    attention_split: dict(hi=(A0, 16), lo=(A4, 16), out=(A1, 4), table=(A5, 16)),
    qkv_attention: dict(A=(A0, 16), Wp=(A1, 16), table=(A7, 16), out=(A4, 4)),
    qkv_attention_q: dict(A=(A0, 16), Wp=(A1, 16), table=(A7, 16), out=(A4, 4)),
    gemm_wonly: dict(X=(A0, 16), Wp=(A1, 16), Y=(A3, 16), bias=(A4, 16)),
    conv_wonly: dict(Wp=(A1, 16), bias=(A6, 16)), conv_wonly_bn_act: dict(Wp=(A1, 16), bias=(A6, 16)),
    ultra_conv0: dict(out=(A4, 16)), ultra_conv: dict(x=(A0, 16), wcodes=(A1, 16), out=(A4, 4)),
    ultra_conv0_int: dict(out=(A4, 16)),
    ultra_conv_int: dict(x=(A0, 16), wcodes=(A1, 16), out=(A4, 4), inc=(A2, 4), bias=(A3, 4)),
    ultra_tail: dict(x=(A0, 16), hcodes=(A7, 16)),
    attention_backward: dict(qkv=(A0, 16), out=(A1, 16), go=(A2, 16), gq=(A3, 16), ws=(A4, 16)),
    pack_w4r: dict(packed=(A0, 16), out=(A1, 16)), pack_w8r: dict(packed=(A0, 16), out=(A1, 16)),
    gemm_qkv_split: dict(A=(A0, 16), Wp=(A1, 16), hi=(A4, 16), lo=(A5, 16), bias=(A6, 16)),
}


@pytest.mark.parametrize("call,rows", TABLE, ids=IDS)
def test_rejection_table(lib, call, rows):
    got = [(kw, call(lib, **kw)) for kw, _ in rows]
    wrong = [(kw, status, want) for (kw, status), (_, want) in zip(got, rows) if status != want]
    assert not wrong, "\n".join(f"{call.__name__}({kw}) returned {s}, expected {w}" for kw, s, w in wrong)


@pytest.mark.parametrize("call", list(ALIGNED), ids=[c.__name__ for c in ALIGNED])
def test_every_aligned_pointer_is_checked(lib, call):
    for arg, (addr, align) in ALIGNED[call].items():   # (only the misaligned call is made: the aligned one would launch)
        assert call(lib, **{arg: addr + align // 2}) == EALIGN, (call.__name__, arg, align)


def test_conv_wgrad_workspace_query_rejects_the_same_geometries(lib):
    assert int(lib.qvit_conv_wgrad_workspace_bytes(*conv_wgrad_geo())) > 0
    for geo in CONV_GEO_BAD:
        assert int(lib.qvit_conv_wgrad_workspace_bytes(*conv_wgrad_geo(**geo))) < 0, geo


def test_every_row_is_answered_before_a_launch():
    """A row is a rejection, or it zeroes the size on which its entry point returns before the launch."""
    for call, rows in TABLE:
        for kw, want in rows:
            assert want in (EINVAL, EALIGN, ENULL) or (want == OK and kw.get(EARLY[call]) == 0), (call.__name__, kw)
