"""C ABI of qvit_im2col_u8_i8 and qvit_u8_normalize_f32: exported symbols, documented signatures, the layout
constants, and the order of the host checks (include/qvit_hip.h), pinned the way tests/test_capi_rejections.py pins
the other entry points. Every call is answered by the host checks alone: nothing is dereferenced and nothing is
launched, so this runs without a GPU. A row is (overrides of a valid call, status); the rows that expect QVIT_OK have
B = 0, which returns before any launch."""
import ctypes
import re
from pathlib import Path

import pytest

from quantized_vit_amd import _lib, build
from test_capi_rejections import CONV_GEO_BAD, _ax

OK, EINVAL, EALIGN, ENULL = 0, -1, -2, -3
IMG0, TAB0, OUT0 = 0x1000, 0x2000, 0x3000
NAMES = ("qvit_im2col_u8_i8", "qvit_u8_normalize_f32")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)   # never dereferenced


def im2col(lib, img=IMG0, B=1, C=3, H=8, W=8, layout=0, k=3, s=1, p=1, dil=1, table=TAB0, codes=OUT0, ldc=32,
           kpad=32, kh=None, kw=None, sh=None, sw=None, ph=None, pw=None, dh=None, dw=None):
    """k, s, p, dil go to both axes; kh .. dw override one axis each."""
    return lib.qvit_im2col_u8_i8(_p(img), B, C, H, W, layout, _ax(kh, k), _ax(kw, k), _ax(sh, s), _ax(sw, s),
                                 _ax(ph, p), _ax(pw, p), _ax(dh, dil), _ax(dw, dil), _p(table), _p(codes), ldc, kpad,
                                 None)


def normalize(lib, img=IMG0, B=1, C=3, H=8, W=8, layout=0, table=TAB0, out=OUT0):
    return lib.qvit_u8_normalize_f32(_p(img), B, C, H, W, layout, _p(table), _p(out), None)


def test_symbols_signatures_and_constants(lib):
    """Fails without the feature: the symbols do not exist."""
    header = (Path(build.INCLUDE) / "qvit_hip.h").read_text()
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(1).replace("\n", " ").split(",")]
        want = [ctypes.c_void_p if ("*" in a or a.startswith("hipStream_t")) else ctype[a.split()[0]] for a in args]
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want, name
        assert fn.restype is ctypes.c_int
    consts = dict(re.findall(r"#define\s+(QVIT_\w+)\s+(-?\d+)", header))
    assert int(consts["QVIT_U8_NCHW"]) == _lib.U8_NCHW == 0 and int(consts["QVIT_U8_NHWC"]) == _lib.U8_NHWC == 1


IM2COL = [
    # NULL pointers first, in front of everything else
    (dict(img=None), ENULL), (dict(table=None), ENULL), (dict(codes=None), ENULL),
    (dict(img=None, layout=2), ENULL), (dict(table=None, s=0), ENULL), (dict(codes=None, C=17), ENULL),
    # the layout, in front of the geometry
    (dict(layout=2), EINVAL), (dict(layout=-1), EINVAL), (dict(layout=2, codes=OUT0 + 4), EINVAL),
    (dict(layout=1, B=0), OK), (dict(layout=0, B=0), OK),
    # the geometry
    *[(g, EINVAL) for g in CONV_GEO_BAD],
    (dict(W=2, pw=0, sw=2, codes=OUT0 + 4), EINVAL), (dict(W=2, pw=0, sw=2, img=None), ENULL),
    (dict(B=-1), EINVAL), (dict(C=0), EINVAL), (dict(H=0), EINVAL), (dict(H=1, W=1, p=0), EINVAL),
    # the channel bound, after the geometry and in front of kpad / ldc
    (dict(C=17, kpad=160, ldc=160), EINVAL), (dict(C=17, kpad=160, ldc=160, B=0), EINVAL),
    (dict(C=16, kpad=144, ldc=144, B=0), OK), (dict(C=17, kpad=160, ldc=168), EINVAL),
    # kpad and ldc sizes (EINVAL), in front of alignment (EALIGN)
    (dict(kpad=16), EINVAL), (dict(kpad=40, ldc=48), EINVAL), (dict(ldc=16), EINVAL),
    (dict(kpad=16, codes=OUT0 + 4), EINVAL), (dict(kpad=16, ldc=40), EINVAL),
    (dict(ldc=40), EALIGN), (dict(codes=OUT0 + 4), EALIGN), (dict(codes=OUT0 + 8, B=0), EALIGN),
    # the image and the table may sit at any address
    (dict(img=IMG0 + 1, table=TAB0 + 3, B=0), OK), (dict(img=IMG0 + 4, layout=1, B=0), OK),
    # each argument reaches its own axis: valid as given, no output with the pair swapped
    (dict(B=0, H=3, W=19, kh=1, kw=7, p=0), OK), (dict(H=3, W=19, kh=7, kw=1, p=0), EINVAL),
    (dict(B=0, C=1, H=3, W=19, k=5, ph=1, pw=0), OK), (dict(C=1, H=3, W=19, k=5, ph=0, pw=1), EINVAL),
]

NORMALIZE = [
    (dict(img=None), ENULL), (dict(table=None), ENULL), (dict(out=None), ENULL), (dict(out=None, layout=2), ENULL),
    (dict(layout=2), EINVAL), (dict(B=-1), EINVAL), (dict(C=0), EINVAL), (dict(H=0), EINVAL), (dict(W=0), EINVAL),
    (dict(C=17), EINVAL), (dict(C=17, B=0), EINVAL), (dict(B=(1 << 20) + 1), EINVAL), (dict(W=(1 << 20) + 1), EINVAL),
    (dict(layout=2, out=OUT0 + 2), EINVAL), (dict(C=17, table=TAB0 + 2), EINVAL),
    (dict(out=OUT0 + 2), EALIGN), (dict(table=TAB0 + 1), EALIGN), (dict(out=OUT0 + 2, B=0), EALIGN),
    (dict(B=0), OK), (dict(B=0, layout=1, C=16), OK), (dict(B=0, img=IMG0 + 1, out=OUT0 + 4), OK),
]
TABLE = [(im2col, IM2COL), (normalize, NORMALIZE)]


@pytest.mark.parametrize("call,rows", TABLE, ids=[c.__name__ for c, _ in TABLE])
def test_rejection_table(lib, call, rows):
    got = [(kw, call(lib, **kw)) for kw, _ in rows]
    wrong = [(kw, status, want) for (kw, status), (_, want) in zip(got, rows) if status != want]
    assert not wrong, "\n".join(f"{call.__name__}({kw}) returned {s}, expected {w}" for kw, s, w in wrong)


def test_every_row_is_answered_before_a_launch():
    for _, rows in TABLE:
        for kw, want in rows:
            assert want in (EINVAL, EALIGN, ENULL) or (want == OK and kw.get("B") == 0), kw
