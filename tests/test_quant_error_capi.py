"""C ABI of qvit_quant_error and its workspace query: exported symbols, documented signatures, every rejection and
the order of the host checks (include/qvit_hip.h), pinned the way tests/test_capi_rejections.py pins the other entry
points. Every call is answered by the host checks alone: nothing is dereferenced and nothing is launched, so this
runs without a GPU. The rows that expect QVIT_OK have rows * cols == 0 under accumulate, which returns before any
launch."""
import ctypes
import re
from pathlib import Path

import pytest

from quantized_vit_amd import _lib, build

OK, EINVAL, EALIGN, ENULL = 0, -1, -2, -3
X0, D0, QM0, T0, ERR0, NCLIP0, WS0 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000
LIN, NONLIN, ULTRA = _lib.QT_LINEAR, _lib.QT_NONLINEAR, _lib.QT_ULTRA_ACT


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)   # never dereferenced


def call(lib, x=X0, rows=4, cols=8, ldx=8, qtype=LIN, d=D0, q_m=QM0, t=None, ncand=2, accumulate=0, err=ERR0,
         nclip=NCLIP0, ws=WS0, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 24   # ample for every size below
    return lib.qvit_quant_error(_p(x), rows, cols, ldx, qtype, _p(d), _p(q_m), _p(t), ncand, accumulate, _p(err),
                                _p(nclip), _p(ws), ws_bytes, None)


def test_symbols_and_signatures(lib):
    """Fails without the feature: the symbols do not exist."""
    header = (Path(build.INCLUDE) / "qvit_hip.h").read_text()
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    for name, ret, restype in (("qvit_quant_error", "int", ctypes.c_int),
                               ("qvit_quant_error_workspace_bytes", "int64_t", ctypes.c_int64)):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.search(r"\b%s\s+%s\(([^;]*)\);" % (ret, name), header)
        assert m, name
        args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(1).replace("\n", " ").split(",")]
        want = [ctypes.c_void_p if ("*" in a or a.startswith("hipStream_t")) else ctype[a.split()[0]] for a in args]
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want, name
        assert fn.restype is restype
    assert "quant_error.hip" in build.SOURCES


ROWS = [
    # NULL scalars, outputs and workspace first, in front of everything else
    (dict(d=None), ENULL), (dict(q_m=None), ENULL), (dict(err=None), ENULL), (dict(nclip=None), ENULL),
    (dict(ws=None), ENULL), (dict(d=None, qtype=7), ENULL), (dict(err=None, ncand=0), ENULL),
    (dict(ws=None, x=X0 + 2), ENULL),
    # the qtype: unknown enum, stray flag bits, the UltraNet quantizer (no d, no q_m to search)
    (dict(qtype=7), EINVAL), (dict(qtype=ULTRA), EINVAL), (dict(qtype=LIN | 0x200), EINVAL),
    (dict(qtype=7, ncand=0, x=X0 + 2), EINVAL), (dict(qtype=7, t=None), EINVAL),
    (dict(qtype=LIN | _lib.QT_FORCE_CAREFUL, rows=0, accumulate=1), OK),
    # the t rule: in front of the sizes
    (dict(qtype=NONLIN, t=None), ENULL), (dict(qtype=NONLIN, t=None, ncand=0), ENULL),
    (dict(qtype=NONLIN, t=None, ldx=4), ENULL), (dict(qtype=NONLIN, t=T0, rows=0, accumulate=1), OK),
    (dict(qtype=LIN, t=T0, rows=0, accumulate=1), OK),
    # the sizes
    (dict(ncand=0), EINVAL), (dict(ncand=65), EINVAL), (dict(ncand=-1), EINVAL), (dict(rows=-1), EINVAL),
    (dict(cols=-1, ldx=8), EINVAL), (dict(ldx=7), EINVAL), (dict(rows=1 << 40, cols=1, ldx=1 << 20), EINVAL),
    (dict(ncand=64, rows=0, accumulate=1), OK), (dict(ncand=1, cols=0, accumulate=1), OK),
    (dict(ncand=65, ws_bytes=0), EINVAL), (dict(ldx=7, err=ERR0 + 4), EINVAL), (dict(ncand=0, x=None), EINVAL),
    # a short workspace: behind the sizes, in front of a NULL x and of alignment
    (dict(ws_bytes=0), EINVAL), (dict(ws_bytes=31), EINVAL), (dict(ws_bytes=32, x=None), ENULL),
    (dict(ws_bytes=31, x=None), EINVAL), (dict(ws_bytes=31, err=ERR0 + 4), EINVAL),
    (dict(rows=0, ncand=3, ws_bytes=47, accumulate=1), EINVAL), (dict(rows=0, ncand=3, ws_bytes=48, accumulate=1), OK),
    # x may be NULL only for an empty tensor
    (dict(x=None), ENULL), (dict(x=None, rows=0, accumulate=1), OK), (dict(x=None, cols=0, accumulate=1), OK),
    (dict(x=None, err=ERR0 + 4), ENULL),
    # alignment last: each pointer in turn
    (dict(x=X0 + 2), EALIGN), (dict(d=D0 + 1), EALIGN), (dict(q_m=QM0 + 2), EALIGN),
    (dict(qtype=NONLIN, t=T0 + 2), EALIGN), (dict(err=ERR0 + 4), EALIGN), (dict(nclip=NCLIP0 + 4), EALIGN),
    (dict(ws=WS0 + 4), EALIGN), (dict(x=X0 + 2, rows=0, accumulate=1), EALIGN),
    (dict(x=X0 + 4, d=D0 + 4, q_m=QM0 + 4, rows=0, accumulate=1), OK),   # 4 bytes is all x, d, q_m need
]


def test_rejection_table(lib):
    got = [(kw, call(lib, **kw)) for kw, _ in ROWS]
    wrong = [(kw, status, want) for (kw, status), (_, want) in zip(got, ROWS) if status != want]
    assert not wrong, "\n".join(f"qvit_quant_error({kw}) returned {s}, expected {w}" for kw, s, w in wrong)


def test_every_row_is_answered_before_a_launch():
    for kw, want in ROWS:
        empty = kw.get("rows", 4) == 0 or kw.get("cols", 8) == 0
        assert want in (EINVAL, EALIGN, ENULL) or (want == OK and empty and kw.get("accumulate") == 1), kw


def test_workspace_query(lib):
    q = lib.qvit_quant_error_workspace_bytes
    # 16 bytes per workgroup and candidate; a workgroup per 256 threads of 4 elements, at most 1024 of them
    assert q(4, 8, 2) == 32 and q(0, 8, 3) == 48 and q(8, 0, 1) == 16
    assert q(1, 8192, 1) == 8 * 16 and q(1, 8193, 1) == 8 * 16 and q(3, 8197, 17) == 25 * 16 * 17
    assert q(50432, 3072, 32) == 1024 * 16 * 32 and q(1 << 20, 1 << 20, 64) == 1024 * 16 * 64
    for bad in ((4, 8, 0), (4, 8, 65), (-1, 8, 2), (4, -1, 2), (1 << 30, 1 << 30, 2)):
        assert q(*bad) == EINVAL, bad
    # the entry point asks for exactly the query's size
    assert call(lib, rows=3, cols=8197, ldx=8197, ncand=17, ws_bytes=25 * 16 * 17 - 1) == EINVAL
    assert call(lib, rows=3, cols=8197, ldx=8197, ncand=17, ws_bytes=25 * 16 * 17, x=None) == ENULL
