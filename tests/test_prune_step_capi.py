"""C ABI of the qvit_prune_* entry points: exported symbols, documented signatures, every rejection in the order
include/qvit_hip.h documents, null and misaligned tables included. Every call is answered by the host checks alone
(the rows that expect QVIT_OK have a count of zero), so this runs without a GPU."""
import ctypes
import re
from pathlib import Path

import pytest

from quantized_vit_amd import _lib, build

OK, EINVAL, EALIGN, ENULL = 0, -1, -2, -3
G0, M0, I0, O0, X0 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
HYPER = (0, 1e-2, 1e-3, 0.9, 0.999, 0.1, 0.001, 0.0, 0.1, 0.001, -1.0, 1.0)   # first_step .. clip_hi
NAMES = ("qvit_prune_scores", "qvit_prune_scores_finish", "qvit_prune_joint_scalars", "qvit_prune_joint_reduce",
         "qvit_prune_joint_finish", "qvit_prune_joint_apply")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)   # never dereferenced


def stream(name):
    def call(lib, groups=G0, ngroups=0, members=M0, nmembers=0, items=I0, nitems=0, out=O0, variant=_lib.QAT_ADAMW):
        return getattr(lib, name)(_p(groups), ngroups, _p(members), nmembers, _p(items), nitems, _p(out), variant,
                                  *HYPER, None)
    call.__name__ = name
    return call


def scores_finish(lib, groups=G0, ngroups=0, items=I0, nitems=0, sums=O0, scores=X0):
    return lib.qvit_prune_scores_finish(_p(groups), ngroups, _p(items), nitems, _p(sums), .2, .2, .2, .2, .2,
                                        _p(scores), None)


def joint_scalars(lib, quants=G0, nquants=0, variant=_lib.QAT_ADAMW, bits=(4, 16)):
    return lib.qvit_prune_joint_scalars(_p(quants), nquants, variant, *HYPER, *bits, None)


def joint_finish(lib, groups=G0, ngroups=0, partials=O0, npartials=0, period=3, t=1, bits=(4, 16), gamma=X0,
                 info=X0 + 64):
    return lib.qvit_prune_joint_finish(_p(groups), ngroups, _p(partials), npartials, 1e-2, period, t, *bits,
                                       _p(gamma), _p(info), None)


STREAM_ROWS = [
    (dict(groups=None), ENULL), (dict(members=None), ENULL), (dict(items=None), ENULL), (dict(out=None), ENULL),
    (dict(groups=None, members=M0 + 4), ENULL), (dict(out=None, ngroups=-1), ENULL),
    (dict(items=None, variant=9), ENULL),
    (dict(groups=G0 + 4), EALIGN), (dict(members=M0 + 4), EALIGN), (dict(items=I0 + 4), EALIGN),
    (dict(out=O0 + 4), EALIGN), (dict(items=I0 + 2, nitems=-1), EALIGN), (dict(groups=G0 + 4, variant=9), EALIGN),
    (dict(ngroups=-1), EINVAL), (dict(nmembers=-1), EINVAL), (dict(nitems=-1), EINVAL), (dict(nitems=1 << 31), EINVAL),
    (dict(ngroups=-1, variant=9), EINVAL),
    (dict(variant=3), EINVAL), (dict(variant=-1), EINVAL), (dict(variant=9, ngroups=4, nmembers=4), EINVAL),
    (dict(), OK), (dict(variant=_lib.QAT_SGD), OK), (dict(variant=_lib.QAT_ADAM), OK),
    (dict(ngroups=3, nmembers=6, nitems=0), OK), (dict(ngroups=0, nmembers=6, nitems=9), OK),
    (dict(ngroups=3, nmembers=0, nitems=9), OK), (dict(groups=G0 + 8, out=O0 + 8), OK),
]
SCORES_FINISH_ROWS = [
    (dict(groups=None), ENULL), (dict(items=None), ENULL), (dict(sums=None), ENULL), (dict(scores=None), ENULL),
    (dict(sums=None, scores=X0 + 2), ENULL), (dict(scores=None, ngroups=-1), ENULL),
    (dict(groups=G0 + 4), EALIGN), (dict(items=I0 + 4), EALIGN), (dict(sums=O0 + 4), EALIGN),
    (dict(scores=X0 + 2), EALIGN), (dict(scores=X0 + 2, nitems=-1), EALIGN), (dict(scores=X0 + 4), OK),
    (dict(ngroups=-1), EINVAL), (dict(nitems=-1), EINVAL), (dict(nitems=1 << 31), EINVAL),
    (dict(), OK), (dict(ngroups=2), OK), (dict(nitems=5), OK),
]
JOINT_SCALARS_ROWS = [
    (dict(quants=None), ENULL), (dict(quants=None, nquants=-1), ENULL), (dict(quants=None, variant=9), ENULL),
    (dict(quants=G0 + 4), EALIGN), (dict(quants=G0 + 4, nquants=-1), EALIGN),
    (dict(nquants=-1), EINVAL), (dict(nquants=-1, variant=9), EINVAL),
    (dict(variant=3), EINVAL), (dict(variant=3, bits=(1, 16)), EINVAL),
    (dict(bits=(1, 16)), EINVAL), (dict(bits=(8, 7)), EINVAL), (dict(bits=(4, 33)), EINVAL),
    (dict(), OK), (dict(bits=(2, 32)), OK), (dict(variant=_lib.QAT_SGD), OK),
]
JOINT_FINISH_ROWS = [
    (dict(groups=None), ENULL), (dict(partials=None), ENULL), (dict(gamma=None), ENULL), (dict(info=None), ENULL),
    (dict(gamma=None, info=X0 + 2), ENULL), (dict(info=None, ngroups=-1), ENULL),
    (dict(groups=G0 + 4), EALIGN), (dict(partials=O0 + 4), EALIGN), (dict(gamma=X0 + 2), EALIGN),
    (dict(info=X0 + 2), EALIGN), (dict(gamma=X0 + 2, period=0), EALIGN), (dict(gamma=X0 + 4), OK),
    (dict(ngroups=-1), EINVAL), (dict(npartials=-1), EINVAL), (dict(npartials=1 << 31), EINVAL),
    (dict(ngroups=-1, period=0), EINVAL),
    (dict(period=0), EINVAL), (dict(t=-1), EINVAL), (dict(t=3), EINVAL), (dict(period=0, bits=(1, 16)), EINVAL),
    (dict(bits=(1, 16)), EINVAL), (dict(bits=(8, 7)), EINVAL), (dict(bits=(4, 33)), EINVAL),
    (dict(), OK), (dict(period=1, t=0), OK), (dict(npartials=7), OK),
]
TABLES = [(stream("qvit_prune_scores"), STREAM_ROWS), (stream("qvit_prune_joint_reduce"), STREAM_ROWS),
          (stream("qvit_prune_joint_apply"), STREAM_ROWS), (scores_finish, SCORES_FINISH_ROWS),
          (joint_scalars, JOINT_SCALARS_ROWS), (joint_finish, JOINT_FINISH_ROWS)]


def test_symbols_and_signatures(lib):
    """Fails without the feature: the symbols do not exist."""
    header = (Path(build.INCLUDE) / "qvit_hip.h").read_text()
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        want = [ctypes.c_void_p if ("*" in a or a.startswith("hipStream_t")) else ctype[a.split()[0]] for a in args]
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want, name
        assert fn.restype is ctypes.c_int
    assert "prune_step.hip" in build.SOURCES and "qat_common.h" in build.HEADERS
    for name in NAMES:
        assert name in header.split("*/")[0], f"{name} is missing from the header comment's list"


@pytest.mark.parametrize("fn,rows", TABLES, ids=[t[0].__name__ for t in TABLES])
def test_rejection_table(lib, fn, rows):
    got = [(kw, fn(lib, **kw)) for kw, _ in rows]
    wrong = [(kw, status, want) for (kw, status), (_, want) in zip(got, rows) if status != want]
    assert not wrong, "\n".join(f"{fn.__name__}({kw}) returned {s}, expected {w}" for kw, s, w in wrong)


def test_every_accepted_row_returns_before_a_launch():
    for kw, want in STREAM_ROWS:
        assert want != OK or not (kw.get("ngroups", 0) and kw.get("nmembers", 0) and kw.get("nitems", 0)), kw
    for kw, want in SCORES_FINISH_ROWS:
        assert want != OK or not (kw.get("ngroups", 0) and kw.get("nitems", 0)), kw
    for kw, want in JOINT_SCALARS_ROWS:
        assert want != OK or kw.get("nquants", 0) == 0, kw
    for kw, want in JOINT_FINISH_ROWS:
        assert want != OK or kw.get("ngroups", 0) == 0, kw


def test_table_layouts_match_the_python_side():
    header = (Path(build.INCLUDE) / "qvit_hip.h").read_text()
    assert f"ngroups descriptors of {_lib.PRUNE_GROUP_BYTES} bytes" in header
    assert f"nmembers descriptors of {_lib.PRUNE_MEMBER_BYTES} bytes" in header
    assert f"nitems entries of {_lib.PRUNE_ITEM_BYTES} bytes" in header
    assert (_lib.PRUNE_IMPORTANT, _lib.PRUNE_REDUNDANT, _lib.PRUNE_PRUNED) == (0, 1, 2)
    assert "state 0 important, 1 active" in header
