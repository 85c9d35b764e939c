"""C ABI of qvit_prune_scores_fold: the exported symbol, the documented signature and every rejection in the order
include/qvit_hip.h documents (a table, sums or unit_sums NULL; any of the five off 8 bytes; a count below 0, nitems or
nunits above 2^31 - 1; ngroups or nunits zero is a no-op success), with mixed errors that pin the order. Every call is
answered by the host checks alone (the rows that expect QVIT_OK have a count of zero), so this runs without a GPU, in
the manner of tests/test_prune_step_capi.py."""
import ctypes
import re
from pathlib import Path

import pytest

from quantized_vit_amd import _lib, build

OK, EINVAL, EALIGN, ENULL = 0, -1, -2, -3
G0, I0, S0, U0, O0 = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
NAME = "qvit_prune_scores_fold"


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)   # never dereferenced


def fold(lib, groups=G0, ngroups=0, items=I0, nitems=0, sums=S0, units=U0, nunits=0, out=O0):
    return lib.qvit_prune_scores_fold(_p(groups), ngroups, _p(items), nitems, _p(sums), _p(units), nunits, _p(out),
                                      None)


ROWS = [
    # NULL first, whatever else is wrong
    (dict(groups=None), ENULL), (dict(items=None), ENULL), (dict(sums=None), ENULL), (dict(units=None), ENULL),
    (dict(out=None), ENULL),
    (dict(groups=None, items=I0 + 4), ENULL), (dict(out=None, ngroups=-1), ENULL),
    (dict(units=None, nunits=1 << 31), ENULL), (dict(sums=None, out=O0 + 2, nitems=-1), ENULL),
    # then alignment, before the counts
    (dict(groups=G0 + 4), EALIGN), (dict(items=I0 + 4), EALIGN), (dict(sums=S0 + 4), EALIGN),
    (dict(units=U0 + 4), EALIGN), (dict(out=O0 + 4), EALIGN), (dict(out=O0 + 1), EALIGN),
    (dict(items=I0 + 2, nitems=-1), EALIGN), (dict(units=U0 + 4, nunits=1 << 31), EALIGN),
    (dict(groups=G0 + 4, ngroups=-1), EALIGN),
    # then the counts
    (dict(ngroups=-1), EINVAL), (dict(nitems=-1), EINVAL), (dict(nunits=-1), EINVAL),
    (dict(nitems=1 << 31), EINVAL), (dict(nunits=1 << 31), EINVAL),
    (dict(ngroups=-1, nunits=0), EINVAL), (dict(ngroups=0, nunits=-1), EINVAL),
    (dict(ngroups=3, nitems=-1, nunits=0), EINVAL),
    # a zero count is a no-op success
    (dict(), OK), (dict(ngroups=3, nitems=9, nunits=0), OK), (dict(ngroups=0, nitems=9, nunits=4), OK),
    (dict(ngroups=0, nitems=(1 << 31) - 1, nunits=(1 << 31) - 1), OK), (dict(groups=G0 + 8, out=O0 + 8), OK),
]


def test_symbol_and_signature(lib):
    header = (Path(build.INCLUDE) / "qvit_hip.h").read_text()
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}
    assert NAME in _lib.EXPORTED_SYMBOLS and hasattr(lib, NAME)
    m = re.search(r"\bint\s+%s\(([^;]*)\);" % NAME, header)
    assert m
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    want = [ctypes.c_void_p if ("*" in a or a.startswith("hipStream_t")) else ctype[a.split()[0]] for a in args]
    fn = getattr(lib, NAME)
    assert list(fn.argtypes) == want and fn.restype is ctypes.c_int
    assert NAME in header.split("*/")[0], "missing from the header comment's list"
    assert "scores_fold: a table, sums or unit_sums NULL; any of the five off 8" in header


def test_rejection_table(lib):
    got = [(kw, fold(lib, **kw)) for kw, _ in ROWS]
    wrong = [(kw, status, want) for (kw, status), (_, want) in zip(got, ROWS) if status != want]
    assert not wrong, "\n".join(f"{NAME}({kw}) returned {s}, expected {w}" for kw, s, w in wrong)


def test_every_accepted_row_returns_before_a_launch():
    for kw, want in ROWS:
        assert want != OK or not (kw.get("ngroups", 0) and kw.get("nunits", 0)), kw
