"""C ABI of qvit_qat_step and qvit_qat_quant_step: exported symbols, documented signatures, every rejection and the
order of the host checks (include/qvit_hip.h), pinned the way tests/test_capi_rejections.py pins the other entry
points. Every call is answered by the host checks alone: nothing is dereferenced and nothing is launched, so this
runs without a GPU. The rows that expect QVIT_OK have a count of zero, which returns before any launch."""
import ctypes
import re
from pathlib import Path

import pytest

from quantized_vit_amd import _lib, build

OK, EINVAL, EALIGN, ENULL = 0, -1, -2, -3
T0, C0, Q0, B0 = 0x1000, 0x2000, 0x3000, 0x4000
HYPER = (0, 1e-2, 1e-3, 0.9, 0.999, 0.1, 0.001, 0.0, 0.1, 0.001, -1.0, 1.0)   # first_step .. clip_hi


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _p(v):
    return None if v is None else ctypes.c_void_p(v)   # never dereferenced


def dense(lib, tensors=T0, ntensors=0, chunks=C0, nchunks=0, variant=_lib.QAT_ADAMW):
    return lib.qvit_qat_step(_p(tensors), ntensors, _p(chunks), nchunks, variant, *HYPER, None)


def quant(lib, quants=Q0, nquants=0, bits=B0, stage=_lib.QAT_RANGE, first_fix=0, variant=_lib.QAT_ADAMW,
          ranges=(4, 16, 4, 16)):
    return lib.qvit_qat_quant_step(_p(quants), nquants, _p(bits), stage, first_fix, variant, *HYPER, *ranges, None)


def test_symbols_and_signatures(lib):
    """Fails without the feature: the symbols do not exist."""
    header = (Path(build.INCLUDE) / "qvit_hip.h").read_text()
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float}
    for name in ("qvit_qat_step", "qvit_qat_quant_step"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(1).replace("\n", " ").split(",")]
        want = [ctypes.c_void_p if ("*" in a or a.startswith("hipStream_t")) else ctype[a.split()[0]] for a in args]
        fn = getattr(lib, name)
        assert list(fn.argtypes) == want, name
        assert fn.restype is ctypes.c_int
    assert "qat_step.hip" in build.SOURCES
    consts = dict(re.findall(r"#define\s+(QVIT_QAT_\w+)\s+(-?\d+)", header))
    for n in ("SGD", "ADAM", "ADAMW", "WARMUP", "RANGE", "FIX"):
        assert int(consts[f"QVIT_QAT_{n}"]) == getattr(_lib, f"QAT_{n}")


DENSE_ROWS = [
    # NULL tables first, in front of everything else
    (dict(tensors=None), ENULL), (dict(chunks=None), ENULL), (dict(tensors=None, chunks=C0 + 4), ENULL),
    (dict(chunks=None, ntensors=-1), ENULL), (dict(tensors=None, variant=9), ENULL),
    # alignment of the tables: 8 bytes
    (dict(tensors=T0 + 4), EALIGN), (dict(chunks=C0 + 4), EALIGN), (dict(tensors=T0 + 4, ntensors=-1), EALIGN),
    (dict(chunks=C0 + 2, variant=9), EALIGN), (dict(tensors=T0 + 8, chunks=C0 + 8), OK),
    # counts
    (dict(ntensors=-1), EINVAL), (dict(nchunks=-1), EINVAL), (dict(nchunks=(1 << 40) + 1), EINVAL),
    (dict(ntensors=-1, variant=9), EINVAL),
    # the variant last
    (dict(variant=3), EINVAL), (dict(variant=-1), EINVAL), (dict(variant=9, ntensors=5), EINVAL),
    (dict(variant=_lib.QAT_SGD), OK), (dict(variant=_lib.QAT_ADAM), OK), (dict(ntensors=5, nchunks=0), OK),
    (dict(ntensors=0, nchunks=7), OK),
]

QUANT_ROWS = [
    (dict(quants=None), ENULL), (dict(bits=None), ENULL), (dict(quants=None, bits=B0 + 2), ENULL),
    (dict(bits=None, nquants=-1), ENULL), (dict(quants=None, stage=7), ENULL),
    (dict(quants=Q0 + 4), EALIGN), (dict(bits=B0 + 2), EALIGN), (dict(bits=B0 + 2, nquants=-1), EALIGN),
    (dict(quants=Q0 + 4, stage=7), EALIGN), (dict(bits=B0 + 4), OK),
    (dict(nquants=-1), EINVAL), (dict(nquants=-1, variant=9), EINVAL),
    (dict(variant=3), EINVAL), (dict(variant=3, stage=7), EINVAL),
    (dict(stage=3), EINVAL), (dict(stage=-1), EINVAL), (dict(stage=3, ranges=(1, 16, 4, 16)), EINVAL),
    # the bit ranges: 2 <= min <= max <= 32 on both sides
    (dict(ranges=(1, 16, 4, 16)), EINVAL), (dict(ranges=(4, 3, 4, 16)), EINVAL), (dict(ranges=(4, 33, 4, 16)), EINVAL),
    (dict(ranges=(4, 16, 1, 16)), EINVAL), (dict(ranges=(4, 16, 8, 7)), EINVAL), (dict(ranges=(4, 16, 4, 33)), EINVAL),
    (dict(ranges=(2, 32, 2, 32)), OK), (dict(stage=_lib.QAT_WARMUP), OK), (dict(stage=_lib.QAT_FIX, first_fix=1), OK),
    (dict(variant=_lib.QAT_SGD), OK),
]


@pytest.mark.parametrize("fn,rows", [(dense, DENSE_ROWS), (quant, QUANT_ROWS)], ids=["qat_step", "qat_quant_step"])
def test_rejection_table(lib, fn, rows):
    got = [(kw, fn(lib, **kw)) for kw, _ in rows]
    wrong = [(kw, status, want) for (kw, status), (_, want) in zip(got, rows) if status != want]
    assert not wrong, "\n".join(f"{fn.__name__}({kw}) returned {s}, expected {w}" for kw, s, w in wrong)


def test_every_row_is_answered_before_a_launch():
    for kw, want in DENSE_ROWS:
        assert want != OK or kw.get("ntensors", 0) == 0 or kw.get("nchunks", 0) == 0, kw
    for kw, want in QUANT_ROWS:
        assert want != OK or kw.get("nquants", 0) == 0, kw


def test_table_layouts_match_the_python_side():
    """The descriptor sizes the optimizer fills as int64 rows are the ones the header documents."""
    header = (Path(build.INCLUDE) / "qvit_hip.h").read_text()
    assert f"ntensors descriptors of {_lib.QAT_TENSOR_BYTES} bytes" in header
    assert f"nquants descriptors of {_lib.QAT_QUANT_BYTES} bytes" in header
    assert _lib.QAT_CHUNK == 4096 and "[4096 index" in header
