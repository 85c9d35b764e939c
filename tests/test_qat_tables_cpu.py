"""The host side of the optimizer's device tables without a GPU: the descriptor dtypes of quantized_vit_amd._lib
against the C structs they mirror, and prune_tables' bytes against a recording of the packed-int64 code it replaced."""
from pathlib import Path

import numpy as np
import torch

from quantized_vit_amd import PruneGroup, _lib, build
from quantized_vit_amd.qat_prune import _GroupState, prune_tables

GOLDEN = Path(__file__).parent / "golden" / "prune_tables_parent.npz"

# (dtype, its *_BYTES constant, the header's words for it, the fields with the offsets of the naturally aligned struct:
# a pointer or int64_t takes 8 bytes on a multiple of 8, an int32_t 4 on a multiple of 4), written out from the struct
# definitions in csrc/qat_step.hip, csrc/qat_common.h and csrc/prune_step.hip
LAYOUTS = [
    (_lib.QAT_TENSOR_DTYPE, _lib.QAT_TENSOR_BYTES, "ntensors descriptors of 48 bytes",
     dict(p=0, grad=8, m=16, v=24, numel=32, lr_class=40, flags=44)),
    (_lib.QAT_CHUNK_DTYPE, 8, "nchunks pairs { int32_t tensor; int32_t index; }", dict(tensor=0, index=4)),
    (_lib.QAT_QUANT_DTYPE, _lib.QAT_QUANT_BYTES, "nquants descriptors of 64 bytes",
     dict(s=0, g=24, mom=48, side=56, flags=60)),
    (_lib.PRUNE_GROUP_DTYPE, _lib.PRUNE_GROUP_BYTES, "ngroups descriptors of 64 bytes",
     dict(d=0, qm=8, t=16, member_begin=24, member_count=28, rows=32, joint=36, red_begin=40, red_count=44, elems=48,
          sections=56, unit_rows=60)),
    (_lib.PRUNE_MEMBER_DTYPE, _lib.PRUNE_MEMBER_BYTES, "nmembers descriptors of 48 bytes",
     dict(p=0, grad=8, m=16, v=24, width=32, quantized=40, flags=44)),
    (_lib.PRUNE_ITEM_DTYPE, _lib.PRUNE_ITEM_BYTES, "nitems entries of 16 bytes",
     dict(group=0, row=4, state=8, link=12)),
]


def test_descriptor_dtypes_are_the_structs():
    header = (Path(build.INCLUDE) / "qvit_hip.h").read_text()
    for dt, nbytes, words, offsets in LAYOUTS:
        assert dt.itemsize == nbytes and words in header, words
        assert list(dt.names) == list(offsets), words   # the struct's fields, in its order
        assert {n: dt.fields[n][1] for n in dt.names} == offsets, words
        ends = list(offsets.values())[1:] + [nbytes]   # no padding: a field ends where the next begins
        for n, end in zip(dt.names, ends):
            field = dt.fields[n][0]
            assert field.base.kind == "i" and field.itemsize == end - offsets[n], (words, n)
    for n in ("s", "g"):   # float* s[3], const float* g[3]
        assert _lib.QAT_QUANT_DTYPE.fields[n][0].shape == (3,) and _lib.QAT_QUANT_DTYPE.fields[n][0].base.itemsize == 8
    assert _lib.Hyper._fields == ("variant", "first_step", "lr", "lr_quant", "first_momentum", "second_momentum",
                                  "alpha1", "alpha2", "weight_decay", "bias_correction1", "bias_correction2", "clip_lo",
                                  "clip_hi")


def test_prune_tables_bytes_are_the_parents():
    """prune_tables' arrays, viewed as int64, against tests/golden/prune_tables_parent.npz: the output of the function
    at commit e590e1d ("Plan lifecycle tests; plans derive later images from what they hold"), the last one that built
    the tables as hand-packed int64 pairs, recorded there for exactly this configuration: a one-row group with weight
    and bias (units 4 and 1 active, 0 pruned), a group that is not prunable, and a head group of sections = 3,
    unit_rows = 2 and 3 heads (head 1 active, head 0 pruned), in the order prunable groups first, folded."""
    K = 3
    basic = PruneGroup("b", None, [torch.zeros(6, K), torch.zeros(6)])
    fixed = PruneGroup("n", None, [torch.zeros(2, K)])
    head = PruneGroup("h", None, [torch.zeros(18, K), torch.zeros(18)], sections=3, unit_rows=2)
    gs = [_GroupState(g) for g in (basic, fixed, head)]
    gs[1].prunable = False
    gs[0].active, gs[0].pruned = [4, 1], [0]
    gs[2].active, gs[2].pruned = [1], [0]
    grow = np.zeros(3, dtype=_lib.PRUNE_GROUP_DTYPE)
    t = prune_tables(gs, [0, 2, 1], True, grow)
    want = np.load(GOLDEN)
    assert want["items"].shape == (26, 2) and want["red"].shape == (8, 2) and want["units"].shape == (9, 2)
    for key, got in (("items", t["items"]), ("red", t["red"]), ("units", t["units"]), ("grow", grow)):
        words = got.view(np.int64).reshape(len(got), got.dtype.itemsize // 8)
        assert words.shape == want[key].shape and (words == want[key]).all(), key
    assert t["joint"] == want["joint"].tolist() == [0, 2]
