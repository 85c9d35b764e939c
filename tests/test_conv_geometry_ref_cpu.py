"""Conditions on the case table and the reference of tests/conv_geometry_ref.py, which the GPU tests of
tests/test_gpu_conv_geometry.py rest on: the inputs are free of rounding ties, the reference's gather is the index
arithmetic it claims to be, and the table tells each per-axis fault from the correct result."""
import pytest
import torch
import torch.nn.functional as F

import conv_geometry_ref as G

ALL_CASES = G.CASES + (G.INT64_CASE,)
GENERIC = [c for c in G.CASES if not c.fast]
FAST = [c for c in G.CASES if c.fast]


def test_table_shape():
    assert len(G.CASES) == 16 and len(set(G.CASE_IDS)) == 16
    assert [c.id for c in FAST] == ["F1", "F2", "F3", "F4"]
    for c in G.CASES:
        oh, ow = c.out_hw
        assert oh > 0 and ow > 0 and c.K <= c.kpad < c.K + 16 and c.kpad % 16 == 0 and c.ldc == c.kpad + 16, c.id
        # `fast` restates the kernel's condition for the patchify path
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = c.k, c.s, c.p, c.d
        cond = kw % 16 == 0 and dw == 1 and ph == 0 and pw == 0 and c.W % 4 == 0 and sw % 4 == 0 and not c.shifted
        assert c.fast == cond, c.id
    a4 = G.CASES[G.CASE_IDS.index("A4")]
    assert (a4.K, a4.kpad, a4.ldc) == (3, 16, 32)
    i = G.INT64_CASE
    assert i.out_hw == (32, 32) and i.rows == 2048 and (i.K, i.kpad) == (30, 32)
    # past the host's limit for the int arm, INT32_MAX - 2 * 256 * 16 * 256 (quant_kernels.hip)
    assert i.rows * G.INT64_LDC > 2 ** 31 - 1 - 2 * 256 * 16 * 256


@pytest.mark.parametrize("quantizer", G.QUANTIZERS)
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_inputs_are_tie_free(case, quantizer):
    """float32 and float64 codes agree on every element (a seed that fails this is changed, not the assertion),
    and the draw reaches both ends of the code range."""
    x = G.make_input(case, quantizer)
    assert x.dtype == torch.float32 and tuple(x.shape) == case.xshape
    c32, c64 = G.codes(x, quantizer, torch.float32), G.codes(x, quantizer, torch.float64)
    assert torch.equal(c32.double(), c64)
    assert torch.equal(G.ref_codes(x, case, quantizer, torch.float32).double(),
                       G.ref_codes(x, case, quantizer, torch.float64))
    if x.numel() >= 200:
        lo, hi = (0, G.ULTRA_LEVELS) if quantizer == G.ULTRA_ACT else (-127, 127)
        assert int(c64.min()) == lo and int(c64.max()) == hi


def test_ultra_inputs_reach_both_clamps():
    x = G.make_input(G.CASES[0], G.ULTRA_ACT)
    assert bool((x < 0).any()) and bool((x > 1).any())


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_out_shape_matches_unfold(case):
    oh, ow = case.out_hw
    cols = F.unfold(torch.zeros(case.xshape), case.k, case.d, case.p, case.s)
    assert tuple(cols.shape) == (case.B, case.K, oh * ow)
    y = F.conv2d(torch.zeros(case.xshape), torch.zeros((1, case.C) + case.k), None, case.s, case.p, case.d)
    assert tuple(y.shape) == (case.B, 1, oh, ow)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id)
def test_unfold_is_the_index_arithmetic(case):
    """F.unfold's rows are the gather the kernel is written as: column c*kh*kw + ih*kw + iw, zero outside."""
    c = G.codes(G.make_input(case, G.LINEAR), G.LINEAR)
    assert torch.equal(G.unfold_rows(c, case), G.gather_codes(c, case))


def _changed(cases, mutation):
    out = []
    for case in cases:
        c = G.codes(G.make_input(case, G.LINEAR), G.LINEAR)
        if not torch.equal(G.gather_codes(c, case, mutation), G.gather_codes(c, case)):
            out.append(case.id)
    return out


@pytest.mark.parametrize("mutation", G.MUTATIONS)
def test_table_discriminates_generic_arm(mutation):
    assert _changed(GENERIC, mutation), mutation


@pytest.mark.parametrize("mutation", G.FAST_PATH_MUTATIONS)
def test_table_discriminates_fast_path(mutation):
    assert _changed(FAST, mutation), mutation


def test_all_asymmetric_case_sees_every_fault():
    a1 = G.CASES[G.CASE_IDS.index("A1")]
    for mutation in G.MUTATIONS:
        assert _changed([a1], mutation) == ["A1"], mutation


def test_padding_cases_have_rows_outside_the_image():
    """A1: the top taps of the first output row lie wholly in the padding; A5: whole output rows do."""
    for cid in ("A1", "A5"):
        case = G.CASES[G.CASE_IDS.index(cid)]
        ones = G.unfold_rows(torch.ones(case.xshape), case)
        oh, ow = case.out_hw
        per_row = ones.view(case.B, oh, ow, case.C, case.k[0], case.k[1])
        if cid == "A1":
            assert float(per_row[:, 0, :, :, 0, :].sum()) == 0 and float(per_row[:, 0].sum()) > 0
        else:
            assert float(per_row[:, 0].sum()) == 0 and float(per_row[:, oh - 1].sum()) == 0
            assert float(per_row.sum()) > 0


def test_lib_conv_out_hw_matches_the_table():
    """The one output-size formula of the Python wrappers against the table's own (no library is loaded)."""
    from quantized_vit_amd import _lib
    assert len(G.CASES) == 16
    for case in G.CASES:
        assert _lib.conv_out_hw(case.H, case.W, case.k, case.s, case.p, case.d) == case.out_hw, case.id
