"""The special-value reference on the CPU: the expected tables as literals (an oracle change shows up here), the
conditions of the tiny-arm inputs (no possible tie), and the negative controls of the three checkers."""
import math

import pytest
import torch

import special_values_ref as S
import vit_codes_ref as V
from oracle import quant_oracle as O

NAN = float("nan")
# order of S.special_names: +nan -nan +inf -inf +0 -0 +max -max +min -min +den -den 1e-31 1e-38 +qm -qm below above
CODES = {
    "linear-L127": [0, 0, 127, -127, 0, 0, 127, -127, 0, 0, 0, 0, 0, 0, 127, -127, 127, 127],
    "linear-L7": [0, 0, 7, -7, 0, 0, 7, -7, 0, 0, 0, 0, 0, 0, 7, -7, 7, 7],
    "nonlinear-t1": [0, 0, 127, -127, 0, 0, 127, -127, 0, 0, 0, 0, 0, 0, 127, -127, 127, 127],
    "nonlinear-t0.8": [0, 0, 127, -127, 0, 0, 127, -127, 0, 0, 0, 0, 0, 0, 127, -127, 127, 127],
    "linear-negative-qm": [0, 0, 10, -10, 0, 0, 10, -10, 10, -10, 10, -10, 10, 10, 10, -10, 10, 10],
    "ultra-levels15": [0, 0, 15, 0, 0, 0, 15, 0, 0, 0, 0, 0, 0, 0, 15, 0, 15, 15],
    "tiny-t0.5": [0, 0, 127, -127, 0, 0, 127, -127, 11, -11, 1, -1, 127, 10, 127, -127, 127, 127],
    "tiny-t1.25": [0, 0, 127, -127, 0, 0, 127, -127, 0, 0, 0, 0, 18, 0, 127, -127, 127, 127],
}
GELU_CODES = {
    "linear-L127": [0, 0, 127, 0, 0, 0, 127, 0, 0, 0, 0, 0, 0, 0, 107, -20, 107, 107],
    "linear-L7": [0, 0, 7, 0, 0, 0, 7, 0, 0, 0, 0, 0, 0, 0, 5, -2, 5, 5],
    "nonlinear-t1": [0, 0, 127, 0, 0, 0, 127, 0, 0, 0, 0, 0, 0, 0, 119, -8, 119, 119],
    "nonlinear-t0.8": [0, 0, 127, 0, 0, 0, 127, 0, 0, 0, 0, 0, 0, 0, 120, -15, 120, 120],
    "linear-negative-qm": [0, 0, 10, 0, 0, 0, 10, 0, 10, -10, 10, -10, 10, 10, 10, -10, 10, 10],
    "ultra-levels15": [0, 0, 15, 0, 0, 0, 15, 0, 0, 0, 0, 0, 0, 0, 13, 0, 13, 13],
}
# fake-quant values in units of the saturation value s = d * L (0.0 stands for either zero)
FQ_SAT = {"linear-L127": 1.0, "linear-L7": 0.5, "nonlinear-t1": 1.5, "nonlinear-t0.8": 1.3831617832183838,
          "linear-negative-qm": 0.5}
FQ_UNITS = {
    "default": [NAN, NAN, 1, -1, 0, 0, 1, -1, 0, 0, 0, 0, 0, 0, 1, -1, 1, 1],
    "linear-negative-qm": [NAN, NAN, 1, -1, 0, 0, 1, -1, 1, -1, 1, -1, 1, 1, 1, -1, 1, 1],
}
TINY_CODES = {"tiny-t0.5": [127, 10, 1, 11, 127, -127, -10, -1, -11, -127],
              "tiny-t1.25": [18, 0, 0, 0, 0, -18, 0, 0, 0, 0]}
TINY_FQ = {"tiny-t0.5": [3.1622998350872e-16, 9.999999682655225e-20, 9.999999682655225e-21, 1.1000000297155601e-19,
                         5.4800000070408225e-18],
           "tiny-t1.25": [1.7999902982006567e-39, 0.0, 0.0, 0.0, 0.0]}


def _x(ps):
    return S.special_inputs(1.0 if ps.qt == V.ULTRA_ACT else ps.qm)


def test_special_inputs_are_what_they_claim():
    x = S.special_inputs(1.5)
    names = [n for n, _ in S.special_names(1.5)]
    assert len(names) == len(set(names)) == x.numel() == 18
    bits = x.view(torch.int32).tolist()
    assert bits[0] == 0x7FC00000 and bits[1] == 0x7FC00000 - (1 << 31)
    assert math.isinf(x[2]) and x[2] > 0 and math.isinf(x[3]) and x[3] < 0
    assert bits[4] == 0 and bits[5] == -(1 << 31)
    assert x[6].item() == torch.finfo(torch.float32).max and x[8].item() == torch.finfo(torch.float32).tiny
    assert 0 < x[10].item() < torch.finfo(torch.float32).tiny and x[11].item() == -x[10].item()      # a denormal
    assert 0 < x[13].item() < torch.finfo(torch.float32).tiny < 1e-31 < V.TINY_SWITCH               # 1e-38 is one too
    assert x[14].item() == 1.5 and x[15].item() == -1.5
    assert x[16].item() < 1.5 < x[17].item() and (x[17] - x[16]).item() == 2.0 ** -22


@pytest.mark.parametrize("ps", S.SETS + S.TINY_SETS, ids=repr)
def test_expected_codes_literal(ps):
    want = torch.tensor(CODES[ps.name], dtype=torch.int8)
    assert torch.equal(S.expected_codes(_x(ps), ps), want)
    # the CPU restatement of the device quantizer (vit_codes_ref) states the same contract
    assert torch.equal(V.device_codes(_x(ps), *ps.args), want)


@pytest.mark.parametrize("ps", S.SETS, ids=repr)
def test_expected_gelu_codes_literal(ps):
    g = O.gelu(_x(ps))
    assert torch.isnan(g[:2]).all() and math.isinf(g[2]) and g[2] > 0 and torch.isnan(g[3])     # gelu(-inf) = -inf * 0
    assert torch.equal(S.expected_gelu_codes(_x(ps), ps), torch.tensor(GELU_CODES[ps.name], dtype=torch.int8))


@pytest.mark.parametrize("ps", [p for p in S.SETS if p.qt != V.ULTRA_ACT], ids=repr)
def test_expected_fake_quant_literal(ps):
    units = torch.tensor(FQ_UNITS.get(ps.name, FQ_UNITS["default"]), dtype=torch.float32)
    want = units * V._f32(FQ_SAT[ps.name])
    got = S.expected_fake_quant(_x(ps), ps)
    assert torch.isnan(got[:2]).all() and not torch.isnan(got[2:]).any()
    assert S.same_values(got, want), got.tolist()


@pytest.mark.parametrize("ps", S.TINY_SETS, ids=repr)
def test_tiny_inputs_have_codes_and_no_ties(ps):
    """The tiny arm's inputs: below quant_fast's switch, non-zero codes where fp32 allows one, outside the double
    rounding mask of vit_codes_ref (so the device codes must equal device_codes bit for bit), and the oracle's own
    fp32 arithmetic agrees with the correctly rounded restatement on them (no tie to prove)."""
    x = S.TINY_INPUTS
    assert bool((x.abs() <= V.TINY_SWITCH).all()) and bool((x.abs() < ps.qm).all())
    both = torch.cat([x, S.special_inputs(ps.qm)])
    assert not V.double_rounding_mask(both, *ps.args).any()
    want = torch.tensor(TINY_CODES[ps.name], dtype=torch.int8)
    assert torch.equal(S.expected_codes(x, ps), want) and torch.equal(V.device_codes(x, *ps.args), want)
    assert int((want != 0).sum()) >= 2
    from oracle.ties import code_position
    pos = code_position(x, ps.qt, float(V._f32(ps.d)), float(V._f32(ps.t)))
    frac = (pos - torch.floor(pos) - 0.5).abs()
    assert float(frac[pos < 200].min()) > 0.1                       # far from every rounding tie
    fq = S.expected_fake_quant(x[:5], ps)
    assert torch.equal(fq, torch.tensor(TINY_FQ[ps.name], dtype=torch.float32)), fq.tolist()
    assert torch.equal(S.expected_fake_quant(x[5:], ps), -fq)


def test_tiny_t05_reaches_every_named_input():
    """Issue: 1e-31, 1e-38 and the denormal get non-zero codes at t = 0.5."""
    ps = S.PSET["tiny-t0.5"]
    k = S.expected_codes(torch.tensor([1e-31, 1e-38, S.DENORMAL]), ps)
    assert k.tolist() == [127, 10, 1]


# ---- the checkers and their negative controls ------------------------------------------------------------------------
def _model(x, ps, nan_code=0, neg_inf_code=None):
    k = S.expected_codes(x, ps).clone()
    k[torch.isnan(x)] = nan_code
    if neg_inf_code is not None:
        k[x == -math.inf] = neg_inf_code
    return k


def test_planted_checker_accepts_the_contract_and_rejects_wrong_models():
    ps = S.PSET["linear-L127"]
    x = _x(ps)
    want = S.expected_codes(x, ps)
    S.assert_planted(_model(x, ps), want)
    with pytest.raises(AssertionError):
        S.assert_planted(_model(x, ps, nan_code=-127), want)          # fmaxf(NaN, -127) reaching to_i8_sat
    with pytest.raises(AssertionError):
        S.assert_planted(_model(x, ps, neg_inf_code=0), want)         # -Inf swallowed
    fq = S.expected_fake_quant(x, ps)
    S.assert_planted(fq.clone(), fq)
    with pytest.raises(AssertionError):
        S.assert_planted(torch.nan_to_num(fq, nan=0.0), fq)           # the fake quantizer swallowing a NaN
    flipped = fq.clone()
    flipped[4] = -0.0
    S.assert_planted(flipped, fq)                                     # the sign of zero is not compared


def test_path_equality_checker():
    ps = S.PSET["linear-L7"]
    x = _x(ps)
    S.assert_paths_equal({"direct": _model(x, ps), "table": _model(x, ps)})
    with pytest.raises(AssertionError):
        S.assert_paths_equal({"direct": _model(x, ps), "table": _model(x, ps, nan_code=-7)})   # bucket 0's lower code
    with pytest.raises(AssertionError):
        S.assert_paths_equal({"direct": _model(x, ps)})
    a = torch.tensor([0.0, NAN])
    S.assert_paths_equal({"a": a, "b": a.clone()})
    with pytest.raises(AssertionError):
        S.assert_paths_equal({"a": a, "b": torch.tensor([-0.0, NAN])})                          # bytes, not values


def test_containment_checker():
    clean = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    poisoned = clean.clone()
    poisoned[1] = NAN
    S.assert_contained(clean, poisoned, S.rows_mask(clean.shape, [1]))
    leaky = poisoned.clone()
    leaky[2, 0] = NAN                                                  # a NaN leaked into a neighbouring row
    with pytest.raises(AssertionError):
        S.assert_contained(clean, leaky, S.rows_mask(clean.shape, [1]))
    off = poisoned.clone()
    off[3, 2] = torch.nextafter(off[3, 2], torch.tensor(0.0))          # one ulp in another row
    with pytest.raises(AssertionError):
        S.assert_contained(clean, off, S.rows_mask(clean.shape, [1]))
    codes = torch.zeros((4, 3), dtype=torch.int8)
    bad = codes.clone()
    bad[0, 2] = -127
    S.assert_contained(codes, bad, S.cols_mask(codes.shape, [2]))
    with pytest.raises(AssertionError):
        S.assert_contained(codes, bad, S.cols_mask(codes.shape, [1]))


def test_masks():
    m = S.im2col_taps(1, 2, 6, 6, 3, 1, 1, [(0, 1, 0, 0)])
    assert m.shape == (36, 18) and int(m.sum()) == 4                   # a corner pixel is tapped by four patches
    assert m[0, 9 + 4] and m[1, 9 + 3] and m[6, 9 + 1] and m[7, 9 + 0]
    assert int(S.im2col_taps(1, 2, 6, 6, 3, 1, 1, [(0, 0, 2, 3)]).sum()) == 9
    a = S.attention_blocks_mask(2, 3, 2, 4, [(0, 1)])
    assert a.shape == (6, 8) and bool(a[:3, 4:].all()) and int(a.sum()) == 12


def test_table_geometry_keeps_bucket0_free():
    """epilogue_table_geometry starts one bucket below the first change point, so bucket 0 holds a single code and the
    device can keep its `lo` byte for a NaN (qvit_epi_table_build rejects a table whose bucket 0 has a change point)."""
    from quantized_vit_amd.quant_layers import epilogue_table_geometry
    from quantized_vit_amd import _lib
    for ps in S.SETS:
        if ps.qt == V.ULTRA_ACT or ps.qm < 0:
            continue
        qt = _lib.QT_LINEAR if ps.qt == O.LINEAR else _lib.QT_NONLINEAR
        L = V.saturation_code(ps.qt, ps.d, ps.qm, ps.t)
        v_lo, w, nb = epilogue_table_geometry(qt, ps.d, ps.qm, ps.t, L, False)
        edge = torch.tensor([v_lo, v_lo + w], dtype=torch.float32)
        assert S.expected_codes(edge, ps).tolist() == [-int(L), -int(L)], ps
        v_lo, w, nb = epilogue_table_geometry(qt, ps.d, ps.qm, ps.t, L, True)
        k = S.expected_gelu_codes(torch.tensor([v_lo - 1.0, v_lo, v_lo + w], dtype=torch.float32), ps)
        assert k.tolist() == [0, 0, 0], ps
