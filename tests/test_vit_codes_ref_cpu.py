"""The CPU restatement of the device quantizer (tests/vit_codes_ref.py) against the oracle, the boundary inputs, and
the conditions under which the GPU comparisons mean something: an (almost) empty double-rounding mask and
possible-tie shares within their caps, all on the reference alone. No GPU."""
import pytest
import torch

import vit_codes_ref as V
from oracle import quant_oracle as O
from oracle.ties import tie_check
from ultra_ref import tie_share

LINEAR_SETS = [p for p in V.PARAM_SETS if p.qt == O.LINEAR]
NONLINEAR_SETS = [p for p in V.PARAM_SETS if p.qt == O.NONLINEAR]


def _inputs(ps):
    g = torch.Generator().manual_seed(1)
    x = torch.cat([V.boundary_inputs(*ps.args), torch.randn(20000, generator=g) * abs(ps.qm) * 0.6])
    return x[~torch.isnan(x)]          # the oracle returns NaN for NaN, the device code 0 (pinned below)


@pytest.mark.parametrize("ps", LINEAR_SETS, ids=repr)
def test_device_codes_equal_oracle_linear(ps):
    x = _inputs(ps)
    assert torch.equal(V.device_codes(x, *ps.args).float(), O.quant_codes(x, ps.qt, ps.d, ps.qm))


@pytest.mark.parametrize("ps", NONLINEAR_SETS, ids=repr)
def test_device_codes_differ_from_oracle_only_at_proven_ties(ps):
    x = _inputs(ps)
    own = O.quant_codes(x, ps.qt, ps.d, ps.qm, ps.t)
    st = tie_check(x, V.device_codes(x, *ps.args).float(), own, ps.qt, ps.d, ps.qm, ps.t)
    assert st["non_ties"] == 0, st
    assert st["flips"] < 0.5 * st["total"]


def test_device_codes_specials():
    x = torch.tensor([0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e-45, -1e-45, 5.0, -5.0])
    for ps in V.VIT_SETS:
        L = min(V.saturation_code(ps.qt, ps.d, ps.qm, ps.t), 127)
        k = V.device_codes(x, *ps.args).tolist()
        assert k[:3] == [0, 0, 0] and k[3:5] == [L, -L], (ps, k)
        assert k[5:7] == ([L, -L] if ps.qm < 0 else [0, 0]), (ps, k)      # |x| >= a negative q_m: saturated
        if abs(ps.qm) < 5:
            assert k[7:] == [L, -L]
    u = V.device_codes(torch.tensor([-1.0, 0.0, 0.5, 1.0, 7.0, float("nan"), float("inf")]), V.ULTRA_ACT, 1, 0, 1, 15)
    assert u.tolist() == [0, 0, 8, 15, 15, 0, 15]                          # 7.5 rounds to even


@pytest.mark.parametrize("ps", V.PARAM_SETS, ids=repr)
def test_boundary_inputs_straddle_every_boundary(ps):
    ulps = 64
    x = V.boundary_inputs(*ps.args, ulps=ulps)
    nb = V.num_boundaries(*ps.args)
    assert nb >= 1 and x.numel() >= 2 * nb * (2 * ulps + 1)
    pos = x[:nb * (2 * ulps + 1)].reshape(nb, 2 * ulps + 1)
    assert torch.equal(x[nb * (2 * ulps + 1):2 * nb * (2 * ulps + 1)].reshape(pos.shape), -pos)
    assert (pos[:, 1:] > pos[:, :-1]).all()
    k = V.device_codes(pos, *ps.args).to(torch.int64)
    kneg = V.device_codes(-pos, *ps.args).to(torch.int64)
    want = torch.arange(nb).unsqueeze(1)
    if ps.qt != V.ULTRA_ACT and ps.qm < 0:
        assert (k == nb).all() and (kneg == -nb).all()      # everything saturates; the boundaries are still walked
        return
    assert ((k == want) | (k == want + 1)).all()
    inside = torch.ones(nb, dtype=torch.bool) if ps.qt == V.ULTRA_ACT else pos[:, -1] < ps.qm
    assert inside[:-1].all() and (inside.all() or ps is V.SAT_OFFSET)     # a boundary past q_m: all saturated
    assert (k == want)[inside].any(dim=1).all() and (k == want + 1).any(dim=1).all()
    assert (k[:, 1:] >= k[:, :-1]).all()
    assert torch.equal(kneg, -k) or ps.qt == V.ULTRA_ACT
    if ps is V.POW2:
        q = pos[:, ulps].double() / ps.d
        assert torch.equal(q, want[:, 0].double() + 0.5)     # exact ties: they must round to even
        assert torch.equal(k[:, ulps], (want[:, 0] + 1) // 2 * 2)


@pytest.mark.parametrize("ps", V.PARAM_SETS, ids=repr)
def test_double_rounding_mask_share(ps):
    x = V.boundary_inputs(*ps.args)
    share = V.double_rounding_mask(x, *ps.args).double().mean().item()
    assert share <= V.CAP_DOUBLE_ROUNDING, share
    if ps.qt != O.NONLINEAR:
        assert share == 0.0
    if ps.qt != V.ULTRA_ACT:
        h = V.gelu_boundary_inputs(ps)
        assert h.numel() >= 4 * V.num_boundaries(*ps.args) or ps.qm < 0
        share = V.double_rounding_mask(O.gelu(h), *ps.args).double().mean().item()
        assert share <= V.CAP_DOUBLE_ROUNDING, share


def test_double_rounding_mask_marks_midpoints():
    """A value whose fp64 log is an fp32 midpoint to within 2^-21 ulp is marked, one 2^-10 ulp away is not."""
    f = torch.tensor([0.75], dtype=torch.float32)
    up = torch.nextafter(f, torch.tensor([2.0]))
    mid = 0.5 * (f.double() + up.double())
    ulp = (up.double() - f.double())
    assert V._near_midpoint(mid + 2.0 ** -21 * ulp).all() and V._near_midpoint(mid - 2.0 ** -21 * ulp).all()
    assert not V._near_midpoint(mid + 2.0 ** -10 * ulp).any() and not V._near_midpoint(f.double()).any()


def test_bracket_ties_marks_exactly_the_straddling_values():
    ps = V.POW2
    v = torch.tensor([0.5, 1.5 - 1e-6, 1.5 + 1e-6, 1.5 + 1e-3, -2.5 + 1e-6], dtype=torch.float64) * ps.d
    ref, tie = V.bracket_ties(v, 1e-5 * ps.d, V.codes_fn(ps))
    assert tie.tolist() == [True, True, True, False, True]
    assert ref[3].item() == 2


# ---- the possible-tie share of every random-data case, on the reference alone ---------------------------------------
@pytest.mark.parametrize("gelu,qt,t", V.GEMM_CODE_CASES)
def test_gemm_code_case_tie_share(gelu, qt, t):
    c = V.gemm_code_case(gelu, qt, t)
    assert tie_share(c.tie) <= c.cap, tie_share(c.tie)
    assert len(torch.unique(c.ref)) > (30 if gelu else 60)


@pytest.mark.parametrize("gelu,qt,t", V.EPI_GEMM_CASES)
def test_epi_gemm_case_tie_share(gelu, qt, t):
    c = V.epi_gemm_case(gelu, qt, t)
    assert tie_share(c.tie) <= c.cap, tie_share(c.tie)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("qt", [O.LINEAR, O.NONLINEAR])
@pytest.mark.parametrize("cols", V.LN_COLS)
def test_layernorm_case_tie_share(cols, qt, affine):
    gamma, beta, xs = V.ln_case_inputs(cols, affine)
    ties = torch.cat([V.ln_ties(x, gamma, beta, V._qset(qt, V.LN_D, V.LN_QM, 1.0))[1].reshape(-1) for x in xs])
    assert tie_share(ties) <= V.CAP_LN, tie_share(ties)


@pytest.mark.parametrize("qt,t", V.ATTN_CODE_CASES)
def test_attention_code_case_tie_share(qt, t):
    c = V.attention_code_case(qt, t)
    assert tie_share(c.tie) <= c.cap, tie_share(c.tie)


def test_attention_split_case_tie_share():
    c = V.attention_split_case()
    assert tie_share(c.tie) <= c.cap, tie_share(c.tie)


@pytest.mark.parametrize("B,N,H,seed", V.FUSED_CODE_CASES + V.FUSED_STORE_CASES)
def test_fused_attention_case_tie_share(B, N, H, seed):
    c = V.fused_attention_case(B, N, H, seed)
    assert tie_share(c.tie) <= c.cap, tie_share(c.tie)
    assert len(torch.unique(c.ref)) > 60


def test_identical_rows_case_tie_share():
    c = V.identical_rows_case()
    assert tie_share(c.tie) <= c.cap, tie_share(c.tie)
    assert len(torch.unique(c.ref)) > 100


def test_saturation_offset_set_separates_the_saturation_code_from_the_code_at_qm():
    ps = V.SAT_OFFSET
    qm = V._f32(ps.qm)
    below = torch.nextafter(qm, torch.zeros(1))
    assert V.device_codes(torch.cat([below, qm, -qm]), *ps.args).tolist() == [126, 127, -127]
    assert (V.boundary_inputs(*ps.args) == qm).any()
