"""Every copy of the device quantizer in the ViT int8 kernels, driven one ulp at a time across every code boundary.

The quantizer's input is set exactly through each kernel (the value itself; a GEMM's bias under zero activation
codes; beta of a constant LayerNorm row, where (x - mean) = 0 in every arm: the row sum of 3.0 is exact and the
division by cols is IEEE; v under attention over one key, where p = l = 1), so the codes must equal
vit_codes_ref.device_codes bit for bit outside the double-rounding mask (empty for the linear and ULTRA_ACT sets,
about 2^-19 of the nonlinear elements). No share of differing codes is allowed anywhere in this file, except where a
docstring says why (`bracket_ties`: attention over 33 keys)."""
import pytest
import torch

import vit_codes_ref as V
from oracle import quant_oracle as O
from quantized_vit_amd import _lib
from test_gpu_kernels import _p, _round_up, pack_codes
from ultra_ref import assert_codes_tie_proven

pytestmark = pytest.mark.gpu

QTC = {O.LINEAR: _lib.QT_LINEAR, O.NONLINEAR: _lib.QT_NONLINEAR, V.ULTRA_ACT: _lib.QT_ULTRA_ACT}
SETS = pytest.mark.parametrize("ps", V.PARAM_SETS, ids=repr)
_CACHE = {}


def _vals(ps, gelu=False):
    """The boundary inputs of a set (the GELU pre-images h for the GELU paths), computed once."""
    key = (ps.name, gelu)
    if key not in _CACHE:
        _CACHE[key] = V.gelu_boundary_inputs(ps) if gelu else V.boundary_inputs(*ps.args)
    return _CACHE[key]


def _q(ps, dev):
    """(qtype, d, qm, t, levels) as the C ABI takes them."""
    if ps.qt == V.ULTRA_ACT:
        return QTC[ps.qt], None, None, None, ps.levels
    return QTC[ps.qt], _p(ps.d, dev), _p(ps.qm, dev), _p(ps.t, dev) if ps.qt == O.NONLINEAR else None, 0


def _okw(ps, dev):
    qt, d, qm, t, lv = _q(ps, dev)
    return dict(out_qtype=qt, out_d=d, out_qm=qm, out_t=t, out_levels=lv)


def _table(ps, gelu, dev):
    """The code table at the plan geometry, or None where the plan builds none (ULTRA_ACT, too many buckets)."""
    from quantized_vit_amd.quant_layers import epilogue_table_geometry, saturation_level
    if ps.qt == V.ULTRA_ACT:
        return None
    qt, d, qm, t, _ = _q(ps, dev)
    geo = epilogue_table_geometry(qt, ps.d, ps.qm, ps.t, saturation_level(qt, ps.d, ps.qm, ps.t), gelu)
    if geo is None:
        return None
    table = _lib.epi_table_build(_lib.EPI_I8_GELU if gelu else _lib.EPI_I8, qt, d, qm, t, 0, *geo, dev)
    torch.cuda.synchronize()
    valid = int(table[12:16].view(torch.int32).item())
    assert valid == 1 or ps.qm < 0, "the device rejected the plan's table"
    return table if valid == 1 else None


def _want(x, ps, gelu=False):
    v = O.gelu(x).reshape(x.shape) if gelu else x
    return V.device_codes(v, *ps.args), V.double_rounding_mask(v, *ps.args)


def assert_exact(got, x, ps, gelu=False, what=""):
    """got == device_codes([gelu](x)) on every element outside the double-rounding mask."""
    want, mask = _want(x, ps, gelu)
    got = got.cpu().reshape(want.shape)
    bad = (got != want) & ~mask
    if bad.any():
        i = bad.reshape(-1).nonzero()[0].item()
        xv = x.reshape(-1)[i]
        raise AssertionError(f"{what} {ps}: {int(bad.sum())} of {bad.numel()} codes differ; first at {i}: x = "
                             f"{xv.item():.9g} ({xv.view(torch.int32).item():#x}), got {int(got.reshape(-1)[i])}, "
                             f"want {int(want.reshape(-1)[i])}")
    assert mask.double().mean().item() <= V.CAP_DOUBLE_ROUNDING


def _chunks(vals, n):
    """[ceil(len / n)][n]: the values in chunks of n, the last one filled by cycling."""
    return V.tile_columns(vals, -(-vals.numel() // n), n)


# ---- the value taken directly -------------------------------------------------------------------------------------
@SETS
def test_quantize_act_boundaries(dev, ps):
    """Vector (cols % 4 == 0) and scalar (cols % 4 == 1, with a partial 16-column chunk) loads, rows 5 and 67; the
    guarded fast path and QT_FORCE_CAREFUL agree on the whole input, mask or not."""
    vals = _vals(ps)
    qt, d, qm, t, lv = _q(ps, dev)
    for rows in (5, 67):
        c4 = _round_up(-(-vals.numel() // rows), 4)
        for cols in (c4, c4 + 1):
            x = V.tile_columns(vals, rows, cols, offset=rows)
            kpad = _round_up(cols, 16)
            outs = []
            for flag in (0, _lib.QT_FORCE_CAREFUL):
                out = torch.full((rows, kpad), 77, dtype=torch.int8, device=dev)
                _lib.quantize_act_i8(x.to(dev), qt | flag, d, qm, t, lv, out, kpad)
                outs.append(out.cpu())
            assert torch.equal(outs[0], outs[1]), "guarded fast path != careful path"
            assert (outs[0][:, cols:] == 0).all()
            assert_exact(outs[0][:, :cols], x, ps, what=f"quantize_act {rows}x{cols}")


@SETS
def test_fake_quant_boundaries(dev, ps):
    """d * code rounded once (ULTRA_ACT: code / levels). A NaN passes through the linear and nonlinear quantizers as
    in the reference (sign(NaN) * output); its code, and ULTRA_ACT's value, stay 0."""
    x = _vals(ps)
    qt, d, qm, t, lv = _q(ps, dev)
    y = _lib.fake_quant_f32(x.to(dev), qt, d, qm, t, lv).cpu()
    k, mask = _want(x, ps)
    want = k.float() / float(ps.levels) if ps.qt == V.ULTRA_ACT else V._f32(ps.d) * k.float()
    nan = torch.isnan(x) if ps.qt != V.ULTRA_ACT else torch.zeros_like(mask)
    assert bool(nan.any()) == (ps.qt != V.ULTRA_ACT) and torch.equal(torch.isnan(y), nan)
    keep = ~mask & ~nan
    assert torch.equal(y[keep], want[keep]), (y[keep] != want[keep]).nonzero()[:4].tolist()


@SETS
def test_gelu_quant_boundaries(dev, ps):
    """h > 0 whose O.gelu(h) lies within 8 ulp of a boundary preimage: codes == device_codes(O.gelu(h))."""
    vals = _vals(ps, gelu=True)
    qt, d, qm, t, lv = _q(ps, dev)
    for rows, extra in ((5, 0), (5, 1), (67, 0)):
        cols = _round_up(-(-vals.numel() // rows), 4) + extra
        h = V.tile_columns(vals, rows, cols)
        kpad = _round_up(cols, 16)
        out = torch.full((rows, kpad), 77, dtype=torch.int8, device=dev)
        _lib.gelu_quant_i8(h.to(dev), qt, d, qm, t, lv, out, kpad)
        assert_exact(out[:, :cols], h, ps, gelu=True, what=f"gelu_quant {rows}x{cols}")


# ---- GEMM epilogues: zero activation codes, the value is bias[n] ---------------------------------------------------
def _weights(dev, N, K, wfmt):
    packed, npad, kpad = pack_codes(torch.zeros((N, K), dtype=torch.int64), _lib.W4 if wfmt != _lib.W8 else _lib.W8, dev)
    if wfmt == _lib.W4R:
        packed = _lib.pack_weight_w4r(packed, npad, kpad)
    elif wfmt == _lib.W8R:
        packed = _lib.pack_weight_w8r(packed, npad, kpad)
    return packed, npad, kpad


def assert_gelu_table_ties(tabled, direct, h, ps):
    """The tabled GELU epilogue against the direct one. fp32 GELU is monotone only up to rounding; where it zig-zags
    by an ulp across a change point the table's bisection picks one of the adjacent transitions (the allowance
    test_epilogue_code_table_equals_direct documents). Here every input sits at a change point, so a share means
    nothing; instead each differing code must be one step off and must be the direct code of an h within 8 ulp."""
    diff = tabled != direct
    if not diff.any():
        return
    assert (tabled[diff].int() - direct[diff].int()).abs().max().item() <= 1
    near = V._neighbours(h[diff].abs(), 8)
    codes = V.device_codes(O.gelu(near.reshape(-1)).reshape(near.shape), *ps.args)
    proven = (codes == tabled[diff].unsqueeze(1)).any(dim=1)
    assert proven.all(), f"{int((~proven).sum())} tabled GELU codes are no neighbour's direct code"


@pytest.mark.parametrize("gelu", [False, True], ids=["i8", "i8-gelu"])
@SETS
def test_gemm_epilogue_boundaries(dev, ps, gelu):
    """A = 0, K = 128: W4, W8, W4R and W8R, direct and through the plan's code table, M in {5, 129}; N = all the values
    (129 column tiles and a ragged tail with a partial 4-column word)."""
    vals = _vals(ps, gelu)
    if vals.numel() % 4 == 0:
        vals = torch.cat([vals, vals[:1]])
    N, K = vals.numel(), 128
    epi = _lib.EPI_I8_GELU if gelu else _lib.EPI_I8
    table = _table(ps, gelu, dev)
    one = _p(1.0, dev)
    first = None
    for wfmt in (_lib.W4, _lib.W8, _lib.W4R, _lib.W8R):
        packed, npad, kpad = _weights(dev, N, K, wfmt)
        bias_pad = _lib.pad_bias(vals.to(dev), N, npad, dev)
        for M in (5, 129):
            A = torch.zeros((M, kpad), dtype=torch.int8, device=dev)
            for tab in ((None,) if table is None else (None, table)):
                out = torch.full((M, _round_up(N, 16)), 99, dtype=torch.int8, device=dev)
                _lib.gemm(A, M, kpad, packed, wfmt, N, npad, one, one, bias_pad, epi, out, epi_table=tab, **_okw(ps, dev))
                torch.cuda.synchronize()
                assert bool((out == out[:1]).all()), "rows of one bias differ"
                assert bool((out[:, N:] == 99).all())
                row = out[0, :N].cpu()
                if tab is None:
                    assert_exact(row, vals, ps, gelu, what=f"gemm wfmt {wfmt} M {M}")
                    first = row if first is None else first
                    assert torch.equal(row, first)
                elif gelu:
                    assert_gelu_table_ties(row, first, vals, ps)
                else:
                    assert torch.equal(row, first), f"tabled != direct, wfmt {wfmt} M {M}"


@pytest.mark.parametrize("wfmt", [_lib.W4, _lib.W8, _lib.W4R, _lib.W8R])
def test_gemm_epilogue_exact_ties_round_to_even(dev, wfmt):
    """Non-zero codes: d_act d_wt = 2^-7 and d = 2^-6, so v / d = acc / 2 exactly; one-hot activation rows -127 .. 127
    against weight codes -7 .. 7 reach every product, and every odd acc below saturation is an exact tie."""
    ps = V.POW2
    a = torch.zeros((255, 128), dtype=torch.int64)
    a[:, 5] = torch.arange(-127, 128)
    w = torch.zeros((15, 128), dtype=torch.int64)
    w[:, 5] = torch.arange(-7, 8)
    packed, npad, kpad = pack_codes(w, _lib.W8 if wfmt == _lib.W8 else _lib.W4, dev)
    if wfmt == _lib.W4R:
        packed = _lib.pack_weight_w4r(packed, npad, kpad)
    elif wfmt == _lib.W8R:
        packed = _lib.pack_weight_w8r(packed, npad, kpad)
    acc = O.int_accumulators(a.float(), w.float())
    v = (acc.double() * 2.0 ** -7).float()
    want = V.device_codes(v, *ps.args)
    n = acc.abs()
    half = torch.where(n >= 254, torch.full_like(n, 127), torch.where(n % 2 == 0, n // 2, n // 2 + (n // 2) % 2))
    assert torch.equal(want.long(), half * torch.sign(acc))            # the restatement itself rounds half to even
    for table in (None, _table(ps, False, dev)):
        out = torch.full((255, 16), 99, dtype=torch.int8, device=dev)
        _lib.gemm(a.to(torch.int8).to(dev), 255, kpad, packed, wfmt, 15, npad, _p(2.0 ** -3, dev), _p(2.0 ** -4, dev),
                  None, _lib.EPI_I8, out, epi_table=table, **_okw(ps, dev))
        assert torch.equal(out[:, :15].cpu(), want)


@pytest.mark.parametrize("gelu", [False, True], ids=["i8", "i8-gelu"])
@SETS
def test_gemm_a32_epilogue_boundaries(dev, ps, gelu):
    """The weight-stationary schedule's epilogue (gemm_ws.hip): A = 0, N = 3072, K = 768, M in {1, 65}; equal to the
    reference and to qvit_gemm on the same bias."""
    N, K = 3072, 768
    epi = _lib.EPI_I8_GELU if gelu else _lib.EPI_I8
    assert _lib.gemm_a32_fits(K, _lib.W4, N, N, epi)
    chunks = _chunks(_vals(ps, gelu), N)
    packed, npad, kpad = _weights(dev, N, K, _lib.W4)
    one = _p(1.0, dev)
    kw = _okw(ps, dev)
    for M in (1, 65):
        A32 = torch.zeros(_lib.t32_rows(M) * K, dtype=torch.int8, device=dev)
        A = torch.zeros((M, K), dtype=torch.int8, device=dev)
        ws = torch.full((len(chunks), M, N), 55, dtype=torch.int8, device=dev)
        tiles = torch.full((len(chunks), M, N), 77, dtype=torch.int8, device=dev)
        for i, c in enumerate(chunks):
            bias_pad = _lib.pad_bias(c.to(dev), N, npad, dev)
            _lib.gemm_a32(A32, M, K, packed, _lib.W4, N, npad, one, one, bias_pad, epi, ws[i], **kw)
            _lib.gemm(A, M, K, packed, _lib.W4, N, npad, one, one, bias_pad, epi, tiles[i], **kw)
        torch.cuda.synchronize()
        assert torch.equal(ws, tiles)
        assert bool((ws == ws[:, :1]).all())
        assert_exact(ws[:, 0], chunks, ps, gelu, what=f"gemm_a32 M {M}")


# ---- LayerNorm: constant rows, the value is beta[c] ----------------------------------------------------------------
LN_BOUNDARY_ARMS = {"persist<1>": 192, "persist<2>": 384, "persist<3>": 768, "persist<4>": 1000, "reg<8>": 1280,
                    "scalar-cols770": 770, "scalar-cols2052": 2052}


def _ln_setup(dev, ps, cols):
    chunks = _chunks(_vals(ps), cols)
    g = torch.Generator().manual_seed(cols)
    gamma = (torch.rand(cols, generator=g) + 0.5).to(dev)
    x = torch.full((5, cols), 3.0, device=dev)
    return chunks, gamma, x


@pytest.mark.parametrize("arm", list(LN_BOUNDARY_ARMS))
@SETS
def test_layernorm_quant_boundaries(dev, ps, arm):
    """Five constant rows x = 3.0 (four rows per workgroup) through each vector arm and two scalar arms, direct and
    (persist arms) through the quantizer's code table."""
    cols = LN_BOUNDARY_ARMS[arm]
    chunks, gamma, x = _ln_setup(dev, ps, cols)
    qt, d, qm, t, lv = _q(ps, dev)
    kpad = _round_up(cols, 128)
    table = _table(ps, False, dev) if arm.startswith("persist") else None
    for tab in ((None,) if table is None else (None, table)):
        out = torch.full((len(chunks), 5, kpad), 77, dtype=torch.int8, device=dev)
        for i, c in enumerate(chunks):
            _lib.layernorm_quant_i8(x, gamma, c.to(dev), 1e-6, qt, d, qm, t, lv, out[i], kpad, code_table=tab)
        torch.cuda.synchronize()
        assert bool((out == out[:, :1]).all()) and bool((out[:, :, cols:] == 0).all())
        assert_exact(out[:, 0, :cols], chunks, ps, what=f"layernorm {arm} table {tab is not None}")


@SETS
def test_layernorm_t32_boundaries(dev, ps):
    """qvit_layernorm_quant_i8_t32 (persist<3>, T32 stores), un-permuted with _lib.t32_to_rows; direct and tabled."""
    cols = kpad = 768
    chunks, gamma, x = _ln_setup(dev, ps, cols)
    qt, d, qm, t, lv = _q(ps, dev)
    table = _table(ps, False, dev)
    for tab in ((None,) if table is None else (None, table)):
        out = torch.full((len(chunks), _lib.t32_rows(5) * kpad), 93, dtype=torch.int8, device=dev)
        for i, c in enumerate(chunks):
            _lib.layernorm_quant_i8_t32(x, gamma, c.to(dev), 1e-6, qt, d, qm, t, lv, out[i], kpad, code_table=tab)
        torch.cuda.synchronize()
        rows = torch.stack([_lib.t32_to_rows(o, 5, kpad) for o in out])
        assert bool((rows == rows[:, :1]).all())
        assert_exact(rows[:, 0], chunks, ps, what=f"layernorm t32 table {tab is not None}")


@pytest.mark.parametrize("M", [5, 129])
@pytest.mark.parametrize("ps", V.VIT_SETS, ids=repr)
def test_gemm_resid_ln_boundaries(dev, ps, M):
    """The LayerNorm behind qvit_gemm_resid_ln's tiles: A = 0 and a zero bias leave the constant residual rows
    constant (3.0 + 0), so y = beta there too."""
    N, K = 768, 256
    chunks, gamma, _ = _ln_setup(dev, ps, N)
    packed, npad, kpad = _weights(dev, N, K, _lib.W4)
    qt, d, qm, t, lv = _q(ps, dev)
    A = torch.zeros((M, kpad), dtype=torch.int8, device=dev)
    one = _p(1.0, dev)
    bias_pad = _lib.pad_bias(None, N, npad, dev)
    table = _table(ps, False, dev)
    for tab in ((None,) if table is None else (None, table)):
        out = torch.full((len(chunks), M, N), 55, dtype=torch.int8, device=dev)
        for i, c in enumerate(chunks):
            C = torch.full((M, N), 3.0, device=dev)
            _lib.gemm_resid_ln(A, M, kpad, packed, _lib.W4, N, npad, one, one, bias_pad, C, gamma, c.to(dev), 1e-6, qt, d,
                               qm, t, lv, tab, out[i], N)
        torch.cuda.synchronize()
        assert bool((C == 3.0).all())
        assert bool((out == out[:, :1]).all())
        assert_exact(out[:, 0], chunks, ps, what=f"gemm_resid_ln M {M} table {tab is not None}")


# ---- attention over one key: out = v -------------------------------------------------------------------------------
def _split_exact(x):
    """The values the fp16 hi / lo operand split carries exactly (every boundary of the power-of-two set, and the
    neighbours whose remainder fits an fp16)."""
    hi = x.half()
    lo = (x - hi.float()).half()
    return x[(hi.float() + lo.float()) == x]


@pytest.mark.parametrize("ldo", [128, 132], ids=["16B-stores", "4B-stores"])
@pytest.mark.parametrize("path", ["fp32-input", "split", "split-table", "fused", "fused-table"])
@pytest.mark.parametrize("ps", [V.POW2, V.PSET["linear-d1/127"], V.PSET["nonlinear-qm1.5-t0.85"]], ids=repr)
def test_attention_one_key_boundaries(dev, ps, path, ldo):
    """N = 1: the score's softmax is exp2(0) / 1 and inv = 1 / (1 * in_scale) = 1, so out = v_hi + v_lo = v bit for
    bit. H = 2, B = 3. The linear power-of-two set, whose boundaries are fp16 values; there the fast quotient is exact,
    so a lost fix-up cannot show, hence also a linear and a nonlinear set with d no power of two, restricted like the
    first to the values the hi / lo split carries exactly (a quarter of the neighbours of every boundary and more)."""
    from test_gpu_attention import split_planes
    B, H = 3, 2
    C = 64 * H
    vals = _split_exact(_vals(ps))
    assert vals.numel() > 2000
    if ps is V.POW2:
        assert (vals == 63.5 * ps.d).any() and (vals == -0.5 * ps.d).any()
    kw = _okw(ps, dev)
    table = _table(ps, False, dev) if path.endswith("table") else None
    assert table is not None or not path.endswith("table")
    fused = path.startswith("fused")
    chunks = _chunks(vals, C if fused else B * C)
    out = torch.full((len(chunks), B, ldo), 99, dtype=torch.int8, device=dev)
    if fused:
        packed, npad, kpad = _weights(dev, 3 * C, 256, _lib.W4)
        A = torch.zeros((B, kpad), dtype=torch.int8, device=dev)
        one = _p(1.0, dev)
    for i, c in enumerate(chunks):
        o = out[i][:, :C] if fused else out[i]
        if fused:
            bias_pad = _lib.pad_bias(torch.cat([torch.zeros(2 * C), c]).to(dev), 3 * C, npad, dev)
            _lib.qkv_attention(A, B, 1, kpad, packed, npad, one, one, bias_pad, H, 0.125, o, _lib.ATT_I8, 1.0,
                               epi_table=table, **kw)
        else:
            qkv = torch.zeros((B, 3 * C))
            qkv[:, 2 * C:] = c.reshape(B, C)
            if path == "fp32-input":
                _lib.attention(qkv.to(dev), B, 1, H, 64, 0.125, o, _lib.ATT_I8, 1.0, **kw)
            else:
                hi, lo = split_planes(qkv, B, 1, H, 1.0)
                _lib.attention_split(hi.to(dev), lo.to(dev), B, 1, H, 64, 0.125, o, _lib.ATT_I8, 1.0, epi_table=table,
                                     **kw)
    torch.cuda.synchronize()
    assert bool((out[:, :, C:] == 99).all())
    got = out[:, :, :C].cpu()
    if fused:
        assert bool((got == got[:, :1]).all())
        got = got[:, 0]
    assert_exact(got.reshape(chunks.shape), chunks, ps, what=f"attention {path} ldo {ldo}")


@pytest.mark.parametrize("path", ["fp32-input", "split", "split-table"])
def test_attention_identical_value_rows(dev, path):
    """N = 33 keys with identical v rows: out = v up to the rounding of sum(p v) / sum(p), so the codes are compared
    through bracket_ties with the attention delta (2e-6 max |out|), not bit for bit. Random v over the whole range
    (boundary inputs would all be possible ties), q and k random; the cap is checked on the CPU."""
    from test_gpu_attention import split_planes
    ps = V.POW2
    B, N, H = 3, 33, 2
    C = 64 * H
    c = V.identical_rows_case(B, N, H)
    qkv, ref, tie = c.qkv, c.ref, c.tie
    out = torch.full((B * N, C), 99, dtype=torch.int8, device=dev)
    if path == "fp32-input":
        _lib.attention(qkv.to(dev), B, N, H, 64, 0.125, out, _lib.ATT_I8, 1.0, **_okw(ps, dev))
    else:
        hi, lo = split_planes(qkv, B, N, H, 1.0)
        _lib.attention_split(hi.to(dev), lo.to(dev), B, N, H, 64, 0.125, out, _lib.ATT_I8, 1.0,
                             epi_table=_table(ps, False, dev) if path == "split-table" else None, **_okw(ps, dev))
    torch.cuda.synchronize()
    assert_codes_tie_proven(out, ref, tie, V.CAP_ATTN)
