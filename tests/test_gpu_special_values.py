"""NaN, Inf, zero and tiny inputs on every forward quantizer path (the "special values" paragraphs of
include/qvit_hip.h). Every test runs its kernel on a clean finite input and again with special values planted at
chosen positions, then asserts (a) the planted positions give the expected table (special_values_ref), (b) every path
of the entry point returns the same bytes, (c) everything outside the outputs that depend on a planted input is bit
identical to the clean run. One or two small launches per path."""
import math

import pytest
import torch
import torch.nn.functional as F

import special_values_ref as S
import vit_codes_ref as V
from oracle import quant_oracle as O
from quantized_vit_amd import _lib
from test_gpu_kernels import _p, _round_up, pack_codes
from test_gpu_quant_boundaries import _okw, _q, _table
from ultra_ref import assert_codes_tie_proven

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), math.inf
ALL_SETS = pytest.mark.parametrize("ps", S.SETS + S.TINY_SETS, ids=repr)
# LayerNorm / GEMM / attention output quantizers: 127 levels (nonlinear) and 7 levels (a 4-bit activation quantizer,
# whose table buckets are wide enough to hold the first change point in bucket 0 unless the geometry avoids it)
NL127 = V.PSet("nonlinear-qm1.5-t0.8-L127", O.NONLINEAR, 1.5 ** 0.8 / 127, 1.5, 0.8)
LIN7 = V.PSet("linear-qm0.5-L7", O.LINEAR, 0.5 / 7, 0.5)
OUT_SETS = pytest.mark.parametrize("ps", [NL127, LIN7], ids=repr)


def _planted(ps):
    sp = S.special_inputs(1.0 if ps.qt == V.ULTRA_ACT else ps.qm)
    return torch.cat([S.TINY_INPUTS, sp]) if ps in S.TINY_SETS else sp


def _clean(shape, ps, seed=0):
    """Finite, ordinary values over 1.2 x the quantizer's range."""
    g = torch.Generator().manual_seed(seed)
    span = 1.2 * (1.0 if ps.qt == V.ULTRA_ACT else abs(ps.qm))
    return (torch.rand(shape, generator=g) * 2 - 1) * span


def _device_rows(x, shift, dev):
    """x [rows][cols] on the device, 16-byte aligned or (shift) 4 bytes past such an address."""
    buf = torch.empty(x.numel() + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[shift:shift + x.numel()].view(x.shape)
    v.copy_(x)
    return v


def _positions(n, total):
    idx = 3 + 83 * torch.arange(n)
    assert int(idx.max()) < total
    return idx


ROW_CASES = [(512, 0), (500, 0), (512, 1)]      # 16-byte loads, scalar loads (cols % 4, partial chunk), x off 16 bytes


def _rows_case(ps, cols):
    rows = 5
    sp = _planted(ps)
    idx = _positions(sp.numel(), rows * cols)
    clean = _clean((rows, cols), ps, seed=cols)
    poisoned = clean.clone()
    poisoned.view(-1)[idx] = sp
    allowed = torch.zeros(rows * cols, dtype=torch.bool)
    allowed[idx] = True
    return sp, idx, clean, poisoned, allowed.view(rows, cols)


# ---- qvit_quantize_act_i8, qvit_fake_quant_f32, qvit_gelu_quant_i8 -----------------------------------------------------
def _codes_entry(dev, ps, fn, want_fn):
    qt, d, qm, t, lv = _q(ps, dev)
    for cols, shift in ROW_CASES:
        sp, idx, clean, poisoned, allowed = _rows_case(ps, cols)
        kpad = _round_up(cols, 16)
        pad = torch.zeros((5, kpad), dtype=torch.bool)
        pad[:, :cols] = allowed
        outs = {}
        for name, x in (("clean", clean), ("poisoned", poisoned)):
            for flag in (0, _lib.QT_FORCE_CAREFUL):
                out = torch.full((5, kpad), 77, dtype=torch.int8, device=dev)
                fn(_device_rows(x, shift, dev), qt | flag, d, qm, t, lv, out, kpad)
                outs[name, flag] = out.cpu()
        what = f"{fn.__name__} {ps} cols {cols} shift {shift}"
        for name in ("clean", "poisoned"):
            S.assert_paths_equal({"fast": outs[name, 0], "careful": outs[name, _lib.QT_FORCE_CAREFUL]}, what + " " + name)
        got = outs["poisoned", 0][:, :cols].reshape(-1)[idx]
        S.assert_planted(got, want_fn(sp, ps), what)
        S.assert_contained(outs["clean", 0], outs["poisoned", 0], pad, what)
        assert bool((outs["poisoned", 0][:, cols:] == 0).all())
        yield sp, got


@ALL_SETS
def test_quantize_act_special_values(dev, ps):
    """NaN -> 0, +-Inf and +-FLT_MAX -> +-min(L, 127), +-0 and a quotient that rounds to 0 -> 0; fast == careful;
    vector, scalar and unaligned loads; nothing else changes. The tiny arm's codes are judged by the tie-proof
    machinery (their double-rounding mask is empty: tests/test_special_values_ref_cpu.py)."""
    for sp, got in _codes_entry(dev, ps, _lib.quantize_act_i8, S.expected_codes):
        assert_codes_tie_proven(got, V.device_codes(sp, *ps.args), V.double_rounding_mask(sp, *ps.args),
                                V.CAP_DOUBLE_ROUNDING)


@pytest.mark.parametrize("ps", S.SETS, ids=repr)
def test_gelu_quant_special_values(dev, ps):
    """codes = quantize(GELU(h)): gelu(NaN) and gelu(-Inf) = -Inf * 0 are NaN (code 0), gelu(+Inf) = +Inf (saturated);
    expected from O.gelu and the oracle quantizer."""
    for _ in _codes_entry(dev, ps, _lib.gelu_quant_i8, S.expected_gelu_codes):
        pass


@ALL_SETS
def test_fake_quant_special_values(dev, ps):
    """fp32 values as the reference returns them, NaN in -> NaN out (ULTRA_ACT: NaN -> 0, round(clamp(x) n) / n)."""
    qt, d, qm, t, lv = _q(ps, dev)
    for cols, shift in ROW_CASES:
        sp, idx, clean, poisoned, allowed = _rows_case(ps, cols)
        if ps.qt == V.ULTRA_ACT:
            want = S.expected_codes(sp, ps).float() / float(ps.levels)
        else:
            want = S.expected_fake_quant(sp, ps)
        outs = {}
        for name, x in (("clean", clean), ("poisoned", poisoned)):
            for flag in (0, _lib.QT_FORCE_CAREFUL):
                outs[name, flag] = _lib.fake_quant_f32(_device_rows(x, shift, dev).view(-1), qt | flag, d, qm, t, lv).cpu()
        what = f"fake_quant {ps} n {5 * cols} shift {shift}"
        for name in ("clean", "poisoned"):
            S.assert_paths_equal({"fast": outs[name, 0], "careful": outs[name, _lib.QT_FORCE_CAREFUL]}, what + " " + name)
        S.assert_planted(outs["poisoned", 0][idx], want, what)
        S.assert_contained(outs["clean", 0], outs["poisoned", 0], allowed.view(-1), what)


# ---- qvit_layernorm_quant_i8 / _t32 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("cols", [192, 1280, 770])
@OUT_SETS
def test_layernorm_special_values(dev, ps, cols, affine):
    """rows = 9 (three workgroups of four rows): a NaN in row 1 and a +Inf in row 6 make the row's mean, and with it
    every y of the row, NaN: the row's codes are all 0, with and without the code table; every other row is bit
    identical to the clean run. One width per dispatch arm (persistent, register, scalar), and the T32 store order."""
    rows = 9
    g = torch.Generator().manual_seed(cols)
    clean = torch.randn(rows, cols, generator=g) * 2 + 0.3
    poisoned = clean.clone()
    poisoned[1, 5] = NAN
    poisoned[6, cols - 3] = INF
    gamma = (torch.rand(cols, generator=g) + 0.5).to(dev) if affine else None
    beta = (torch.randn(cols, generator=g) * 0.1).to(dev) if affine else None
    qt, d, qm, t, lv = _q(ps, dev)
    table = _table(ps, False, dev)
    assert table is not None
    kpad = _round_up(cols, 64)
    allowed = S.rows_mask((rows, kpad), [1, 6])
    y = F.layer_norm(poisoned, (cols,), None if gamma is None else gamma.cpu(), None if beta is None else beta.cpu(), 1e-6)
    want = S.expected_codes(y[[1, 6]], ps)
    assert not want.any()                                            # NaN rows: every code 0

    def run(x, tab, t32=False):
        if t32:
            out = torch.full((_lib.t32_rows(rows) * kpad,), 93, dtype=torch.int8, device=dev)
            _lib.layernorm_quant_i8_t32(x.to(dev), gamma, beta, 1e-6, qt, d, qm, t, lv, out, kpad, code_table=tab)
            return _lib.t32_to_rows(out, rows, kpad).cpu()
        out = torch.full((rows, kpad), 77, dtype=torch.int8, device=dev)
        _lib.layernorm_quant_i8(x.to(dev), gamma, beta, 1e-6, qt, d, qm, t, lv, out, kpad, code_table=tab)
        return out.cpu()

    paths = {"direct": (None, False), "table": (table, False)}
    if cols == 192:
        paths.update({"t32-direct": (None, True), "t32-table": (table, True)})
    res = {name: (run(clean, *a), run(poisoned, *a)) for name, a in paths.items()}
    what = f"layernorm {ps} cols {cols}"
    S.assert_paths_equal({n: r[0] for n, r in res.items()}, what + " clean")
    S.assert_paths_equal({n: r[1] for n, r in res.items()}, what + " poisoned")
    for name, (c, p) in res.items():
        S.assert_planted(p[[1, 6], :cols], want, f"{what} {name}")
        S.assert_contained(c, p, allowed, f"{what} {name}")
        assert bool((p[:, cols:] == 0).all())


# ---- qvit_im2col_quant_i8 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [S.PSET["linear-L127"], S.PSET["nonlinear-t0.8"], S.PSET["ultra-levels15"]], ids=repr)
def test_im2col_special_values(dev, ps):
    """k3 s1 p1, C = 2, H = W = 6: one NaN pixel (a corner: 4 patches) and one +Inf pixel (9 patches); exactly the
    entries that tap them change, to 0 and to the saturation code."""
    B, C, H, W, k = 1, 2, 6, 6, 3
    clean = _clean((B, C, H, W), ps, seed=3)
    poisoned = clean.clone()
    poisoned[0, 1, 0, 0] = NAN
    poisoned[0, 0, 2, 3] = INF
    K, kpad = C * k * k, 32
    qt, d, qm, t, lv = _q(ps, dev)
    outs = {}
    for name, x in (("clean", clean), ("poisoned", poisoned)):
        for flag in (0, _lib.QT_FORCE_CAREFUL):
            out = torch.full((B * H * W, kpad), 77, dtype=torch.int8, device=dev)
            _lib.im2col_quant_i8(x.to(dev), k, k, 1, 1, 1, 1, 1, 1, qt | flag, d, qm, t, lv, out, kpad)
            outs[name, flag] = out.cpu()
    for name in ("clean", "poisoned"):
        S.assert_paths_equal({"fast": outs[name, 0], "careful": outs[name, _lib.QT_FORCE_CAREFUL]}, f"im2col {ps} {name}")
    nan_taps = S.im2col_taps(B, C, H, W, k, 1, 1, [(0, 1, 0, 0)])
    inf_taps = S.im2col_taps(B, C, H, W, k, 1, 1, [(0, 0, 2, 3)])
    assert int(nan_taps.sum()) == 4 and int(inf_taps.sum()) == 9
    allowed = torch.zeros((B * H * W, kpad), dtype=torch.bool)
    allowed[:, :K] = nan_taps | inf_taps
    got = outs["poisoned", 0]
    S.assert_contained(outs["clean", 0], got, allowed, f"im2col {ps}")
    code = S.expected_codes(torch.tensor([NAN, INF]), ps)
    S.assert_planted(got[:, :K][nan_taps], code[:1].expand(4), f"im2col {ps} NaN taps")
    S.assert_planted(got[:, :K][inf_taps], code[1:].expand(9), f"im2col {ps} Inf taps")
    assert bool((got[:, K:] == 0).all())


# ---- qvit_gemm ----------------------------------------------------------------------------------------------------------
D_ACT, D_WT = 0.02, 0.01
BIAS_COLS = [0, 255, 256]                  # NaN, +Inf, -Inf (255 | 256: the edge of the 256-column tile)


def _gemm_operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    bias = torch.randn(N, generator=g) * 0.3
    poisoned = bias.clone()
    poisoned[BIAS_COLS] = torch.tensor([NAN, INF, -INF])
    return a, w, bias, poisoned


def _formats(w, dev):
    p4, npad, kpad = pack_codes(w, _lib.W4, dev)
    p8, _, _ = pack_codes(w, _lib.W8, dev)
    return {_lib.W4: p4, _lib.W8: p8, _lib.W4R: _lib.pack_weight_w4r(p4, npad, kpad),
            _lib.W8R: _lib.pack_weight_w8r(p4, npad, kpad)}, npad, kpad


@pytest.mark.parametrize("K", [128, 384], ids=["K128", "K384-register-ring"])
@OUT_SETS
def test_gemm_int8_epilogues_special_bias(dev, ps, K):
    """M = 129, N = 257: a NaN, +Inf and -Inf bias entry change only their columns; there W4, W8, W4R and W8R, direct
    and through the code table, give the codes of the oracle (I8: 0, L, -L; I8_GELU: 0, L, 0)."""
    M, N = 129, 257
    a, w, bias, pbias = _gemm_operands(M, N, K, seed=K)
    fmts, npad, kpad = _formats(w, dev)
    A = a.to(torch.int8).to(dev)
    da, dw = _p(D_ACT, dev), _p(D_WT, dev)
    allowed = S.cols_mask((M, _round_up(N, 16)), BIAS_COLS)
    for gelu in (False, True):
        epi = _lib.EPI_I8_GELU if gelu else _lib.EPI_I8
        table = _table(ps, gelu, dev)
        assert table is not None
        sp = pbias[BIAS_COLS]
        want = (S.expected_gelu_codes if gelu else S.expected_codes)(sp, ps).unsqueeze(0).expand(M, 3)
        res = {}
        for wfmt, packed in fmts.items():
            for tab in (None, table):
                pair = []
                for b in (bias, pbias):
                    out = torch.full((M, _round_up(N, 16)), 99, dtype=torch.int8, device=dev)
                    _lib.gemm(A, M, kpad, packed, wfmt, N, npad, da, dw, _lib.pad_bias(b.to(dev), N, npad, dev), epi, out,
                              epi_table=tab, **_okw(ps, dev))
                    pair.append(out.cpu())
                res[f"wfmt{wfmt}-{'table' if tab is not None else 'direct'}"] = pair
        what = f"gemm {ps} K {K} gelu {gelu}"
        for name, (c, p) in res.items():
            S.assert_planted(p[:, BIAS_COLS], want, f"{what} {name}")
            S.assert_contained(c, p, allowed, f"{what} {name}")
            assert bool((p[:, N:] == 99).all())
        S.assert_paths_equal({n: r[1][:, BIAS_COLS].contiguous() for n, r in res.items()}, what + " poisoned columns")
        S.assert_paths_equal({n: r[1] for n, r in res.items() if n.endswith("direct")}, what + " direct")
        if not gelu:      # (the tabled GELU may take the neighbouring transition at a change point: assert_gelu_table_ties)
            S.assert_paths_equal({n: r[1] for n, r in res.items()}, what + " every path")


@pytest.mark.parametrize("K", [128, 384], ids=["K128", "K384-register-ring"])
def test_gemm_fp32_epilogues_special_bias(dev, K):
    """EPI_F32 / EPI_F32_RESID: the bias columns come out NaN, +Inf, -Inf and nothing else changes; a NaN in C[3, 7] of
    the residual stays that one element."""
    M, N = 129, 257
    a, w, bias, pbias = _gemm_operands(M, N, K, seed=K + 1)
    fmts, npad, kpad = _formats(w, dev)
    A = a.to(torch.int8).to(dev)
    da, dw = _p(D_ACT, dev), _p(D_WT, dev)
    ldc = _round_up(N, 4)
    c0 = torch.randn(M, ldc, generator=torch.Generator().manual_seed(5))
    c0p = c0.clone()
    c0p[3, 7] = NAN
    cols = S.cols_mask((M, ldc), BIAS_COLS)
    want = torch.tensor([NAN, INF, -INF]).unsqueeze(0).expand(M, 3)
    res = {}
    for wfmt, packed in fmts.items():
        for epi, name in ((_lib.EPI_F32, "f32"), (_lib.EPI_F32_RESID, "resid")):
            pair = []
            for b, c in ((bias, c0), (pbias, c0p)):
                out = c.clone().to(dev) if epi == _lib.EPI_F32_RESID else torch.full((M, ldc), 7.0, device=dev)
                _lib.gemm(A, M, kpad, packed, wfmt, N, npad, da, dw, _lib.pad_bias(b.to(dev), N, npad, dev), epi, out)
                pair.append(out.cpu())
            res[f"wfmt{wfmt}-{name}"] = pair
    for name, (c, p) in res.items():
        allowed = cols.clone()
        if name.endswith("resid"):
            allowed[3, 7] = True
            assert math.isnan(p[3, 7])
        S.assert_planted(p[:, BIAS_COLS], want, f"gemm {name} K {K}")
        S.assert_contained(c, p, allowed, f"gemm {name} K {K}")
    for name in ("f32", "resid"):
        S.assert_paths_equal({n: r[1] for n, r in res.items() if n.endswith(name)}, f"gemm {name} K {K} formats")


# ---- qvit_gemm_a32, qvit_gemm_resid_ln ------------------------------------------------------------------------------------
@OUT_SETS
def test_gemm_a32_special_bias(dev, ps):
    """The weight-stationary schedule (M = 65, N = 3072, K = 768): the same three bias columns, I8 and I8_GELU, direct
    and tabled; equal to qvit_gemm on the poisoned bias."""
    M, N, K = 65, 3072, 768
    a, w, bias, pbias = _gemm_operands(M, N, K, seed=9)
    packed, npad, kpad = pack_codes(w, _lib.W4, dev)
    A = a.to(torch.int8).to(dev)
    A32 = _lib.rows_to_t32(A, K)
    da, dw = _p(D_ACT / 4, dev), _p(D_WT, dev)
    allowed = S.cols_mask((M, N), BIAS_COLS)
    for gelu in (False, True):
        epi = _lib.EPI_I8_GELU if gelu else _lib.EPI_I8
        assert _lib.gemm_a32_fits(K, _lib.W4, N, N, epi)
        table = _table(ps, gelu, dev)
        want = (S.expected_gelu_codes if gelu else S.expected_codes)(pbias[BIAS_COLS], ps).unsqueeze(0).expand(M, 3)
        res = {}
        for tab in (None, table):
            pair = []
            for b in (bias, pbias):
                out = torch.full((M, N), 55, dtype=torch.int8, device=dev)
                _lib.gemm_a32(A32, M, K, packed, _lib.W4, N, npad, da, dw, _lib.pad_bias(b.to(dev), N, npad, dev), epi, out,
                              epi_table=tab, **_okw(ps, dev))
                pair.append(out.cpu())
            res["table" if tab is not None else "direct"] = pair
        tiles = torch.full((M, N), 77, dtype=torch.int8, device=dev)
        _lib.gemm(A, M, K, packed, _lib.W4, N, npad, da, dw, _lib.pad_bias(pbias.to(dev), N, npad, dev), epi, tiles,
                  **_okw(ps, dev))
        what = f"gemm_a32 {ps} gelu {gelu}"
        for name, (c, p) in res.items():
            S.assert_planted(p[:, BIAS_COLS], want, f"{what} {name}")
            S.assert_contained(c, p, allowed, f"{what} {name}")
        S.assert_paths_equal({"direct": res["direct"][1][:, BIAS_COLS].contiguous(),
                              "table": res["table"][1][:, BIAS_COLS].contiguous()}, what + " poisoned columns")
        S.assert_paths_equal({"gemm_a32": res["direct"][1], "gemm": tiles.cpu()}, what + " against qvit_gemm")


@OUT_SETS
def test_gemm_resid_ln_special_residual(dev, ps):
    """M = 129, N = 192: a NaN in one residual element stays that element of C and makes that row's LayerNorm codes
    the NaN-row codes (all 0), with and without ln_table; every other row of C and of the codes is bit identical."""
    M, N, K = 129, 192, 128
    g = torch.Generator().manual_seed(21)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    bias = torch.randn(N, generator=g) * 0.3
    gamma, beta = (torch.rand(N, generator=g) + 0.5).to(dev), (torch.randn(N, generator=g) * 0.1).to(dev)
    c0 = torch.randn(M, N, generator=g)
    c0p = c0.clone()
    c0p[70, 5] = NAN
    packed, npad, kpad = pack_codes(w, _lib.W4, dev)
    A = a.to(torch.int8).to(dev)
    da, dw = _p(D_ACT, dev), _p(D_WT, dev)
    bias_pad = _lib.pad_bias(bias.to(dev), N, npad, dev)
    qt, d, qm, t, lv = _q(ps, dev)
    table = _table(ps, False, dev)
    assert table is not None
    c_allowed = torch.zeros((M, N), dtype=torch.bool)
    c_allowed[70, 5] = True
    res = {}
    for tab in (None, table):
        pair = []
        for c in (c0, c0p):
            C = c.clone().to(dev)
            codes = torch.full((M, N), 55, dtype=torch.int8, device=dev)
            _lib.gemm_resid_ln(A, M, kpad, packed, _lib.W4, N, npad, da, dw, bias_pad, C, gamma, beta, 1e-6, qt, d, qm, t, lv,
                               tab, codes, N)
            torch.cuda.synchronize()
            pair.append((C.cpu(), codes.cpu()))
        res["table" if tab is not None else "direct"] = pair
    for name, ((cc, kc), (cp, kp)) in res.items():
        what = f"gemm_resid_ln {ps} {name}"
        assert math.isnan(cp[70, 5])
        S.assert_contained(cc, cp, c_allowed, what + " C")
        S.assert_contained(kc, kp, S.rows_mask((M, N), [70]), what + " codes")
        S.assert_planted(kp[70], torch.zeros(N, dtype=torch.int8), what + " NaN row")
    S.assert_paths_equal({n: r[1][1] for n, r in res.items()}, f"gemm_resid_ln {ps} codes")
    S.assert_paths_equal({n: r[1][0] for n, r in res.items()}, f"gemm_resid_ln {ps} C")


# ---- qvit_gemm_wonly ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [True, False], ids=["split-K-workspace", "no-split"])
@pytest.mark.parametrize("M", [5, 65])
def test_gemm_wonly_special_rows(dev, M, split):
    """fp32 X against int4 codes (N = 256, K = 256: two tiles at most, so split=True takes the split-K workspace): a
    NaN in row 1 and a +Inf in row 3 change only those rows of Y; the NaN row is NaN wherever the fp64 product is."""
    N, K = 256, 256
    g = torch.Generator().manual_seed(M)
    codes = torch.randint(-8, 8, (N, K), generator=g)
    x = torch.randn(M, K, generator=g)
    xp = x.clone()
    xp[1, 77] = NAN
    xp[3, 130] = INF
    bias = torch.randn(N, generator=g) * 0.1
    packed, npad, kpad = pack_codes(codes, _lib.W4, dev)
    bias_pad = _lib.pad_bias(bias.to(dev), N, npad, dev)
    ys = []
    for xx in (x, xp):
        y = torch.full((M, N), 3.0, device=dev)
        _lib.gemm_wonly(xx.to(dev), M, kpad, packed, _lib.W4, N, npad, _p(0.0123, dev), bias_pad, y, split=split)
        torch.cuda.synchronize()
        ys.append(y.cpu())
    S.assert_contained(ys[0], ys[1], S.rows_mask((M, N), [1, 3]), f"gemm_wonly M {M} split {split}")
    ref = xp.double() @ (0.0123 * codes.double()).t() + bias.double()
    assert bool(torch.isnan(ref[1]).all())
    assert torch.equal(torch.isnan(ys[1][1]), torch.isnan(ref[1]))


# ---- qvit_attention, qvit_attention_split -------------------------------------------------------------------------------
ATT_B, ATT_N, ATT_H = 2, 33, 2
ATT_BLOCKS = [(0, 1), (1, 0)]              # (image, head) holding the planted q and v elements


def _attention_case(hd, value):
    C = ATT_H * hd
    qkv = torch.randn(ATT_B * ATT_N, 3 * C, generator=torch.Generator().manual_seed(hd))
    p = qkv.clone()
    p[0 * ATT_N + 4, 1 * hd + 3] = value                      # q of image 0, head 1, query 4
    p[1 * ATT_N + 7, 2 * C + 0 * hd + 9] = value              # v of image 1, head 0, key 7
    return qkv, p, S.attention_blocks_mask(ATT_B, ATT_N, ATT_H, hd, ATT_BLOCKS)


def _planes(qkv, hd, dev):
    if hd == 80:
        from test_gpu_attention_split_hd80 import planes
        return planes(qkv, ATT_B, ATT_N, ATT_H, 1.0, dev)
    from test_gpu_attention import split_planes
    hi, lo = split_planes(qkv, ATT_B, ATT_N, ATT_H, 1.0)
    return hi.to(dev), lo.to(dev)


def _attend(dev, qkv, hd, entry, mode=_lib.ATT_F32, table=None, **kw):
    C = ATT_H * hd
    out = (torch.full((ATT_B * ATT_N, C), 7.0, device=dev) if mode == _lib.ATT_F32
           else torch.full((ATT_B * ATT_N, C), 99, dtype=torch.int8, device=dev))
    if entry == "attention":
        _lib.attention(qkv.to(dev), ATT_B, ATT_N, ATT_H, hd, hd ** -0.5, out, mode, 1.0, **kw)
    else:
        hi, lo = _planes(qkv, hd, dev)
        _lib.attention_split(hi, lo, ATT_B, ATT_N, ATT_H, hd, hd ** -0.5, out, mode, 1.0, epi_table=table, **kw)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("value", [NAN, INF, -INF], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("entry", ["attention", "attention_split"])
@pytest.mark.parametrize("hd", [64, 80])
def test_attention_fp32_special_values(dev, hd, entry, value):
    """B = 2, N = 33, H = 2, ATT_F32: a special value in one q element of (image 0, head 1) and one v element of
    (image 1, head 0) leaves the other (image, head) blocks bit identical. For a NaN the NaN positions inside the
    poisoned blocks equal those of the fp64 reference (the query's row; the v element's column). For +-Inf only
    the containment is asserted: inf - inf inside the softmax has no single right answer (DESIGN.md records what the
    kernels return)."""
    qkv, p, allowed = _attention_case(hd, value)
    clean, got = _attend(dev, qkv, hd, entry), _attend(dev, p, hd, entry)
    assert bool(torch.isfinite(clean).all())
    S.assert_contained(clean, got, allowed, f"{entry} hd {hd}")
    if math.isnan(value):
        ref = V.ref_attention(p, ATT_B, ATT_N, ATT_H, hd, hd ** -0.5)
        assert int(torch.isnan(ref).sum()) == hd + ATT_N
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), (
            f"{entry} hd {hd}: NaN at {int(torch.isnan(got).sum())} outputs, the fp64 reference at {int(torch.isnan(ref).sum())}")


@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "+inf"])
@OUT_SETS
def test_attention_int8_special_values(dev, ps, value):
    """head_dim 64, ATT_I8: the fp32-input kernel, and the split kernel direct and through the code table (byte for
    byte equal). A NaN output has code 0: the codes of the query's row and of the v element's column."""
    hd = 64
    qkv, p, allowed = _attention_case(hd, value)
    table = _table(ps, False, dev)
    assert table is not None
    kw = _okw(ps, dev)
    res = {}
    for name, entry, tab in (("fp32-input", "attention", None), ("split-direct", "attention_split", None),
                             ("split-table", "attention_split", table)):
        res[name] = (_attend(dev, qkv, hd, entry, _lib.ATT_I8, tab, **kw), _attend(dev, p, hd, entry, _lib.ATT_I8, tab, **kw))
    for name, (c, g) in res.items():
        S.assert_contained(c, g, allowed, f"attention int8 {ps} {name}")
        if math.isnan(value):
            nan = torch.isnan(V.ref_attention(p, ATT_B, ATT_N, ATT_H, hd, hd ** -0.5))
            S.assert_planted(g[nan], torch.zeros(int(nan.sum()), dtype=torch.int8), f"attention int8 {ps} {name}")
    S.assert_paths_equal({"direct": res["split-direct"][0], "table": res["split-table"][0]}, f"attention_split {ps} clean")
    S.assert_paths_equal({"direct": res["split-direct"][1], "table": res["split-table"][1]}, f"attention_split {ps} poisoned")


# ---- the code table itself ----------------------------------------------------------------------------------------------
def test_table_with_change_point_in_bucket0_is_rejected(dev):
    """A bucket 0 that holds a change point has no byte left for the code of a NaN: the device marks such a table
    invalid (the epilogues then evaluate directly), and the plan's geometry never builds one."""
    ps = LIN7
    qt, d, qm, t, _ = _q(ps, dev)
    w = 0.8 * ps.d
    v_lo = -6.5 * ps.d - 0.2 * w          # bucket 0 is [v_lo - w / 2, v_lo + w / 2): it holds the change point -6.5 d
    nb = int(math.ceil(-2 * v_lo / w)) + 3
    bad = _lib.epi_table_build(_lib.EPI_I8, qt, d, qm, t, 0, v_lo, w, nb, dev)
    good = _lib.epi_table_build(_lib.EPI_I8, qt, d, qm, t, 0, v_lo - w, w, nb + 1, dev)
    torch.cuda.synchronize()
    assert int(bad[12:16].view(torch.int32).item()) == 0
    assert int(good[12:16].view(torch.int32).item()) == 1


# ---- module level ---------------------------------------------------------------------------------------------------------
def test_quantize_linear_fake_quant_route_propagates_nan(dev):
    """A QuantizeLinear whose levels fit no packed format quantizes its activations with qvit_fake_quant_f32; under
    autograd a NaN in one input element makes the same outputs NaN as the CPU reference layer (its whole row)."""
    import test_gpu_layer_autograd as LA
    kind = LA.R.LINEAR
    layer, x, W, b, wq, aq = LA._build(dev, kind, "fp32")
    plan = layer.quant_plan()
    assert not plan.int_path and not plan.extra.get("wonly")
    x = x.clone()
    x[2, 5] = NAN
    q = O.LayerQ(O.LINEAR, O.WEIGHT_AND_ACTIVATION, wq[0], wq[1], 1.0, aq[0], aq[1], 1.0)
    ref = O.quantize_linear(x, W, b, q)
    assert bool(torch.isnan(ref[2]).all()) and int(torch.isnan(ref).sum()) == ref.shape[1]
    xd = x.to(dev).requires_grad_(True)
    y = layer(xd)
    assert y.requires_grad
    assert torch.equal(torch.isnan(y.detach().cpu()), torch.isnan(ref))
    keep = ~torch.isnan(ref)
    assert torch.allclose(y.detach().cpu()[keep], ref[keep], rtol=1e-4, atol=1e-4)
