"""GPU parity of the HIP kernels (through the C-ABI) against the CPU oracle.

Bars:
  * integer work (packing, MFMA accumulation, linear-quantizer codes): bit-exact;
  * nonlinear-quantizer codes (exp/log in fp32: ocml on the GPU vs the CPU's libm/Sleef): identical
    except at ulp-level rounding-boundary ties, bounded here at <= 1e-4 of elements, each off by 1;
  * fp32 epilogues: relative error <= 1e-6 against fp64 evaluation of the same integer result.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vit_codes_ref as V
from oracle import quant_oracle as O
from quantized_vit_amd import _lib
from ultra_ref import assert_codes_tie_proven

pytestmark = pytest.mark.gpu

QT = {O.LINEAR: _lib.QT_LINEAR, O.NONLINEAR: _lib.QT_NONLINEAR}


def _p(v, dev):
    return torch.tensor([float(v)], dtype=torch.float32, device=dev)


def _round_up(v, m):
    return (v + m - 1) // m * m


def pack_codes(codes_w: torch.Tensor, wfmt: int, dev):
    """Packs integer weight codes exactly (linear quantizer with d = 1, q_m large => code = w)."""
    n, k = codes_w.shape
    npad, kpad = _round_up(n, _lib.TILE_N), _round_up(k, _lib.TILE_K)
    w = codes_w.float().to(dev).contiguous()
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    packed = _lib.pack_weight(w, _lib.QT_LINEAR, _p(1.0, dev), _p(1000.0, dev), None, wfmt, npad, kpad, ovf)
    torch.cuda.synchronize()
    assert ovf.item() == 0
    return packed, npad, kpad


def act_buffer(codes_a: torch.Tensor, kpad: int, dev):
    m, k = codes_a.shape
    A = torch.zeros((m, kpad), dtype=torch.int8, device=dev)
    A[:, :k] = codes_a.to(torch.int8).to(dev)
    return A


SHAPES = [(1, 1, 1), (128, 128, 128), (300, 200, 200), (257, 2304, 768), (1576, 768, 192), (7, 15, 768),
          (33, 3072, 768), (129, 768, 3072), (64, 100, 1000)]


@pytest.mark.parametrize("wfmt", [_lib.W4, _lib.W8])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_int32_exact(dev, wfmt, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 13 + K)
    a = torch.randint(-127, 128, (M, K), generator=g)
    lim = 8 if wfmt == _lib.W4 else 128
    w = torch.randint(-lim, lim, (N, K), generator=g)
    packed, npad, kpad = pack_codes(w, wfmt, dev)
    A = act_buffer(a, kpad, dev)
    C = torch.full((M, _round_up(N, 4)), -7, dtype=torch.int32, device=dev)
    _lib.gemm(A, M, kpad, packed, wfmt, N, npad, None, None, None, _lib.EPI_I32, C)
    torch.cuda.synchronize()
    ref = O.int_accumulators(a.float(), w.float())
    assert torch.equal(C[:, :N].cpu().long(), ref)
    if C.shape[1] > N:
        assert (C[:, N:] == -7).all()   # nothing written past N


def test_gemm_extreme_values_exact(dev):
    M, N, K = 130, 256, 4096
    a = torch.full((M, K), -127)
    w = torch.full((N, K), -8)
    a[1::2] = 127
    w[1::3] = 7
    packed, npad, kpad = pack_codes(w, _lib.W4, dev)
    C = torch.empty((M, N), dtype=torch.int32, device=dev)
    _lib.gemm(act_buffer(a, kpad, dev), M, kpad, packed, _lib.W4, N, npad, None, None, None, _lib.EPI_I32, C)
    assert torch.equal(C.cpu().long(), O.int_accumulators(a.float(), w.float()))


@pytest.mark.parametrize("epi", [_lib.EPI_F32, _lib.EPI_F32_RESID])
def test_gemm_f32_epilogues(dev, epi):
    M, N, K = 515, 384, 768
    g = torch.Generator().manual_seed(5)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    bias = torch.randn(N, generator=g)
    packed, npad, kpad = pack_codes(w, _lib.W4, dev)
    d_a, d_w = 0.0123, 0.00457
    bias_pad = _lib.pad_bias(bias.to(dev), N, npad, dev)
    base = torch.randn(M, N, generator=g)
    C = base.clone().to(dev) if epi == _lib.EPI_F32_RESID else torch.empty((M, N), device=dev)
    _lib.gemm(act_buffer(a, kpad, dev), M, kpad, packed, _lib.W4, N, npad, _p(d_a, dev), _p(d_w, dev), bias_pad,
              epi, C)
    acc = O.int_accumulators(a.float(), w.float()).double()
    alpha = float(np.float32(d_a) * np.float32(d_w))
    ref = alpha * acc + bias.double()
    if epi == _lib.EPI_F32_RESID:
        ref = ref + base.double()
    err = (C.cpu().double() - ref).abs().max() / ref.abs().max()
    assert err < 1e-6, err


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("qt,t", [(O.LINEAR, 1.0), (O.NONLINEAR, 1.0), (O.NONLINEAR, 0.85)])
def test_gemm_int8_code_epilogue(dev, gelu, qt, t):
    M, N, K = 300, 640, 768
    g = torch.Generator().manual_seed(11)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    bias = torch.randn(N, generator=g) * 0.1
    packed, npad, kpad = pack_codes(w, _lib.W4, dev)
    d_a, d_w = 0.002, 0.0011
    bias_pad = _lib.pad_bias(bias.to(dev), N, npad, dev)
    dn, qmn = 0.9 / 127, 0.9
    out = torch.empty((M, _round_up(N, 16)), dtype=torch.int8, device=dev)
    _lib.gemm(act_buffer(a, kpad, dev), M, kpad, packed, _lib.W4, N, npad, _p(d_a, dev), _p(d_w, dev), bias_pad,
              _lib.EPI_I8_GELU if gelu else _lib.EPI_I8, out, out_qtype=QT[qt], out_d=_p(dn, dev),
              out_qm=_p(qmn, dev), out_t=_p(t, dev) if qt == O.NONLINEAR else None)
    # reference: fp32 epilogue value, torch GELU (erf), oracle quantizer codes
    acc = O.int_accumulators(a.float(), w.float()).float()
    v = (torch.tensor(d_a, dtype=torch.float32) * torch.tensor(d_w, dtype=torch.float32)) * acc + bias
    if gelu:
        v = F.gelu(v)
    ref = O.quant_codes(v, qt, dn, qmn, t)
    got = out[:, :N].cpu().float()
    diff = (got - ref).abs()
    assert diff.max() <= 1
    # the fp32 epilogue value itself differs by ulps (fma vs mul+add, erf implementation), so
    # boundary ties may flip; require them to be rare
    assert (diff > 0).float().mean() <= 2e-4
    # and every differing code is a proven tie of the fp64 value (vit_codes_ref: delta derived, not measured)
    c = V.gemm_code_case(gelu, qt, t)
    assert torch.equal(c.a, a) and torch.equal(c.w, w) and torch.equal(c.bias, bias)
    assert_codes_tie_proven(out[:, :N], c.ref, c.tie, c.cap)


def _epi_gemm(dev, gelu, qt, t, table_mode, M=4096, N=768, K=256, seed=5, dn=1.4 / 127, qmn=1.4):
    """int8-code epilogue on random codes; table_mode: None (direct), "auto" (the plan geometry) or
    "bad" (a table whose range is far too narrow -> must be rejected on the device)."""
    from quantized_vit_amd.quant_layers import epilogue_table_geometry, saturation_level
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    bias = torch.randn(N, generator=g) * 0.5
    packed, npad, kpad = pack_codes(w, _lib.W4, dev)
    bias_pad = _lib.pad_bias(bias.to(dev), N, npad, dev)
    qtc = QT[qt]
    tt = t if qt == O.NONLINEAR else 1.0
    if qt == O.NONLINEAR:
        dn = qmn ** t / 127
    epi = _lib.EPI_I8_GELU if gelu else _lib.EPI_I8
    kw = dict(out_qtype=qtc, out_d=_p(dn, dev), out_qm=_p(qmn, dev), out_t=_p(t, dev) if qt == O.NONLINEAR else None)
    table = None
    if table_mode is not None:
        L = saturation_level(qtc, dn, qmn, tt)
        geo = epilogue_table_geometry(qtc, dn, qmn, tt, L, gelu)
        assert geo is not None
        if table_mode == "bad":
            geo = (-0.01, geo[1], 4)
        table = _lib.epi_table_build(epi, qtc, kw["out_d"], kw["out_qm"], kw["out_t"], 0, *geo, dev)
    out = torch.empty((M, N), dtype=torch.int8, device=dev)
    _lib.gemm(act_buffer(a, kpad, dev), M, kpad, packed, _lib.W4, N, npad, _p(0.004, dev), _p(0.0011, dev),
              bias_pad, epi, out, epi_table=table, **kw)
    torch.cuda.synchronize()
    valid = None if table is None else int(table[12:16].view(torch.int32).item())
    return out.cpu(), valid


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("qt,t", [(O.LINEAR, 1.0), (O.NONLINEAR, 1.0), (O.NONLINEAR, 0.8), (O.NONLINEAR, 1.25)])
def test_epilogue_code_table_equals_direct(dev, gelu, qt, t):
    """The table-driven int8 epilogue re-expresses the per-element one (3.1 M codes spanning the
    quantizer's whole range, both signs, saturation). The fp32 GELU is monotone only up to rounding:
    where it zig-zags by an ulp across a change point, bisection picks one of the adjacent transitions,
    so a code may differ at such a point (measured: 0-4 in 3.1 M) — the same tie-level class as the
    GPU-vs-CPU bar (2e-4 against the oracle); bound it at 1e-5 of codes, off by one."""
    direct, _ = _epi_gemm(dev, gelu, qt, t, None)
    tabled, valid = _epi_gemm(dev, gelu, qt, t, "auto")
    assert valid == 1
    assert len(torch.unique(direct)) > 100 or not gelu
    d = (direct.to(torch.int32) - tabled.to(torch.int32)).abs()
    assert d.max().item() <= 1
    assert (d > 0).float().mean().item() <= 1e-5
    c = V.epi_gemm_case(gelu, qt, t)          # the direct run against the fp64 value: only proven ties may differ
    assert_codes_tie_proven(direct, c.ref, c.tie, c.cap)


def test_epilogue_code_table_rejected_when_invalid(dev):
    direct, _ = _epi_gemm(dev, True, O.NONLINEAR, 1.0, None)
    tabled, valid = _epi_gemm(dev, True, O.NONLINEAR, 1.0, "bad")
    assert valid == 0
    assert torch.equal(direct, tabled)


def _quant_inputs(g, n=300_000, scale=0.6):
    x = torch.randn(n, generator=g) * scale
    x[:1000] = 0.0
    x[1000:2000] = (torch.arange(-500, 500, dtype=torch.float32) + 0.5) * 0.01   # near/at ties
    return x


@pytest.mark.parametrize("qt,d,qm,t", [(O.LINEAR, 0.01, 1.0, 1.0), (O.LINEAR, 1 / 127, 1.0, 1.0),
                                       (O.NONLINEAR, 0.01, 1.0, 1.0), (O.NONLINEAR, 0.02, 1.5, 0.9),
                                       (O.NONLINEAR, 0.005, 0.6, 1.25), (O.LINEAR, 0.05, -0.5, 1.0)])
def test_quantize_act_codes_vs_oracle(dev, qt, d, qm, t):
    g = torch.Generator().manual_seed(3)
    x = _quant_inputs(g)
    rows, cols = 600, 500
    x2 = x.view(rows, cols)
    kpad = 512
    tt = _p(t, dev) if qt == O.NONLINEAR else None
    fast = torch.empty((rows, kpad), dtype=torch.int8, device=dev)
    careful = torch.empty_like(fast)
    _lib.quantize_act_i8(x2.to(dev), QT[qt], _p(d, dev), _p(qm, dev), tt, 0, fast, kpad)
    _lib.quantize_act_i8(x2.to(dev), QT[qt] | _lib.QT_FORCE_CAREFUL, _p(d, dev), _p(qm, dev), tt, 0, careful, kpad)
    fast, careful = fast.cpu(), careful.cpu()
    assert torch.equal(fast, careful), "guarded fast path must equal the careful path bit for bit"
    assert (fast[:, cols:] == 0).all()
    ref = O.quant_codes(x2, qt, d, qm, t)
    got = fast[:, :cols].float()
    if qt == O.LINEAR:
        assert torch.equal(got, ref)
    else:
        diff = (got - ref).abs().reshape(-1)
        assert diff.max() <= 1
        # random inputs: exp/log are rounded from double on the device, as torch's CPU kernels
        # are for >99.7% of inputs, so flips need both a non-CR CPU result and a near tie
        rand_flips = (diff[2000:] > 0).float().mean().item()
        tie_flips = (diff[1000:2000] > 0).float().mean().item()
        print(f"nonlinear flips: random {rand_flips:.2e}, crafted ties {tie_flips:.2e}")
        assert rand_flips <= 1e-5
        assert tie_flips <= 0.02


@pytest.mark.parametrize("qt,t", [(O.LINEAR, 1.0), (O.NONLINEAR, 1.0), (O.NONLINEAR, 0.7)])
def test_fake_quant_values_vs_oracle(dev, qt, t):
    g = torch.Generator().manual_seed(4)
    x = _quant_inputs(g, 100_000)
    d, qm = 0.013, 1.1
    y = _lib.fake_quant_f32(x.to(dev), QT[qt], _p(d, dev), _p(qm, dev), _p(t, dev) if qt == O.NONLINEAR else None)
    ref = O.fake_quant(x, qt, d, qm, t)
    if qt == O.LINEAR:
        assert torch.equal(y.cpu(), ref)
    else:
        assert ((y.cpu() - ref).abs() > 0).float().mean() <= 1e-4


def test_pack_weight_overflow_flag(dev):
    w = torch.linspace(-1, 1, 128 * 128, device=dev).view(128, 128).contiguous()
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.pack_weight(w, _lib.QT_LINEAR, _p(1 / 8, dev), _p(1.0, dev), None, _lib.W4, 256, 128, ovf)
    assert ovf.item() == 1          # level 8 does not fit int4
    ovf.zero_()
    _lib.pack_weight(w, _lib.QT_LINEAR, _p(1 / 7, dev), _p(1.0, dev), None, _lib.W4, 256, 128, ovf)
    assert ovf.item() == 0


# patch embeddings (k = s: 16 @224 and @384, 8 with 4 trailing pixels past the last patch, 4) and padded /
# strided / 1x1 convolutions
@pytest.mark.parametrize("conv", [dict(k=16, s=16, p=0, C=3, H=224), dict(k=3, s=1, p=1, C=16, H=20),
                                  dict(k=3, s=2, p=1, C=5, H=17), dict(k=1, s=1, p=0, C=64, H=13),
                                  dict(k=16, s=16, p=0, C=3, H=384), dict(k=8, s=8, p=0, C=2, H=44),
                                  dict(k=4, s=4, p=0, C=8, H=20)])
def test_im2col_quant_vs_oracle(dev, conv):
    g = torch.Generator().manual_seed(6)
    B = 2
    x = torch.randn(B, conv["C"], conv["H"], conv["H"], generator=g) * 0.5
    d, qm = 1.0 / 127, 1.0
    k, s, p = conv["k"], conv["s"], conv["p"]
    K = conv["C"] * k * k
    kpad = _round_up(K, 128)
    OH = (conv["H"] + 2 * p - k) // s + 1
    out = torch.empty((B * OH * OH, kpad), dtype=torch.int8, device=dev)
    _lib.im2col_quant_i8(x.to(dev), k, k, s, s, p, p, 1, 1, _lib.QT_LINEAR, _p(d, dev), _p(qm, dev), None, 0, out,
                         kpad)
    codes = O.quant_codes(x, O.LINEAR, d, qm)
    ref = F.unfold(codes, k, padding=p, stride=s).transpose(1, 2).reshape(B * OH * OH, K)
    got = out.cpu()
    assert torch.equal(got[:, :K].float(), ref)
    assert (got[:, K:] == 0).all()


# Every arm of qvit_layernorm_quant_i8's host dispatch (quant_kernels.hip), named with the width that selects it:
#   layernorm_quant_persist_kernel<NV>  cols % 4 == 0, ldx % 4 == 0, 16-B aligned x / gamma / beta, cols <= 1024
#   layernorm_quant_reg_kernel<8>       the same with cols in 1025 .. 2048
#   layernorm_quant_kernel (scalar)     everything else
# (cols, ldx or None for contiguous, operand shifted by 4 bytes or None)
LN_ARMS = {
    "persist<1>-cols192": (192, None, None),
    "persist<2>-cols384": (384, None, None),
    "persist<3>-cols768": (768, None, None),
    "persist<4>-cols1000": (1000, None, None),
    "reg<8>-cols1280": (1280, None, None),
    "reg<8>-cols2048": (2048, None, None),
    "scalar-cols2052-wider-than-2048": (2052, None, None),
    "scalar-cols770-not-multiple-of-4": (770, None, None),
    "scalar-cols1": (1, None, None),
    "scalar-cols768-ldx771": (768, 771, None),
    "scalar-cols768-x-offset-4B": (768, None, "x"),
    "scalar-cols768-gamma-offset-4B": (768, None, "gamma"),
}
LN_ROWS = [1, 5, 333]


def _shift4(t, dev):
    """t on the device at an address 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev)
    off = ((16 - buf.data_ptr() % 16) % 16) // 4 + 1
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _ln_operands(dev, x, gamma, beta, ldx, shift):
    rows, cols = x.shape
    if ldx is not None:
        full = torch.full((rows, ldx), float("nan"), device=dev)
        full[:, :cols] = x.to(dev)
        xd = full[:, :cols]
    else:
        xd = _shift4(x, dev) if shift == "x" else x.to(dev)
    gd = None if gamma is None else (_shift4(gamma, dev) if shift == "gamma" else gamma.to(dev))
    bd = None if beta is None else beta.to(dev)
    return xd, gd, bd


def _ln_ref64(x, gamma, beta, qt, d, qm, t):
    y = F.layer_norm(x.double(), (x.shape[1],), None if gamma is None else gamma.double(),
                     None if beta is None else beta.double(), 1e-6)
    return O.quant_codes(y.float(), qt, d, qm, t if qt == O.NONLINEAR else None)


@pytest.mark.parametrize("affine", [True, False], ids=["gamma-beta", "null-gamma-beta"])
@pytest.mark.parametrize("qt", [O.LINEAR, O.NONLINEAR])
@pytest.mark.parametrize("arm", list(LN_ARMS))
def test_layernorm_quant_vs_oracle(dev, arm, qt, affine):
    """Random rows through every dispatch arm against F.layer_norm in fp64 + O.quant_codes, rows in {1, 5, 333}
    (four rows per workgroup), gamma / beta given or both NULL. Bar: every code within 1, differing codes <= 5e-4
    of the 339 x cols codes of the three row counts together.

    The bar is a cap, not a measurement: the fp32 reference alone (F.layer_norm in fp32 against fp64 through the same
    quantizer, on the CPU, these inputs) differs in a share of 1.5e-5 of the codes at cols 192, 3e-6 at 1000 and 2048
    and in none at 384, 768, 1280, 2052, 770 and 1 (with gamma / beta; none anywhere with both NULL; the same for the
    linear and the nonlinear quantizer), never by more than 1."""
    cols, ldx, shift = LN_ARMS[arm]
    g = torch.Generator().manual_seed(8 + cols)
    gamma = (torch.rand(cols, generator=g) + 0.5) if affine else None
    beta = (torch.randn(cols, generator=g) * 0.1) if affine else None
    d, qm, t = 4.0 / 127, 4.0, 1.0
    kpad = _round_up(cols, 128)
    flips = total = 0
    ps = V._qset(qt, d, qm, t)
    gots, refs, ties, need = [], [], [], 0.0
    for rows in LN_ROWS:
        x = torch.randn(rows, cols, generator=g) * 2 + 0.3
        xd, gd, bd = _ln_operands(dev, x, gamma, beta, ldx, shift)
        out = torch.full((rows, kpad), 77, dtype=torch.int8, device=dev)
        _lib.layernorm_quant_i8(xd, gd, bd, 1e-6, QT[qt], _p(d, dev), _p(qm, dev),
                                _p(t, dev) if qt == O.NONLINEAR else None, 0, out, kpad)
        got = out.cpu()
        diff = (got[:, :cols].float() - _ln_ref64(x, gamma, beta, qt, d, qm, t)).abs()
        assert diff.max() <= 1, rows
        assert (got[:, cols:] == 0).all()
        flips += int((diff > 0).sum())
        total += diff.numel()
        ref, tie = V.ln_ties(x, gamma, beta, ps)
        need = max(need, V.ln_needed_c(x, gamma, beta, ps, got[:, :cols]))
        gots.append(got[:, :cols].reshape(-1)), refs.append(ref.reshape(-1)), ties.append(tie.reshape(-1))
    assert flips <= 5e-4 * total, (flips, total)
    # every differing code is a possible tie within C_LN e32(row) of the fp64 value; `need` is the smallest C that
    # would do for this arm (DESIGN.md section 16 records the figures; above 16 is a bug, not a bound to widen)
    print(f"layernorm {arm} {qt} affine {affine}: smallest sufficient C = {need:.3f} (C_LN = {V.C_LN})")
    assert need <= 16
    assert_codes_tie_proven(torch.cat(gots), torch.cat(refs), torch.cat(ties), V.CAP_LN)


def ln_stress_rows(cols, g):
    """Rows that separate a two-pass LayerNorm from a one-pass one: a constant row (variance 0: eps alone sets the
    scale, y = beta exactly: 3.0 sums exactly in fp32 in any order) and, for even cols, a row of mean 1e3 and
    standard deviation 1e-2 (half the columns 1000.01, half 999.99, shuffled)."""
    rows = [torch.full((cols,), 3.0)]
    if cols % 2 == 0:
        r = torch.full((cols,), 1000.01)
        r[torch.randperm(cols, generator=g)[:cols // 2]] = 999.99
        rows.append(r)
    return torch.stack(rows)


@pytest.mark.parametrize("affine", [True, False], ids=["gamma-beta", "null-gamma-beta"])
@pytest.mark.parametrize("qt", [O.LINEAR, O.NONLINEAR])
@pytest.mark.parametrize("arm", list(LN_ARMS))
def test_layernorm_quant_stress_rows(dev, arm, qt, affine):
    """The statistics under stress, through every dispatch arm. In fp32 the mean of the 1e3 +- 1e-2 row is off by up
    to about ulp(1e3 cols) / cols = 1e-4, i.e. 1e-2 of a standard deviation, so against ordinary quantizer steps no
    fp32 LayerNorm meets the 5e-4 cap on it. The step is therefore chosen so that it does: with d = 1 / 3 and gamma
    = 2, beta = 1 (or NULL) the normalized values -1 / +1 give y in {-1, 3} (or {-1, 1}), codes 3 d^-1 y at the
    centre of their bins, half a step (0.17) from a boundary. Measured on the CPU: fp32 F.layer_norm against fp64
    through O.quant_codes differs in 0 of these codes at every width. Bar: the same as for random rows (<= 1 off,
    <= 5e-4 differing, so none of these few). A one-pass variance (E[x^2] - mean^2: 1e6 known to 6e-2 against a
    variance of 1e-4) lands codes 2 or more off."""
    cols, ldx, shift = LN_ARMS[arm]
    g = torch.Generator().manual_seed(80 + cols)
    x = ln_stress_rows(cols, g)
    gamma = torch.full((cols,), 2.0) if affine else None
    beta = torch.full((cols,), 1.0) if affine else None
    d, qm, t = 1.0 / 3, 4.0, 1.0
    kpad = _round_up(cols, 128)
    xd, gd, bd = _ln_operands(dev, x, gamma, beta, ldx, shift)
    out = torch.full((x.shape[0], kpad), 77, dtype=torch.int8, device=dev)
    _lib.layernorm_quant_i8(xd, gd, bd, 1e-6, QT[qt], _p(d, dev), _p(qm, dev),
                            _p(t, dev) if qt == O.NONLINEAR else None, 0, out, kpad)
    got = out.cpu()
    ref = _ln_ref64(x, gamma, beta, qt, d, qm, t)
    assert len(torch.unique(ref)) == (1 if cols % 2 else 3)
    diff = (got[:, :cols].float() - ref).abs()
    assert diff.max() <= 1
    assert (diff > 0).float().mean() <= 5e-4
    assert (got[:, cols:] == 0).all()


# persist<3>, <1>, <4>; persist<2> (cols 257 .. 512: ViT-Small's 384) with many and with few rows; reg<8> (cols 1280)
# and the scalar kernel (cols 770), which take no table: one passed to them must change nothing
@pytest.mark.parametrize("cols,rows", [(768, 20000), (192, 40000), (1000, 3000), (768, 7), (384, 20000), (384, 6),
                                       (1280, 300), (770, 5)])
@pytest.mark.parametrize("qt,t", [(O.LINEAR, 1.0), (O.NONLINEAR, 1.0), (O.NONLINEAR, 0.8)])
def test_layernorm_quant_code_table_equals_direct(dev, cols, rows, qt, t):
    """The persistent LayerNorm kernel quantizing through the code table writes exactly the codes of the
    per-element quantizer (several rows per wave: rows > 8 x 4 x CUs for the larger cases), also on rows with
    ldx = cols + 4 and NaN in the pad columns; the arms without a table path ignore the table."""
    from quantized_vit_amd.quant_layers import epilogue_table_geometry, saturation_level
    g = torch.Generator().manual_seed(cols + rows)
    x = (torch.randn(rows, cols, generator=g) * 2 + 0.3).to(dev)
    gamma = (torch.rand(cols, generator=g) + 0.5).to(dev)
    beta = (torch.randn(cols, generator=g) * 0.1).to(dev)
    qm = 3.0
    d = qm / 127 if qt == O.LINEAR else qm ** t / 127
    qtc = _lib.QT_LINEAR if qt == O.LINEAR else _lib.QT_NONLINEAR
    tt = _p(t, dev) if qt == O.NONLINEAR else None
    geo = epilogue_table_geometry(qtc, d, qm, t, saturation_level(qtc, d, qm, t), False)
    table = _lib.epi_table_build(_lib.EPI_I8, qtc, _p(d, dev), _p(qm, dev), tt, 0, *geo, dev)
    assert int(table[12:16].view(torch.int32).item()) == 1
    kpad = _round_up(cols, 128)
    outs = []
    for tab in (None, table):
        out = torch.full((rows, kpad), 77, dtype=torch.int8, device=dev)
        _lib.layernorm_quant_i8(x, gamma, beta, 1e-6, qtc, _p(d, dev), _p(qm, dev), tt, 0, out, kpad,
                                code_table=tab)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    wide = torch.full((rows, cols + 4), float("nan"), device=dev)
    wide[:, :cols] = x
    out = torch.full((rows, kpad), 77, dtype=torch.int8, device=dev)
    _lib.layernorm_quant_i8(wide[:, :cols], gamma, beta, 1e-6, qtc, _p(d, dev), _p(qm, dev), tt, 0, out, kpad,
                            code_table=table)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], out.cpu()), "ldx > cols with the code table"
    assert (outs[1][:, cols:] == 0).all()
    ref = O.quant_codes(F.layer_norm(x[:50].cpu(), (cols,), gamma.cpu(), beta.cpu(), 1e-6), qt, d, qm,
                        t if qt == O.NONLINEAR else None)
    diff = (outs[1][:50, :cols].float() - ref).abs()
    assert diff.max() <= 1 and (diff > 0).float().mean() <= 5e-4
