"""Footprint of the output-writing entry points of include/qvit_hip.h: each runs once *embedded* in a poisoned
arena (tests/footprint_tools.py: leading dimensions larger than the width, poisoned pad columns and guard rows,
bases 16-byte but not 32-byte aligned) and once *tight* (fresh contiguous tensors, as every other test calls it).

Asserted per case: (a) no byte outside the documented output changed; (b) the embedded result equals the tight
one bit for bit; (c) the embedded result meets the oracle / fp64 reference at the bar of that kernel's own test
(test_gpu_kernels.py, test_gpu_wonly.py, test_gpu_gemm_ws.py, test_gpu_attention.py, test_gpu_ultranet.py): integer results exact, fp32 epilogues 1e-6 relative
to the fp64 evaluation, nonlinear codes off by at most one in at most the stated share. An over-read (pad columns
[K, lda), [cols, ldx)) pulls NaN / garbage codes into the result and fails (b) and (c).

Tile sizes read from the code: gemm_w4a8.hip BM = 128 rows x BN = 256 weight rows x BK = 64 (K granularity 128;
the register-weight formats take the two-ahead activation ring from K / BK >= 4, i.e. K >= 256); gemm_ws.hip and
the T32 layout: 64-row wave tiles; the row quantizers: 4 rows (waves) per workgroup; gemm_wonly.hip: 64-row tiles.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import quant_backward_ref as R
from footprint_tools import Arena, pack_codes, round_up as _round_up, scalar as _p
from oracle import quant_oracle as O
from quantized_vit_amd import _lib

pytestmark = pytest.mark.gpu

BM = 128
MB = 1 << 20


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _ok(code, what):
    assert code == 0, f"{what}: status {code}"


# ---- qvit_gemm ------------------------------------------------------------------------------------------
GEMM_M = [1, BM - 1, BM + 1, 2 * BM + 2]
GEMM_N = [1, 200, 257]
QM, QT_T = 1.4, 0.85
QD = QM ** QT_T / 127
_case_cache = {}


def _gemm_data(K, lim=7):
    """lim: 7 for the int4 images (W4, and W4R / W8R, which are built from a W4 image), 127 for W8."""
    if (K, lim) not in _case_cache:
        g = torch.Generator().manual_seed(1000 + K + lim)
        a = torch.randint(-127, 128, (max(GEMM_M), K), generator=g)
        w = torch.randint(-lim, lim + 1, (max(GEMM_N), K), generator=g)
        bias = torch.randn(max(GEMM_N), generator=g) * 0.3
        base = torch.randn(max(GEMM_M), max(GEMM_N), generator=g)
        _case_cache[(K, lim)] = (a, w, bias, base, O.int_accumulators(a.float(), w.float()))
    return _case_cache[(K, lim)]


def _pack(w, wfmt, dev):
    base_fmt = _lib.W8 if wfmt == _lib.W8 else _lib.W4
    packed, npad, kpad = pack_codes(w, base_fmt, dev)
    if wfmt == _lib.W4R:
        packed = _lib.pack_weight_w4r(packed, npad, kpad)
    elif wfmt == _lib.W8R:
        packed = _lib.pack_weight_w8r(packed, npad, kpad)
    return packed, npad, kpad


def _table(dev, epi, gelu):
    from quantized_vit_amd.quant_layers import epilogue_table_geometry, saturation_level
    qtc = _lib.QT_NONLINEAR
    geo = epilogue_table_geometry(qtc, QD, QM, QT_T, saturation_level(qtc, QD, QM, QT_T), gelu)
    assert geo is not None
    tab = _lib.epi_table_build(epi, qtc, _p(QD, dev), _p(QM, dev), _p(QT_T, dev), 0, *geo, dev)
    assert int(tab[12:16].view(torch.int32).item()) == 1
    return tab


EPIS = ["i32", "f32", "f32_resid", "i8", "i8_table", "i8_gelu", "i8_gelu_table"]
WFMTS = {"W4": _lib.W4, "W8": _lib.W8, "W4R": _lib.W4R, "W8R": _lib.W8R}


@pytest.mark.parametrize("epi_name", EPIS)
@pytest.mark.parametrize("K", [128, 384], ids=["K128_one_ahead", "K384_two_ahead_for_register_weights"])
@pytest.mark.parametrize("wname", list(WFMTS))
def test_gemm_embedded(dev, wname, K, epi_name):
    """M in {1, BM - 1, BM + 1, 2 BM + 2} x N in {1, 200, 257} (N < npad, a second N tile, N % 4 != 0 with ldc
    rounded up), lda = K + 16, ldc = N rounded up to the alignment unit plus one unit. The int8-code share bar
    (2e-4, test_gemm_int8_code_epilogue) is taken over the 235 870 codes of the twelve shapes together. The fp32 bar
    of test_gemm_f32_epilogues (max error 1e-6 of max |ref|) means little for a 1 x 1 result, so every element must
    also lie within 1e-6 of the magnitude of its terms |alpha acc| + |bias| (+ |base|): the fused multiply-add and
    the residual add round twice, 2 x 2^-24 = 1.2e-7 of that magnitude."""
    wfmt = WFMTS[wname]
    lim = 127 if wfmt == _lib.W8 else 7
    a_all, w_all, bias_all, base_all, acc_all = _gemm_data(K, lim)
    epi = {"i32": _lib.EPI_I32, "f32": _lib.EPI_F32, "f32_resid": _lib.EPI_F32_RESID}.get(
        epi_name, _lib.EPI_I8_GELU if "gelu" in epi_name else _lib.EPI_I8)
    i8 = epi_name.startswith("i8")
    cdt = torch.int8 if i8 else (torch.int32 if epi == _lib.EPI_I32 else torch.float32)
    unit = 16 if i8 else 4
    d_a = 0.01
    # |a| ~ 73, |w| ~ 0.58 lim per term: alpha acc has a standard deviation of 0.5, the quantizer's range
    d_w = 0.5 / (73.3 * 0.583 * (lim + 0.5) * math.sqrt(K)) / d_a
    alpha32 = torch.tensor(d_a, dtype=torch.float32) * torch.tensor(d_w, dtype=torch.float32)
    kw = {}
    if i8:
        kw = dict(out_qtype=_lib.QT_NONLINEAR, out_d=_p(QD, dev), out_qm=_p(QM, dev), out_t=_p(QT_T, dev))
        if "table" in epi_name:
            kw["epi_table"] = _table(dev, epi, "gelu" in epi_name)
    da_t, dw_t = (None, None) if epi == _lib.EPI_I32 else (_p(d_a, dev), _p(d_w, dev))
    flips = total = 0
    for N in GEMM_N:
        packed, npad, kpad = _pack(w_all[:N], wfmt, dev)
        assert kpad == K
        bias = bias_all[:N]
        for M in GEMM_M:
            a, acc = a_all[:M], acc_all[:M, :N]
            base = base_all[:M, :N]
            ldc = _round_up(N, unit) + unit
            ar = Arena(dev, 2 * MB)
            A = ar.put(a.to(torch.int8).to(dev), ld=K + 16, name="A")
            bias_pad = ar.put(_lib.pad_bias(bias.to(dev), N, npad, dev), name="bias")
            C = ar.carve(M, N, ldc, cdt, writable=True, name="C")
            if epi == _lib.EPI_F32_RESID:
                C.copy_(base.to(dev))
            ar.seal()
            _lib.gemm(A, M, K, packed, wfmt, N, npad, da_t, dw_t, None if epi == _lib.EPI_I32 else bias_pad, epi, C, **kw)
            torch.cuda.synchronize()
            ar.assert_untouched()                                            # (a)
            # tight
            At = a.to(torch.int8).to(dev).contiguous()
            Ct = torch.full((M, _round_up(N, unit)), 7, dtype=cdt, device=dev)
            if epi == _lib.EPI_F32_RESID:
                Ct[:, :N] = base.to(dev)
            _lib.gemm(At, M, K, packed, wfmt, N, npad, da_t, dw_t,
                      None if epi == _lib.EPI_I32 else _lib.pad_bias(bias.to(dev), N, npad, dev), epi, Ct, **kw)
            torch.cuda.synchronize()
            got = C.cpu()
            if cdt == torch.float32:
                assert torch.equal(got.view(torch.int32), Ct[:, :N].cpu().view(torch.int32)), (M, N)   # (b)
            else:
                assert torch.equal(got, Ct[:, :N].cpu()), (M, N)                                       # (b)
            # (c)
            if epi == _lib.EPI_I32:
                assert torch.equal(got.long(), acc), (M, N)
            elif not i8:
                ref = float(alpha32) * acc.double() + bias.double()
                mag = float(alpha32) * acc.double().abs() + bias.double().abs()
                if epi == _lib.EPI_F32_RESID:
                    ref, mag = ref + base.double(), mag + base.double().abs()
                err = (got.double() - ref).abs()
                assert (err <= 1e-6 * mag).all(), (M, N, float((err / mag).max()))
                if M * N >= 1000:
                    assert err.max() / ref.abs().max() < 1e-6, (M, N)
            else:
                v = alpha32 * acc.float() + bias
                if "gelu" in epi_name:
                    v = F.gelu(v)
                ref = O.quant_codes(v, O.NONLINEAR, QD, QM, QT_T)
                diff = (got.float() - ref).abs()
                assert diff.max() <= 1, (M, N)
                flips += int((diff > 0).sum())
                total += diff.numel()
    if i8:
        print(f"{wname} K={K} {epi_name}: {flips} of {total} codes off by one")
        assert flips <= 2e-4 * total, (flips, total)


# ---- qvit_gemm_qkv_split ----------------------------------------------------------------------------------
@pytest.mark.parametrize("wname", ["W4", "W4R", "W8"])
@pytest.mark.parametrize("seq,H", [(5, 1), (5, 3), (197, 1), (197, 3)])
def test_gemm_qkv_split_embedded(dev, wname, seq, H):
    """M = 2 seq, N = 3 x 64 x H, lda > K; the fp16 planes ([B][N / 64][seq][64] = M N halves each) sit between
    guards. Reference: the exact fp16 hi / lo split of in_scale times the fp64-checked EPI_F32 value."""
    from test_gpu_attention import split_planes
    wfmt = WFMTS[wname]
    M, N, K = 2 * seq, 3 * 64 * H, 384
    g = torch.Generator().manual_seed(seq + H)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    bias = torch.randn(N, generator=g)
    packed, npad, kpad = _pack(w, wfmt, dev)
    da, dw, s = _p(0.01, dev), _p(0.003, dev), 2.0 ** -3
    ar = Arena(dev, 4 * MB)
    A = ar.put(a.to(torch.int8).to(dev), ld=K + 16, name="A")
    bias_pad = ar.put(_lib.pad_bias(bias.to(dev), N, npad, dev), name="bias")
    hi = ar.carve_flat(M * N, torch.float16, writable=True, name="qkv_hi")
    lo = ar.carve_flat(M * N, torch.float16, writable=True, name="qkv_lo")
    ar.seal()
    _lib.gemm_qkv_split(A, M, K, packed, wfmt, N, npad, da, dw, bias_pad, seq, s, hi, lo)
    torch.cuda.synchronize()
    ar.assert_untouched()
    At = a.to(torch.int8).to(dev)
    hit = torch.full((M * N,), float("nan"), dtype=torch.float16, device=dev)
    lot = torch.full((M * N,), float("nan"), dtype=torch.float16, device=dev)
    bpt = _lib.pad_bias(bias.to(dev), N, npad, dev)
    _lib.gemm_qkv_split(At, M, K, packed, wfmt, N, npad, da, dw, bpt, seq, s, hit, lot)
    f32 = torch.empty((M, N), device=dev)
    _lib.gemm(At, M, K, packed, wfmt, N, npad, da, dw, bpt, _lib.EPI_F32, f32)
    torch.cuda.synchronize()
    assert torch.equal(hi.cpu().view(torch.int16), hit.cpu().view(torch.int16))
    assert torch.equal(lo.cpu().view(torch.int16), lot.cpu().view(torch.int16))
    ref = float(torch.tensor(0.01) * torch.tensor(0.003)) * O.int_accumulators(a.float(), w.float()).double() + bias.double()
    assert (f32.cpu().double() - ref).abs().max() / ref.abs().max() < 1e-6
    whi, wlo = split_planes(f32.cpu(), 2, seq, H, s)
    assert torch.equal(hi.cpu(), whi) and torch.equal(lo.cpu(), wlo)


# ---- qvit_layernorm_quant_i8_t32 and qvit_gemm_a32 -------------------------------------------------------
def _ln_inputs(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * 2 + 0.3
    gamma = torch.rand(cols, generator=g) + 0.5
    beta = torch.randn(cols, generator=g) * 0.1
    return x, gamma, beta


def _ln_oracle(x, gamma, beta, qt, d, qm, t):
    return O.quant_codes(F.layer_norm(x.double(), (x.shape[1],), None if gamma is None else gamma.double(),
                                      None if beta is None else beta.double(), 1e-6).float(), qt, d, qm, t)


@pytest.mark.parametrize("M", [1, 63, 65, 130])
def test_layernorm_t32_embedded(dev, M):
    """cols = kpad = 768, ldx > cols with NaN pads; the T32 buffer holds ceil(M / 64) x 64 rows and rows >= M keep
    their poison ("rows past M are never stored"). Bar of test_layernorm_quant_vs_oracle (<= 1 off, <= 5e-4)."""
    cols = 768
    x, gamma, beta = _ln_inputs(M, cols, 40 + M)
    d, qm = 4.0 / 127, 4.0
    R64 = _lib.t32_rows(M)
    ar = Arena(dev, 2 * MB)
    X = ar.put(x.to(dev), ld=cols + 4, name="x")
    G = ar.put(gamma.to(dev), name="gamma")
    Bt = ar.put(beta.to(dev), name="beta")
    T = ar.carve_flat(R64 * cols, torch.int8, name="codes_t32")       # writable: the bytes of rows < M only
    ar.allow_bytes(T, _lib.t32_to_rows(torch.arange(R64 * cols, device=dev), M, cols))   # byte offsets of rows < M
    ar.seal()
    q = (_lib.QT_NONLINEAR, _p(d, dev), _p(qm, dev), _p(1.0, dev), 0)
    _lib.layernorm_quant_i8_t32(X, G, Bt, 1e-6, *q, T, cols)
    torch.cuda.synchronize()
    ar.assert_untouched()
    Tt = torch.full((R64 * cols,), 93, dtype=torch.int8, device=dev)
    _lib.layernorm_quant_i8_t32(x.to(dev), gamma.to(dev), beta.to(dev), 1e-6, *q, Tt, cols)
    torch.cuda.synchronize()
    got = _lib.t32_to_rows(T, M, cols).cpu()
    assert torch.equal(got, _lib.t32_to_rows(Tt, M, cols).cpu())
    diff = (got.float() - _ln_oracle(x, gamma, beta, O.NONLINEAR, d, qm, 1.0)).abs()
    assert diff.max() <= 1 and (diff > 0).float().mean() <= 5e-4


@pytest.mark.parametrize("M", [1, 63, 65, 130])
@pytest.mark.parametrize("gelu", [False, True])
def test_gemm_a32_embedded(dev, M, gelu):
    """The one supported geometry (N = npad = 3072, K = 768). The T32 activation rows >= M hold poison codes; C
    rows >= M and columns [N, ldc) are guarded. Bar of test_gemm_int8_code_epilogue (<= 1 off, <= 2e-4)."""
    N, K = 3072, 768
    g = torch.Generator().manual_seed(60 + M)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    bias = torch.randn(N, generator=g) * 0.3
    packed, npad, kpad = pack_codes(w, _lib.W4, dev)
    d_a, d_w = 0.01, 0.5 / (317.0 * math.sqrt(K)) / 0.01
    epi = _lib.EPI_I8_GELU if gelu else _lib.EPI_I8
    kw = dict(out_qtype=_lib.QT_NONLINEAR, out_d=_p(QD, dev), out_qm=_p(QM, dev), out_t=_p(QT_T, dev),
              epi_table=_table(dev, epi, gelu))
    R64 = _lib.t32_rows(M)
    ar = Arena(dev, 2 * MB)
    T = ar.carve_flat(R64 * K, torch.int8, name="A_t32")
    idx = _lib.t32_to_rows(torch.arange(R64 * K, device=dev), M, K)
    T[idx.reshape(-1)] = a.to(torch.int8).to(dev).reshape(-1)                 # rows >= M stay poisoned
    bias_pad = ar.put(_lib.pad_bias(bias.to(dev), N, npad, dev), name="bias")
    C = ar.carve(M, N, N + 16, torch.int8, writable=True, name="C")
    ar.seal()
    _lib.gemm_a32(T, M, K, packed, _lib.W4, N, npad, _p(d_a, dev), _p(d_w, dev), bias_pad, epi, C, **kw)
    torch.cuda.synchronize()
    ar.assert_untouched()
    Ct = torch.full((M, N), 55, dtype=torch.int8, device=dev)
    _lib.gemm_a32(_lib.rows_to_t32(a.to(torch.int8).to(dev), K), M, K, packed, _lib.W4, N, npad, _p(d_a, dev),
                  _p(d_w, dev), _lib.pad_bias(bias.to(dev), N, npad, dev), epi, Ct, **kw)
    torch.cuda.synchronize()
    assert torch.equal(C.cpu(), Ct.cpu())
    v = (torch.tensor(d_a) * torch.tensor(d_w)) * O.int_accumulators(a.float(), w.float()).float() + bias
    ref = O.quant_codes(F.gelu(v) if gelu else v, O.NONLINEAR, QD, QM, QT_T)
    diff = (C.cpu().float() - ref).abs()
    assert diff.max() <= 1 and (diff > 0).float().mean() <= 2e-4


# ---- qvit_gemm_resid_ln -----------------------------------------------------------------------------------
def _resid_ln_args(dev, M, N, K, wfmt, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-127, 128, (M, K), generator=g)
    lim = 7 if wfmt == _lib.W4 else 127
    w = torch.randint(-lim, lim + 1, (N, K), generator=g)
    bias = torch.randn(N, generator=g) * 0.2
    base = torch.randn(M, N, generator=g)
    gamma = torch.rand(N, generator=g) + 0.5
    beta = torch.randn(N, generator=g) * 0.1
    return a, w, bias, base, gamma, beta


@pytest.mark.parametrize("wname", ["W4", "W8"])
@pytest.mark.parametrize("N", [192, 768])
@pytest.mark.parametrize("M", [1, 129, 333])
def test_gemm_resid_ln_embedded(dev, wname, M, N):
    """ldc > N, ldcodes > kpad_codes > N (codes [N, kpad_codes) zero, [kpad_codes, ldcodes) untouched), the counters
    exactly ceil(M / 128) ints between guards. Reference: EPI_F32_RESID (1e-6 of fp64), then the oracle LayerNorm +
    quantizer of the updated rows (<= 1 off, <= 5e-4); bit-identical to the two-launch form on tight buffers."""
    wfmt, K = WFMTS[wname], 256
    a, w, bias, base, gamma, beta = _resid_ln_args(dev, M, N, K, wfmt, M + N)
    packed, npad, kpad = pack_codes(w, wfmt, dev)
    d_a, d_w, qmn = 0.0123, 0.00457 if wfmt == _lib.W4 else 0.00457 / 16, 3.0
    dn = qmn / 127
    q = (_lib.QT_NONLINEAR, _p(dn, dev), _p(qmn, dev), _p(1.0, dev), 0)
    kpad_c, ldcodes = _round_up(N, 128) + 128, _round_up(N, 128) + 128 + 16
    nblk = (M + BM - 1) // BM
    ar = Arena(dev, 4 * MB)
    A = ar.put(a.to(torch.int8).to(dev), ld=K + 16, name="A")
    bias_pad = ar.put(_lib.pad_bias(bias.to(dev), N, npad, dev), name="bias")
    G = ar.put(gamma.to(dev), name="gamma")
    Bt = ar.put(beta.to(dev), name="beta")
    C = ar.carve(M, N, N + 4, torch.float32, writable=True, name="C")
    C.copy_(base.to(dev))
    codes = ar.carve(M, N, ldcodes, torch.int8, misalign=4, writable=kpad_c, name="codes")
    cnt = ar.carve_flat(nblk, torch.int32, misalign=4, writable=True, name="counters")
    ar.seal()
    lib = _lib.load()
    da_t, dw_t = _p(d_a, dev), _p(d_w, dev)      # (kept alive across the raw-pointer call)
    _ok(lib.qvit_gemm_resid_ln(A.data_ptr(), M, K, A.stride(0), packed.data_ptr(), wfmt, N, npad, da_t.data_ptr(),
                               dw_t.data_ptr(), bias_pad.data_ptr(), C.data_ptr(), C.stride(0), G.data_ptr(),
                               Bt.data_ptr(), 1e-6, q[0], q[1].data_ptr(), q[2].data_ptr(), q[3].data_ptr(), 0, None,
                               codes.data_ptr(), ldcodes, kpad_c, cnt.data_ptr(), _stream(dev)), "qvit_gemm_resid_ln")
    torch.cuda.synchronize()
    ar.assert_untouched()
    zero_pad = torch.as_strided(codes, (M, kpad_c - N), (ldcodes, 1), codes.storage_offset() + N)
    assert (zero_pad == 0).all()
    # two-launch form on tight buffers
    At, bpt = a.to(torch.int8).to(dev), _lib.pad_bias(bias.to(dev), N, npad, dev)
    xt = base.to(dev)
    _lib.gemm(At, M, K, packed, wfmt, N, npad, _p(d_a, dev), _p(d_w, dev), bpt, _lib.EPI_F32_RESID, xt)
    ct = torch.full((M, _round_up(N, 128)), 77, dtype=torch.int8, device=dev)
    _lib.layernorm_quant_i8(xt, gamma.to(dev), beta.to(dev), 1e-6, *q, ct, _round_up(N, 128))
    torch.cuda.synchronize()
    assert torch.equal(C.cpu().view(torch.int32), xt.cpu().view(torch.int32))
    assert torch.equal(codes.cpu(), ct[:, :N].cpu())
    alpha = float(torch.tensor(d_a) * torch.tensor(d_w))
    ref = alpha * O.int_accumulators(a.float(), w.float()).double() + bias.double() + base.double()
    assert (C.cpu().double() - ref).abs().max() / ref.abs().max() < 1e-6
    diff = (codes.cpu().float() - _ln_oracle(C.cpu(), gamma, beta, O.NONLINEAR, dn, qmn, 1.0)).abs()
    assert diff.max() <= 1 and (diff > 0).float().mean() <= 5e-4


# ---- row quantizers: qvit_quantize_act_i8, qvit_layernorm_quant_i8, qvit_im2col_quant_i8 -------------------
@pytest.mark.parametrize("rows", [1, 3, 5])
@pytest.mark.parametrize("cols", [100, 192])
@pytest.mark.parametrize("qt", [O.LINEAR, O.NONLINEAR])
def test_quantize_act_embedded(dev, rows, cols, qt):
    """Four rows per workgroup; ldx > cols (NaN pads), ldc > kpad > cols: [cols, kpad) zero, [kpad, ldc) untouched;
    codes 16-byte aligned only. Bar of test_quantize_act_codes_vs_oracle: linear exact; nonlinear <= 1 off in <= 1e-5 of codes."""
    d, qm, t = 0.02, 1.5, 0.9
    g = torch.Generator().manual_seed(rows * 7 + cols)
    if qt == O.LINEAR:
        x = torch.randn(rows, cols, generator=g) * 0.6
    else:   # away from rounding ties, so the random-input bar (<= 1e-5 of codes) means no flip among these few
        x = R.tie_free_values((rows, cols), R.NONLINEAR, d, qm, t, seed=rows * 7 + cols)
    kpad, ldc = _round_up(cols, 16) + 16, _round_up(cols, 16) + 32
    ar = Arena(dev, MB)
    X = ar.put(x.to(dev), ld=cols + 4, name="x")
    Cd = ar.carve(rows, cols, ldc, torch.int8, writable=kpad, name="codes")
    ar.seal()
    q = (_lib.QT_NONLINEAR if qt == O.NONLINEAR else _lib.QT_LINEAR, _p(d, dev), _p(qm, dev),
         _p(t, dev) if qt == O.NONLINEAR else None, 0)
    _lib.quantize_act_i8(X, *q, Cd, kpad)
    torch.cuda.synchronize()
    ar.assert_untouched()
    assert (torch.as_strided(Cd, (rows, kpad - cols), (ldc, 1), Cd.storage_offset() + cols) == 0).all()
    Ct = torch.full((rows, kpad), 77, dtype=torch.int8, device=dev)
    _lib.quantize_act_i8(x.to(dev), *q, Ct, kpad)
    torch.cuda.synchronize()
    assert torch.equal(Cd.cpu(), Ct[:, :cols].cpu())
    ref = O.quant_codes(x, qt, d, qm, t)
    diff = (Cd.cpu().float() - ref).abs()
    assert diff.max() <= (0 if qt == O.LINEAR else 1)
    assert (diff > 0).float().mean() <= (0.0 if qt == O.LINEAR else 1e-5)


@pytest.mark.parametrize("cols,ldx,arm", [(192, 196, "persist<1>"), (384, 388, "persist<2>"), (768, 772, "persist<3>"),
                                          (1000, 1004, "persist<4>"), (1280, 1284, "reg<8>"),
                                          (768, 771, "scalar (ldx % 4 != 0)"), (770, 774, "scalar (cols % 4 != 0)")])
def test_layernorm_quant_embedded(dev, cols, ldx, arm):
    """Every kind of LayerNorm kernel embedded, rows in {1, 3, 5} (four rows per workgroup): ldx > cols with NaN pads
    (a mean over ldx columns is NaN), codes base 4-byte aligned only (the documented requirement), ldc > kpad > cols.
    Bar of test_layernorm_quant_vs_oracle: <= 1 off, <= 5e-4 of the 9 x cols codes of the three row counts together."""
    d, qm = 4.0 / 127, 4.0
    kpad, ldc = _round_up(cols, 128) + 128, _round_up(cols, 128) + 128 + 4
    q = (_lib.QT_NONLINEAR, _p(d, dev), _p(qm, dev), _p(1.0, dev), 0)
    flips = {"embedded": 0, "tight": 0}
    for rows in (1, 3, 5):
        x, gamma, beta = _ln_inputs(rows, cols, rows + cols)
        ar = Arena(dev, MB)
        X = ar.put(x.to(dev), ld=ldx, misalign=16 if ldx % 4 == 0 else 4, name="x")
        G = ar.put(gamma.to(dev), name="gamma")
        Bt = ar.put(beta.to(dev), name="beta")
        Cd = ar.carve(rows, cols, ldc, torch.int8, misalign=4, writable=kpad, name="codes")
        ar.seal()
        _lib.layernorm_quant_i8(X, G, Bt, 1e-6, *q, Cd, kpad)
        torch.cuda.synchronize()
        ar.assert_untouched()
        assert (torch.as_strided(Cd, (rows, kpad - cols), (ldc, 1), Cd.storage_offset() + cols) == 0).all()
        Ct = torch.full((rows, kpad), 77, dtype=torch.int8, device=dev)
        _lib.layernorm_quant_i8(x.to(dev), gamma.to(dev), beta.to(dev), 1e-6, *q, Ct, kpad)
        torch.cuda.synchronize()
        if ldx % 4 == 0:   # (ldx 771: the tight call runs persist<3>, another kernel: both held to the oracle only)
            assert torch.equal(Cd.cpu(), Ct[:, :cols].cpu())
        for name, got in (("embedded", Cd.cpu()), ("tight", Ct[:, :cols].cpu())):
            diff = (got.float() - _ln_oracle(x, gamma, beta, O.NONLINEAR, d, qm, 1.0)).abs()
            assert diff.max() <= 1, (name, rows)
            flips[name] += int((diff > 0).sum())
    assert max(flips.values()) <= 5e-4 * 9 * cols, flips


@pytest.mark.parametrize("B", [1, 3, 5])
def test_im2col_quant_embedded(dev, B):
    """A padded strided 3x3 conv with one output pixel per image (rows = B in {1, 3, 5}) and a 16-wide patchify
    (the float4 path); ldc > kpad > K. Linear quantizer: exact (test_im2col_quant_vs_oracle)."""
    for conv in (dict(k=3, s=2, p=1, C=5, H=2), dict(k=16, s=16, p=0, C=1, H=16)):
        g = torch.Generator().manual_seed(B + conv["k"])
        x = torch.randn(B, conv["C"], conv["H"], conv["H"], generator=g) * 0.5
        d, qm = 1.0 / 127, 1.0
        k, s, p = conv["k"], conv["s"], conv["p"]
        K = conv["C"] * k * k
        OH = (conv["H"] + 2 * p - k) // s + 1
        rows = B * OH * OH
        kpad, ldc = _round_up(K, 16) + 16, _round_up(K, 16) + 32
        ar = Arena(dev, MB)
        X = ar.put(x.reshape(-1).to(dev), name="x").view(x.shape)
        Cd = ar.carve(rows, K, ldc, torch.int8, writable=kpad, name="codes")
        ar.seal()
        q = (_lib.QT_LINEAR, _p(d, dev), _p(qm, dev), None, 0)
        _lib.im2col_quant_i8(X, k, k, s, s, p, p, 1, 1, *q, Cd, kpad)
        torch.cuda.synchronize()
        ar.assert_untouched()
        assert (torch.as_strided(Cd, (rows, kpad - K), (ldc, 1), Cd.storage_offset() + K) == 0).all()
        Ct = torch.full((rows, kpad), 77, dtype=torch.int8, device=dev)
        _lib.im2col_quant_i8(x.to(dev), k, k, s, s, p, p, 1, 1, *q, Ct, kpad)
        torch.cuda.synchronize()
        assert torch.equal(Cd.cpu(), Ct[:, :K].cpu())
        ref = F.unfold(O.quant_codes(x, O.LINEAR, d, qm), k, padding=p, stride=s).transpose(1, 2).reshape(rows, K)
        assert torch.equal(Cd.cpu().float(), ref)


# ---- elementwise kernels (the C-ABI directly: the wrappers allocate their own outputs) ---------------------
ELEM_N = [0, 1, 3, 5, 1023, 4097]


@pytest.mark.parametrize("n", ELEM_N)
def test_fake_quant_and_gelu_embedded(dev, n):
    """x and y between guards, bases 16-byte aligned only. fake quant (linear): exact; GELU: bit-identical to
    the oracle's GELU (test_gelu_bit_exact_all_floats)."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(max(n, 1), generator=g) * 0.6
    d, qm = 0.013, 1.1
    d_t, qm_t = _p(d, dev), _p(qm, dev)           # (kept alive across the raw-pointer calls)
    for which in ("fake_quant", "gelu"):
        ar = Arena(dev, MB)
        X = ar.put(x.to(dev), name="x")
        Y = ar.carve_flat(max(n, 1), torch.float32, writable=n > 0, name="y")
        ar.seal()
        if which == "fake_quant":
            _ok(lib.qvit_fake_quant_f32(X.data_ptr(), n, _lib.QT_LINEAR, d_t.data_ptr(), qm_t.data_ptr(),
                                        None, 0, Y.data_ptr(), _stream(dev)), which)
        else:
            _ok(lib.qvit_gelu_f32(X.data_ptr(), n, Y.data_ptr(), _stream(dev)), which)
        torch.cuda.synchronize()
        ar.assert_untouched()
        if n:
            if which == "fake_quant":
                ref = O.fake_quant(x[:n], O.LINEAR, d, qm, 1.0)
                tight = _lib.fake_quant_f32(x[:n].to(dev), _lib.QT_LINEAR, _p(d, dev), _p(qm, dev), None)
            else:
                ref, tight = O.gelu(x[:n]), _lib.gelu_f32(x[:n].to(dev))
            assert torch.equal(Y.cpu().view(torch.int32), tight.cpu().view(torch.int32)), which
            assert torch.equal(Y.cpu(), ref), which


@pytest.mark.parametrize("n", ELEM_N)
@pytest.mark.parametrize("params", [R.PARAM_SETS[0], R.PARAM_SETS[-1]], ids=lambda p: str(p[0]))
def test_quant_backward_embedded(dev, n, params):
    """grad_x, the three scalars and the workspace at exactly qvit_quant_backward_workspace_bytes(n) between guards;
    x, grad_out, grad_x 16-byte aligned only. Bars of test_grad_x_and_sums (grad_x exact, sums within bounds)."""
    lib = _lib.load()
    kind, d, q_m, t = params
    clip = R.CLIPS[0]
    x, g = R.make_inputs(max(n, 1), kind, d, q_m, t, clip)
    nbytes = int(lib.qvit_quant_backward_workspace_bytes(n))
    assert nbytes >= 0
    ar = Arena(dev, MB)
    X = ar.put(x.to(dev), name="x")
    Gd = ar.put(g.to(dev), name="grad_out")
    GX = ar.carve_flat(max(n, 1), torch.float32, writable=n > 0, name="grad_x")
    S = ar.carve_flat(3, torch.float32, misalign=4, writable=True, name="grad_scalars")
    WS = ar.carve_flat(max(nbytes, 8), torch.uint8, misalign=8, writable=nbytes > 0, name="workspace")
    if 0 < nbytes:
        assert ar.carves[-1]["cols"] == nbytes
    ar.seal()
    keep = [None if v is None else _p(v, dev) for v in (d, q_m, t)]   # (alive across the raw-pointer call)
    f = lambda i: None if keep[i] is None else keep[i].data_ptr()
    _ok(lib.qvit_quant_backward(X.data_ptr(), Gd.data_ptr(), n, 0 if kind == R.LINEAR else 1, f(0), f(1), f(2),
                                float(clip[0]), float(clip[1]), 0.0, GX.data_ptr(), S.data_ptr(), WS.data_ptr(), nbytes,
                                _stream(dev)), "qvit_quant_backward")
    torch.cuda.synchronize()
    ar.assert_untouched()
    if n == 0:
        assert S.cpu().tolist() == [0.0, 0.0, 0.0]
        return
    gxt, st = _lib.quant_backward(x[:n].to(dev), g[:n].to(dev), 0 if kind == R.LINEAR else 1, _p(d, dev), _p(q_m, dev),
                                  None if t is None else _p(t, dev), clip[0], clip[1])
    assert torch.equal(GX.cpu(), gxt.cpu()) and torch.equal(S.cpu().view(torch.int32), st.cpu().view(torch.int32))
    r64, r32, floor, bounds = R.sum_bounds(x[:n], g[:n], kind, d, q_m, t, clip)
    assert torch.equal(GX.cpu(), r64["grad_x"].float())
    for i in range(3):
        assert abs(float(S[i]) - float(r64["sums"][i])) <= bounds[i], (i, float(S[i]), float(r64["sums"][i]))


@pytest.mark.parametrize("n,npad", [(1, 256), (200, 256), (257, 512)])
def test_pad_bias_embedded(dev, n, npad):
    lib = _lib.load()
    b = torch.randn(n, generator=torch.Generator().manual_seed(n))
    for bias in (b, None):
        ar = Arena(dev, MB)
        Bv = ar.put(b.to(dev), misalign=4, name="bias")
        out = ar.carve_flat(npad, torch.float32, misalign=4, writable=True, name="out")
        ar.seal()
        _ok(lib.qvit_pad_bias(None if bias is None else Bv.data_ptr(), n, out.data_ptr(), npad, _stream(dev)), "pad_bias")
        torch.cuda.synchronize()
        ar.assert_untouched()
        ref = torch.zeros(npad)
        if bias is not None:
            ref[:n] = b
        assert torch.equal(out.cpu(), ref)
        assert torch.equal(out.cpu(), _lib.pad_bias(None if bias is None else b.to(dev), n, npad, dev).cpu())


# ---- qvit_gemm_wonly / qvit_conv_wonly ---------------------------------------------------------------------
def _wonly_close(y, x, codes, d_w, bias):
    xd, wd = x.double(), d_w * codes.double()
    ref = xd @ wd.t() + bias.double()
    mag = xd.abs() @ wd.abs().t() + bias.double().abs()
    err = (y.double() - ref).abs()
    assert (err <= 1e-5 * mag + 1e-30).all(), float((err / (mag + 1e-30)).max())     # test_gpu_wonly.py TOL


@pytest.mark.parametrize("split", [3, 0], ids=["split_k_3", "unsplit"])
@pytest.mark.parametrize("wname", ["W4", "W16"])
@pytest.mark.parametrize("M", [1, 65])
def test_gemm_wonly_embedded(dev, M, wname, split):
    """ldx > K with NaN pads, ldy > N, the split-K workspace carved to exactly the bytes passed (3 partial sets:
    the kernel takes as many splits as fit), and the unsplit launch (no workspace)."""
    N, K = 200, 384
    g = torch.Generator().manual_seed(M + N)
    lim = 8 if wname == "W4" else 20000
    codes = torch.randint(-lim, lim, (N, K), generator=g)
    x = torch.randn(M, K, generator=g) * 3
    bias = torch.randn(N, generator=g) * 0.1
    npad = _round_up(N, 256)
    if wname == "W4":
        packed, npad, kpad = pack_codes(codes, _lib.W4, dev)
        wfmt = _lib.W4
    else:
        packed, wfmt = _lib.pack_weight_wide(codes.float().to(dev), npad, K)
        assert wfmt == _lib.W16
    d_w = 0.0123
    lib = _lib.load()
    ws_bytes = split * M * npad * 4
    dw_t = _p(d_w, dev)

    def call(X, Y, bp, ws):
        _ok(lib.qvit_gemm_wonly(X.data_ptr(), M, K, X.stride(0), packed.data_ptr(), wfmt, N, npad, dw_t.data_ptr(),
                                bp.data_ptr(), Y.data_ptr(), Y.stride(0), None if ws is None else ws.data_ptr(),
                                ws_bytes if ws is not None else 0, _stream(dev)), "qvit_gemm_wonly")
        torch.cuda.synchronize()

    ar = Arena(dev, 2 * MB)
    X = ar.put(x.to(dev), ld=K + 4, name="X")
    bp = ar.put(_lib.pad_bias(bias.to(dev), N, npad, dev), name="bias")
    Y = ar.carve(M, N, N + 4, torch.float32, writable=True, name="Y")
    WS = ar.carve_flat(ws_bytes // 4, torch.float32, writable=True, name="workspace") if split else None
    ar.seal()
    call(X, Y, bp, WS)
    ar.assert_untouched()
    Yt = torch.full((M, N), float("nan"), device=dev)
    wst = torch.empty(ws_bytes // 4, device=dev) if split else None
    call(x.to(dev), Yt, _lib.pad_bias(bias.to(dev), N, npad, dev), wst)
    assert torch.equal(Y.cpu().view(torch.int32), Yt.cpu().view(torch.int32))
    if split:   # the split really ran: the workspace holds partials
        assert not torch.isnan(WS).all()
    _wonly_close(Y.cpu(), x, codes, d_w, bias)


@pytest.mark.parametrize("narrow", [1, 0], ids=["narrow", "wide"])
def test_conv_wonly_embedded(dev, narrow):
    """One padded strided conv (3x3, stride 2, pad 1, 16 -> 40 channels, 15 x 15) on both schedules, X and Y
    (contiguous NCHW by contract) between guards, bases 16-byte aligned only."""
    B, C, H, N, k, s, p = 2, 16, 15, 40, 3, 2, 1
    g = torch.Generator().manual_seed(77)
    codes = torch.randint(-8, 8, (N, C * k * k), generator=g)
    x = torch.randn(B, C, H, H, generator=g)
    bias = torch.randn(N, generator=g) * 0.1
    packed, npad, kpad = pack_codes(codes, _lib.W4, dev)
    OH = (H + 2 * p - k) // s + 1
    d_w = 0.02
    lib = _lib.load()
    dw_t = _p(d_w, dev)
    prev = _lib.conv_wonly_narrow(narrow)
    try:
        assert _lib.narrow_conv_fits(_lib.W4, N, C * k * k, H, H) == bool(narrow)
        ar = Arena(dev, 2 * MB)
        X = ar.put(x.reshape(-1).to(dev), name="X")
        bp = ar.put(_lib.pad_bias(bias.to(dev), N, npad, dev), name="bias")
        Y = ar.carve_flat(B * N * OH * OH, torch.float32, writable=True, name="Y")
        ar.seal()
        _ok(lib.qvit_conv_wonly(X.data_ptr(), B, C, H, H, k, k, s, s, p, p, 1, 1, packed.data_ptr(), _lib.W4, N, npad, kpad,
                                dw_t.data_ptr(), bp.data_ptr(), Y.data_ptr(), None, 0, _stream(dev)), "conv_wonly")
        torch.cuda.synchronize()
        ar.assert_untouched()
        yt = _lib.conv_wonly(x.to(dev), (k, k), (s, s), (p, p), (1, 1), packed, _lib.W4, N, npad, kpad, _p(d_w, dev),
                             _lib.pad_bias(bias.to(dev), N, npad, dev), split=False)
        torch.cuda.synchronize()
    finally:
        _lib.conv_wonly_narrow(int(prev))
    y = Y.cpu().view(B, N, OH, OH)
    assert torch.equal(y.view(torch.int32), yt.cpu().view(torch.int32))
    wd = (d_w * codes.double()).view(N, C, k, k)
    ref = F.conv2d(x.double(), wd, bias.double(), stride=s, padding=p)
    mag = F.conv2d(x.double().abs(), wd.abs(), bias.double().abs(), stride=s, padding=p)
    assert ((y.double() - ref).abs() <= 1e-5 * mag).all()


# ---- qvit_attention / qvit_attention_split: guard rows after row B N ---------------------------------------
@pytest.mark.parametrize("kernel", ["fp32_input", "split"])
@pytest.mark.parametrize("mode", ["f32", "i8"])
@pytest.mark.parametrize("N", [1, 197])
def test_attention_tail_rows_embedded(dev, N, mode, kernel):
    """Guard rows after row B N (N = 1: the single-token edge) for the fp32 and int8 outputs, ldq / ldo > width.
    Bars of test_gpu_attention.py: 2e-6 of max |out| against fp64; codes <= 1 off in <= 1e-3."""
    from test_gpu_attention import ref_attention, split_planes
    B, H = 2, 2
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(B * N, 3 * H * 64, generator=g) * 1.5
    d, qm = 1.2 / 127, 1.2
    i8 = mode == "i8"
    kw = dict(out_qtype=_lib.QT_LINEAR, out_d=_p(d, dev), out_qm=_p(qm, dev)) if i8 else {}
    amode = _lib.ATT_I8 if i8 else _lib.ATT_F32
    odt = torch.int8 if i8 else torch.float32
    ar = Arena(dev, 4 * MB)
    out = ar.carve(B * N, H * 64, H * 64 + (16 if i8 else 4), odt, writable=True, name="out")
    if kernel == "split":
        hi, lo = split_planes(qkv, B, N, H, 1.0)
        hi_d, lo_d = ar.put(hi.to(dev), name="qkv_hi"), ar.put(lo.to(dev), name="qkv_lo")
        ar.seal()
        _lib.attention_split(hi_d, lo_d, B, N, H, 64, 0.125, out, amode, 1.0, **kw)
    else:
        Q = ar.put(qkv.to(dev), ld=3 * H * 64 + 4, name="qkv")
        ar.seal()
        _lib.attention(Q, B, N, H, 64, 0.125, out, amode, 1.0, **kw)
    torch.cuda.synchronize()
    ar.assert_untouched()
    tight = torch.zeros((B * N, H * 64), dtype=odt, device=dev)
    if kernel == "split":
        _lib.attention_split(hi.to(dev), lo.to(dev), B, N, H, 64, 0.125, tight, amode, 1.0, **kw)
    else:
        _lib.attention(qkv.to(dev), B, N, H, 64, 0.125, tight, amode, 1.0, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), tight.cpu())
    ref = ref_attention(qkv, B, N, H, 64, 0.125)
    if i8:
        diff = (out.cpu().float() - O.quant_codes(ref.float(), O.LINEAR, d, qm, None)).abs()
        assert diff.max() <= 1 and (diff > 0).float().mean() <= 1e-3
    else:
        assert (out.cpu().double() - ref).abs().max() <= 2e-6 * ref.abs().max()


@pytest.mark.parametrize("N", [1, 197])
def test_qkv_attention_embedded(dev, N):
    """qvit_qkv_attention with lda > K (poison codes in [K, lda)), ldo > width and guard rows after row B N.
    Reference: softmax(q k^T scale) v in fp64 from the fp32 qkv projection (QVIT_EPI_F32 on the same codes). Bar: the
    fused kernel is held to 2e-6 of max |out| against the split path (test_qkv_attention_fused_f32_vs_split_path),
    which is held to 2e-6 against this fp64 value (test_attention_fp32_vs_fp64): 4e-6 together."""
    from test_gpu_attention import _fused_case, ref_attention
    B, H, K = 2, 2, 256
    At, packed, npad, kpad, bias_pad, da, dw = _fused_case(dev, B, N, H, seed=N, K=K)
    ar = Arena(dev, 2 * MB)
    A = ar.put(At, ld=K + 16, name="A")
    out = ar.carve(B * N, 64 * H, 64 * H + 4, torch.float32, writable=True, name="out")
    ar.seal()
    _lib.qkv_attention(A, B, N, K, packed, npad, da, dw, bias_pad, H, 0.125, out, _lib.ATT_F32, 2.0 ** -2)
    torch.cuda.synchronize()
    ar.assert_untouched()
    tight = torch.full((B * N, 64 * H), float("nan"), device=dev)
    _lib.qkv_attention(At, B, N, K, packed, npad, da, dw, bias_pad, H, 0.125, tight, _lib.ATT_F32, 2.0 ** -2)
    qkv = torch.empty((B * N, 3 * 64 * H), device=dev)
    _lib.gemm(At, B * N, K, packed, _lib.W4, 3 * 64 * H, npad, da, dw, bias_pad, _lib.EPI_F32, qkv)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), tight.cpu().view(torch.int32))
    ref = ref_attention(qkv.cpu(), B, N, H, 64, 0.125)
    assert (out.cpu().double() - ref).abs().max() <= 4e-6 * ref.abs().max()


# ---- UltraNet: qvit_ultra_conv, qvit_ultra_tail ---------------------------------------------------------------
ULTRA_DEN = 7 * 15      # (2^(w_bit - 1) - 1)(2^a_bit - 1) at w_bit = a_bit = 4


def _ultra_layer(cin, ks, cout, seed):
    """Weight codes [round_up(cout, 16)][kpad] in K order (ky, kx, c), zero padded, and BN constants that spread the
    codes over 0 .. 15 (every third channel decreasing)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-7, 8, (cout, ks, ks, cin), generator=g)
    kpad = _round_up(ks * ks * cin, 64)
    wc = torch.zeros((_round_up(cout, 16), kpad), dtype=torch.int8)
    wc[:cout, :ks * ks * cin] = w.reshape(cout, -1).to(torch.int8)
    ystd = 8.7 * 4.3 * math.sqrt(ks * ks * cin) / ULTRA_DEN
    alpha = (0.3 / ystd) * (torch.rand(cout, generator=g) + 0.5)
    alpha[2::3] *= -1
    shift = torch.rand(cout, generator=g) * 0.4 + 0.3
    return w, wc, alpha, shift


def _ultra_acc(x, w):
    """Exact integer accumulators of the 'same'-padded conv: x codes NHWC [B, H, W, cin], w [cout, ks, ks, cin]."""
    return F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(),
                    padding=w.shape[1] // 2).permute(0, 2, 3, 1)


def _ultra_codes_ref(x, w, alpha, shift, pool=False):
    v = (alpha.double() * (_ultra_acc(x, w) / ULTRA_DEN) + shift.double()).clamp(0, 1) * 15
    c = torch.round(v)                                                        # round half to even
    if pool:
        c = F.max_pool2d(c.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    return c


def _assert_ultra_codes(got, want):
    d = (got.cpu().double() - want).abs()                                     # the bar of test_gpu_ultranet.py
    assert d.max() <= 1 and (d > 0).double().mean() <= 1e-4, (float(d.max()), float((d > 0).double().mean()))


@pytest.mark.parametrize("mode,cin,ks,cout", [("codes", 16, 3, 20), ("codes", 64, 3, 52), ("codes_pool", 32, 3, 52),
                                              ("f32", 64, 1, 36)])
def test_ultra_conv_embedded(dev, mode, cin, ks, cout):
    """B = 2 maps of 10 x 14 pixels (more than one workgroup tile, ragged in both directions), cout below the
    kernel's channel tile, ldo = cout + 4 and guard pixels after the last. Reference: the exact integer conv, then
    the header's epilogue in fp64; codes <= 1 off in <= 1e-4, the fp32 head 1e-5 relative (test_gpu_ultranet.py)."""
    B, H, W = 2, 10, 14
    w, wc, alpha, shift = _ultra_layer(cin, ks, cout, cin + cout)
    x = torch.randint(0, 16, (B, H, W, cin), generator=torch.Generator().manual_seed(cout), dtype=torch.int8)
    lmode = {"codes": _lib.ULTRA_CODES, "codes_pool": _lib.ULTRA_CODES_POOL, "f32": _lib.ULTRA_F32}[mode]
    OH, OW = (H // 2, W // 2) if mode == "codes_pool" else (H, W)
    f32 = mode == "f32"
    ar = Arena(dev, 2 * MB)
    X = ar.put(x.reshape(-1).to(dev), name="in")
    Wc = ar.put(wc.reshape(-1).to(dev), name="wcodes")
    Al = None if f32 else ar.put(alpha.to(dev), misalign=4, name="alpha")
    Sh = ar.put(shift.to(dev), misalign=4, name="shift")
    out = ar.carve(B * OH * OW, cout, cout + 4, torch.float32 if f32 else torch.int8, misalign=16 if f32 else 4,
                   writable=True, name="out")
    ar.seal()
    _ok(_lib.load().qvit_ultra_conv(X.data_ptr(), B, H, W, cin, ks, Wc.data_ptr(), wc.shape[1], cout, 4, 4,
                                    None if f32 else Al.data_ptr(), Sh.data_ptr(), lmode, out.data_ptr(), cout + 4,
                                    _stream(dev)), "qvit_ultra_conv")
    torch.cuda.synchronize()
    ar.assert_untouched()
    tight = _lib.ultra_conv(x.to(dev), ks, wc.to(dev), cout, 4, 4, None if f32 else alpha.to(dev), shift.to(dev), lmode)
    torch.cuda.synchronize()
    got = out.cpu().view(B, OH, OW, cout)
    if f32:
        assert torch.equal(got.view(torch.int32), tight.cpu().view(torch.int32))
        ref = _ultra_acc(x, w) / ULTRA_DEN + shift.double()
        assert ((got.double() - ref).norm() / ref.norm()).item() <= 1e-5
    else:
        assert torch.equal(got, tight.cpu())
        want = _ultra_codes_ref(x, w, alpha, shift, pool=mode == "codes_pool")
        assert len(torch.unique(want)) >= 8
        _assert_ultra_codes(got, want)


def test_ultra_tail_embedded(dev):
    """qvit_ultra_tail (four 3x3 64 -> 64 blocks and the 1x1 head, one launch) on B = 2 maps of 10 x 14 with
    ldo = hout + 4 and guard pixels after the last. Bit-identical to a tight call and to the per-layer
    qvit_ultra_conv launches (the header's statement); each of those layers is held to the integer reference on
    the codes that entered it (<= 1 off in <= 1e-4; the head 1e-5 relative), which carries the bar to the tail."""
    B, H, W, hout = 2, 10, 14, 36
    layers = [_ultra_layer(64, 3, 64, 900 + l) for l in range(4)]
    hw, hwc, _, hbias = _ultra_layer(64, 1, hout, 950)
    hwc = hwc[:48]
    x = torch.randint(0, 16, (B, H, W, 64), generator=torch.Generator().manual_seed(5), dtype=torch.int8)
    ar = Arena(dev, 2 * MB)
    X = ar.put(x.reshape(-1).to(dev), name="in")
    Ws = [ar.put(l[1].reshape(-1).to(dev), name=f"wcodes{i}") for i, l in enumerate(layers)]
    Als = [ar.put(l[2].to(dev), misalign=4, name=f"alpha{i}") for i, l in enumerate(layers)]
    Shs = [ar.put(l[3].to(dev), misalign=4, name=f"shift{i}") for i, l in enumerate(layers)]
    Hc = ar.put(hwc.reshape(-1).to(dev), name="hcodes")
    Hb = ar.put(hbias.to(dev), misalign=4, name="hbias")
    out = ar.carve(B * H * W, hout, hout + 4, torch.float32, writable=True, name="out")
    ar.seal()
    import ctypes
    arr = lambda ts: (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ts])
    _ok(_lib.load().qvit_ultra_tail(X.data_ptr(), B, H, W, arr(Ws), layers[0][1].shape[1], arr(Als), arr(Shs),
                                    Hc.data_ptr(), hwc.shape[1], Hb.data_ptr(), hout, 4, 4, out.data_ptr(), hout + 4,
                                    None, 0, 0, 0.0, None, None, _stream(dev)), "qvit_ultra_tail")
    torch.cuda.synchronize()
    ar.assert_untouched()
    dW = [l[1].to(dev) for l in layers]
    dA, dS = [l[2].to(dev) for l in layers], [l[3].to(dev) for l in layers]
    tight = _lib.ultra_tail(x.to(dev), dW, dA, dS, hwc.to(dev), hbias.to(dev), hout, 4, 4)
    h = x
    for (w, wc, alpha, shift), wd, ad, sd in zip(layers, dW, dA, dS):
        nxt = _lib.ultra_conv(h.to(dev), 3, wd, 64, 4, 4, ad, sd, _lib.ULTRA_CODES).cpu()
        _assert_ultra_codes(nxt, _ultra_codes_ref(h, w, alpha, shift))
        h = nxt
    head = _lib.ultra_conv(h.to(dev), 1, hwc.to(dev), hout, 4, 4, None, hbias.to(dev), _lib.ULTRA_F32)
    torch.cuda.synchronize()
    got = out.cpu().view(B, H, W, hout)
    assert torch.equal(got.view(torch.int32), tight.cpu().view(torch.int32))
    assert torch.equal(got.view(torch.int32), head.cpu().view(torch.int32))
    assert len(torch.unique(h)) >= 8
    ref = _ultra_acc(h, hw) / ULTRA_DEN + hbias.double()
    assert ((got.double() - ref).norm() / ref.norm()).item() <= 1e-5


# ---- the chunked launch of gemm_w4a8.hip ------------------------------------------------------------------
def test_gemm_chunked_launch(dev):
    """launch() starts one kernel per chunk of rows whose A span stays below 2^32 bytes: rows = (2^32 - 1 - K) / lda
    rounded down to BM. lda = 2^24 and K = 128 give 128 rows per chunk, so M = 300 runs as 128 + 128 + 44 with the
    chunk offsets A + m0 lda, C + m0 ldc esize, counters + m0 / BM and codes + m0 ldcodes. A is a view of a ~5 GB
    torch.empty buffer of which only the K valid columns are ever written. Checked against the same calls on a
    contiguous copy of A (one chunk) and against the oracle."""
    M, N, K, lda = 300, 200, 128, 1 << 24
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    rows_per_chunk = ((1 << 32) - 1 - K) // lda // BM * BM
    assert rows_per_chunk == BM and M > 2 * rows_per_chunk and M % rows_per_chunk
    g = torch.Generator().manual_seed(300)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w = torch.randint(-7, 8, (N, K), generator=g)
    bias = torch.randn(N, generator=g) * 0.2
    base = torch.randn(M, N, generator=g)
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.1
    packed, npad, kpad = pack_codes(w, _lib.W4, dev)
    bias_pad = _lib.pad_bias(bias.to(dev), N, npad, dev)
    acc = O.int_accumulators(a.float(), w.float())
    big = torch.empty((M - 1) * lda + K, dtype=torch.int8, device=dev)
    try:
        A = torch.as_strided(big, (M, K), (lda, 1))
        At = a.to(torch.int8).to(dev)
        A.copy_(At)
        d_a, d_w = _p(0.0123, dev), _p(0.00457, dev)
        qk = dict(out_qtype=_lib.QT_NONLINEAR, out_d=_p(QD, dev), out_qm=_p(QM, dev), out_t=_p(QT_T, dev))
        # EPI_I32 (esize 4), exact
        ar = Arena(dev, 2 * MB)
        C = ar.carve(M, N, N + 4, torch.int32, writable=True, name="C_i32")
        C8 = ar.carve(M, N, _round_up(N, 16) + 16, torch.int8, writable=True, name="C_i8")
        Cr = ar.carve(M, N, N + 4, torch.float32, writable=True, name="C_resid")
        Cr.copy_(base.to(dev))
        kpad_c, ldcodes = 256, 272
        codes = ar.carve(M, N, ldcodes, torch.int8, misalign=4, writable=kpad_c, name="codes")
        cnt = ar.carve_flat((M + BM - 1) // BM, torch.int32, misalign=4, writable=True, name="counters")
        ar.seal()
        _lib.gemm(A, M, K, packed, _lib.W4, N, npad, None, None, None, _lib.EPI_I32, C)
        _lib.gemm(A, M, K, packed, _lib.W4, N, npad, d_a, d_w, bias_pad, _lib.EPI_I8, C8, **qk)
        lnq = (_lib.QT_NONLINEAR, _p(3.0 / 127, dev), _p(3.0, dev), _p(1.0, dev), 0)
        lib = _lib.load()
        Gm, Bt = gamma.to(dev), beta.to(dev)
        _ok(lib.qvit_gemm_resid_ln(A.data_ptr(), M, K, lda, packed.data_ptr(), _lib.W4, N, npad, d_a.data_ptr(),
                                   d_w.data_ptr(), bias_pad.data_ptr(), Cr.data_ptr(), Cr.stride(0), Gm.data_ptr(),
                                   Bt.data_ptr(), 1e-6, lnq[0], lnq[1].data_ptr(), lnq[2].data_ptr(), lnq[3].data_ptr(), 0,
                                   None, codes.data_ptr(), ldcodes, kpad_c, cnt.data_ptr(), _stream(dev)), "resid_ln")
        torch.cuda.synchronize()
        ar.assert_untouched()
        assert torch.equal(C.cpu().long(), acc)
        # the same calls on a contiguous copy of A (a single chunk)
        Ct = torch.empty((M, N), dtype=torch.int32, device=dev)
        C8t = torch.empty((M, _round_up(N, 16)), dtype=torch.int8, device=dev)
        xt = base.to(dev)
        ct = torch.full((M, kpad_c), 77, dtype=torch.int8, device=dev)
        _lib.gemm(At, M, K, packed, _lib.W4, N, npad, None, None, None, _lib.EPI_I32, Ct)
        _lib.gemm(At, M, K, packed, _lib.W4, N, npad, d_a, d_w, bias_pad, _lib.EPI_I8, C8t, **qk)
        _lib.gemm(At, M, K, packed, _lib.W4, N, npad, d_a, d_w, bias_pad, _lib.EPI_F32_RESID, xt)   # the two-launch form
        _lib.layernorm_quant_i8(xt, Gm, Bt, 1e-6, *lnq, ct, kpad_c)
        torch.cuda.synchronize()
        assert torch.equal(C.cpu(), Ct.cpu())
        assert torch.equal(C8.cpu(), C8t[:, :N].cpu())
        assert torch.equal(Cr.cpu().view(torch.int32), xt.cpu().view(torch.int32))
        assert torch.equal(codes.cpu(), ct[:, :N].cpu())
        assert (torch.as_strided(codes, (M, kpad_c - N), (ldcodes, 1), codes.storage_offset() + N) == 0).all()
        v = (torch.tensor(0.0123) * torch.tensor(0.00457)) * acc.float() + bias
        diff = (C8.cpu().float() - O.quant_codes(v, O.NONLINEAR, QD, QM, QT_T)).abs()
        assert diff.max() <= 1 and (diff > 0).float().mean() <= 2e-4
        diff = (codes.cpu().float() - _ln_oracle(Cr.cpu(), gamma, beta, O.NONLINEAR, 3.0 / 127, 3.0, 1.0)).abs()
        assert diff.max() <= 1 and (diff > 0).float().mean() <= 5e-4
        assert torch.cuda.max_memory_allocated(dev) < 6 << 30
    finally:
        del big
        A = None
        torch.cuda.empty_cache()
