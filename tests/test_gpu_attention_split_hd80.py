"""qvit_attention_split and qvit_gemm_qkv_split_hd at head_dim 80 (planes [B][3H][N][80], 160-B rows).

The attention tests build the planes on the host from an fp32 qkv with the documented formula (hi = f16(x s),
lo = f16(x s - hi), head-major), so they do not depend on the GEMM epilogue. Reference, criterion and C_FWD are those
of test_gpu_attention_hd80.py (the float64 restatement in attention_hd_ref.py). The plane buffers are allocated
exactly, between two NaN guard regions: a DMA one row or one head too far puts NaN into a softmax or a P.V sum.

What can go wrong here is an offset: 80-element rows under a 64-column image and a 16-column tail, a tail source row
that is not clamped with its image row, h * 80 bytes of codes that are no multiple of 64, and a ring whose blocks
carry five DMAs per wave where the 64-wide kernel counts four."""
import pytest
import torch

import attention_hd_ref as R
import vit_codes_ref as V
from oracle import quant_oracle as O
from test_gpu_attention_hd80 import HD, SCALE, check_fwd, run_fwd
from ultra_ref import assert_codes_tie_proven

pytestmark = pytest.mark.gpu

# smallest; h * 80 no multiple of 64; one past a key block; exactly one query block; one past a 192- and a 256-query
# group (ViT-Huge's N); two groups; 640 units (more than the resident grid: the ring crosses units with one query block)
SHAPES = [(1, 1, 1), (1, 5, 2), (3, 33, 2), (1, 64, 3), (1, 193, 1), (2, 257, 2), (1, 300, 1), (40, 5, 16)]
GUARD = 4096    # fp16 elements of NaN on either side of a plane buffer (a multiple of 8: 16-B alignment kept)


def _p(v, dev):
    return torch.tensor([v], dtype=torch.float32, device=dev)


def planes(qkv, B, N, H, in_scale, dev):
    """Device hi/lo planes [B][3H][N][80] of in_scale * qkv as exact-size views between NaN guards."""
    x = qkv[:, :3 * H * HD].float() * in_scale
    hi = x.half()
    lo = (x - hi.float()).half()
    out = []
    for t in (hi, lo):
        flat = t.reshape(B, N, 3 * H, HD).permute(0, 2, 1, 3).contiguous().reshape(-1)
        buf = torch.full((flat.numel() + 2 * GUARD,), float("nan"), dtype=torch.float16, device=dev)
        buf[GUARD:GUARD + flat.numel()] = flat.to(dev)
        out.append(buf[GUARD:GUARD + flat.numel()])
    return out


def in_scale_of(qkv):
    from quantized_vit_amd.vit_model import _pow2_scale
    return _pow2_scale(float(qkv.abs().max()))


def run_split_f32(dev, qkv, B, N, H, pad=0, extra_rows=0, poison=float("nan")):
    from quantized_vit_amd import _lib
    s = in_scale_of(qkv)
    hi, lo = planes(qkv, B, N, H, s, dev)
    obuf = torch.full((B * N + extra_rows, H * HD + pad), poison, dtype=torch.float32, device=dev)
    _lib.attention_split(hi, lo, B, N, H, HD, SCALE, obuf[:B * N, :H * HD], _lib.ATT_F32, s)
    torch.cuda.synchronize()
    return obuf


@pytest.mark.parametrize("B,N,H", SHAPES)
def test_f32_vs_float64_and_the_fp32_input_kernel(dev, B, N, H):
    qkv, _, o64, o32, _, _ = R.case(B, N, H, HD)
    o = run_split_f32(dev, qkv, B, N, H)
    check_fwd(f"split B={B} N={N} H={H}", o, o64, o32)
    o_in = run_fwd(dev, qkv, B, N, H)[0]
    print(f"split B={B} N={N} H={H}: max |split - qvit_attention(hd=80)| = {float((o - o_in).abs().max()):.3e}")
    assert torch.equal(o, o_in)     # the same arithmetic in the same order, as at 64


def test_f32_row_stride_and_untouched_padding(dev):
    B, N, H = 3, 33, 2
    qkv, _, o64, o32, _, _ = R.case(B, N, H, HD)
    obuf = run_split_f32(dev, qkv, B, N, H, pad=4, extra_rows=2, poison=-77.0)
    assert obuf.stride(0) == H * HD + 4
    check_fwd("split, padded rows", obuf[:B * N, :H * HD], o64, o32)
    assert bool((obuf[:, H * HD:] == -77.0).all()) and bool((obuf[B * N:] == -77.0).all())
    assert torch.equal(obuf[:B * N, :H * HD], run_split_f32(dev, qkv, B, N, H))


QUANTIZERS = [(O.LINEAR, 1.0), (O.NONLINEAR, 0.8)]


def _quantizer(qt, t, dev):
    from quantized_vit_amd import _lib
    from quantized_vit_amd.quant_layers import epilogue_table_geometry, saturation_level
    qm = 1.2
    d = qm ** t / 127 if qt == O.NONLINEAR else qm / 127
    qtc = _lib.QT_LINEAR if qt == O.LINEAR else _lib.QT_NONLINEAR
    kw = dict(out_qtype=qtc, out_d=_p(d, dev), out_qm=_p(qm, dev), out_t=_p(t, dev) if qt == O.NONLINEAR else None)
    geo = epilogue_table_geometry(qtc, d, qm, t, saturation_level(qtc, d, qm, t), False)
    table = _lib.epi_table_build(_lib.EPI_I8, qtc, kw["out_d"], kw["out_qm"], kw["out_t"], 0, *geo, dev)
    assert int(table[12:16].view(torch.int32).item()) == 1
    return V.PSet("split-hd80", qt, d, qm, t), kw, table


@pytest.mark.parametrize("qt,t", QUANTIZERS)
def test_i8_codes(dev, qt, t):
    """Per shape and per store path (ldo % 16 == 0: the 16-B transposed stores; ldo % 16 == 4: 4-B stores): the codes
    with a valid code table are the codes without one, byte for byte, and the columns [H * 80, ldo) and the rows past
    B * N keep their poison. Over all shapes together: the codes against the device quantizer's restatement applied
    to this kernel's own fp32 output, by the rule of the width-64 tests (vit_codes_ref.attention_ties: every code
    outside a possible tie within 2e-6 max|out| is equal, a possible tie differs by at most 1, ties <= CAP_ATTN)."""
    from quantized_vit_amd import _lib
    ps, kw, table = _quantizer(qt, t, dev)
    got, ref, tie = [], [], []
    for B, N, H in SHAPES:
        qkv = R.case(B, N, H, HD)[0]
        s = in_scale_of(qkv)
        hi, lo = planes(qkv, B, N, H, s, dev)
        o32 = run_split_f32(dev, qkv, B, N, H)
        C = H * HD
        first = None
        for ldo in ((C + 15) // 16 * 16 + 16, (C + 15) // 16 * 16 + 4):
            outs = []
            for tab in (None, table):
                cbuf = torch.full((B * N + 2, ldo), 99, dtype=torch.int8, device=dev)
                _lib.attention_split(hi, lo, B, N, H, HD, SCALE, cbuf[:B * N], _lib.ATT_I8, s, epi_table=tab, **kw)
                torch.cuda.synchronize()
                assert bool((cbuf[:, C:] == 99).all()) and bool((cbuf[B * N:] == 99).all()), (B, N, H, ldo)
                outs.append(cbuf[:B * N, :C].cpu())
            assert torch.equal(outs[0], outs[1]), (B, N, H, ldo, "code table against the per-element quantizer")
            first = outs[0] if first is None else first
            assert torch.equal(outs[0], first), (B, N, H, ldo, "the two store paths")
        r, tt = V.attention_ties(o32.double().cpu(), ps)
        n_diff = int((first.to(torch.int32) - r.to(torch.int32)).ne(0).sum())
        print(f"i8 {ps.qt} B={B} N={N} H={H}: {n_diff} of {r.numel()} codes differ from the quantizer of the fp32 output, "
              f"{int(tt.sum())} possible ties")
        got.append(first.reshape(-1)); ref.append(r.reshape(-1)); tie.append(tt.reshape(-1))
    got, ref, tie = torch.cat(got), torch.cat(ref), torch.cat(tie)
    assert len(torch.unique(got)) > 50
    assert_codes_tie_proven(got, ref, tie, V.CAP_ATTN)


# ---- qvit_gemm_qkv_split_hd ------------------------------------------------------------------------------------------
def _gemm_case(dev, wfmt, seq, B, N, K=256):
    from quantized_vit_amd import _lib
    from test_gpu_kernels import act_buffer, pack_codes
    M = B * seq
    g = torch.Generator().manual_seed(seq + B + N)
    a = torch.randint(-127, 128, (M, K), generator=g)
    w4 = wfmt in (_lib.W4, _lib.W4R, _lib.W8R)
    lim = 7 if w4 else 127
    w = torch.randint(-lim, lim + 1, (N, K), generator=g)
    bias = torch.randn(N, generator=g)
    packed, npad, kpad = pack_codes(w, _lib.W4 if w4 else _lib.W8, dev)
    if wfmt == _lib.W4R:
        packed = _lib.pack_weight_w4r(packed, npad, kpad)
    elif wfmt == _lib.W8R:
        packed = _lib.pack_weight_w8r(packed, npad, kpad)
    bias_pad = _lib.pad_bias(bias.to(dev), N, npad, dev)
    return M, npad, kpad, act_buffer(a, kpad, dev), packed, bias_pad, _p(0.01, dev), _p(0.003, dev)


def _split_hd(dev, A, M, kpad, packed, wfmt, N, npad, da, dw, bias_pad, seq, s, hd):
    """(hi, lo) of gemm_qkv_split at head_dim hd, written into exact-size views between NaN guards (checked)."""
    from quantized_vit_amd import _lib
    bufs = [torch.full((M * N + 2 * GUARD,), float("nan"), dtype=torch.float16, device=dev) for _ in range(2)]
    hi, lo = (b[GUARD:GUARD + M * N] for b in bufs)
    _lib.gemm_qkv_split(A, M, kpad, packed, wfmt, N, npad, da, dw, bias_pad, seq, s, hi, lo, head_dim=hd)
    torch.cuda.synchronize()
    for b in bufs:
        assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + M * N:]).all())
    return hi.cpu(), lo.cpu()


def _wfmts():
    from quantized_vit_amd import _lib
    return [_lib.W4, _lib.W8, _lib.W4R, _lib.W8R]


@pytest.mark.parametrize("wfmt", _wfmts())
@pytest.mark.parametrize("seq,B,N", [(5, 2, 480), (33, 5, 720)])
def test_gemm_qkv_split_hd80_equals_f32_epilogue(dev, wfmt, seq, B, N):
    """hi/lo planes are the exact split of in_scale times the QVIT_EPI_F32 output at the head-major position.
    N 480: npad 512, the last column tile half empty. M = 165: crosses a 128-row tile with a seq that does not
    divide 128; N 720: heads straddle the 64-column waves and the 256-column tiles."""
    from quantized_vit_amd import _lib
    M, npad, kpad, A, packed, bias_pad, da, dw = _gemm_case(dev, wfmt, seq, B, N)
    ref = torch.empty((M, N), device=dev)
    _lib.gemm(A, M, kpad, packed, wfmt, N, npad, da, dw, bias_pad, _lib.EPI_F32, ref)
    s = 2.0 ** -3
    hi, lo = _split_hd(dev, A, M, kpad, packed, wfmt, N, npad, da, dw, bias_pad, seq, s, HD)
    x = ref.cpu() * s
    whi = x.half()
    wlo = (x - whi.float()).half()
    f = lambda t: t.reshape(B, seq, N // HD, HD).permute(0, 2, 1, 3).contiguous().reshape(-1)
    assert torch.equal(hi.view(torch.int16), f(whi).view(torch.int16))
    assert torch.equal(lo.view(torch.int16), f(wlo).view(torch.int16))


@pytest.mark.parametrize("wfmt", _wfmts())
def test_gemm_qkv_split_hd64_is_the_existing_entry_point(dev, wfmt):
    """lib.qvit_gemm_qkv_split_hd(head_dim 64), called directly (the wrapper routes 64 to the old symbol)."""
    from quantized_vit_amd import _lib
    seq, B, N = 33, 5, 192
    M, npad, kpad, A, packed, bias_pad, da, dw = _gemm_case(dev, wfmt, seq, B, N)
    s = 2.0 ** -3
    old = _split_hd(dev, A, M, kpad, packed, wfmt, N, npad, da, dw, bias_pad, seq, s, 64)
    new = [torch.full((M * N,), float("nan"), dtype=torch.float16, device=dev) for _ in range(2)]
    rc = _lib.load().qvit_gemm_qkv_split_hd(A.data_ptr(), M, kpad, A.stride(0), packed.data_ptr(), wfmt, N, npad,
                                            da.data_ptr(), dw.data_ptr(), bias_pad.data_ptr(), seq, 64, s,
                                            new[0].data_ptr(), new[1].data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(old[0]).any())
    assert torch.equal(new[0].cpu().view(torch.int16), old[0].view(torch.int16))
    assert torch.equal(new[1].cpu().view(torch.int16), old[1].view(torch.int16))
