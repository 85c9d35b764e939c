"""qvit_attention (fp32 output) and qvit_attention_backward at head_dim 80 against the float64 restatement of the
reference attention (attention_hd_ref.py).

Metric, as test_gpu_attention_backward.py: err = max |x - x64| / max |x64| for the output and for each section
(dq, dk, dv) of grad_qkv; err_t is the same figure for the fp32 CPU evaluation of the same expression, floored at
fp32's eps; the assertion is err <= C max(err_t, eps). Where the true dq, dk vanish by cancellation (one key) the
denominator is the size of the cancelling terms, for both err and err_t.

C_FWD, C_BWD: the next power of two at or above twice the worst err / max(err_t, eps) measured on an MI355X over
SHAPES (DESIGN.md section 19 records the worst ratios and their shapes). Two chained hi/lo products allow 4x each,
so a ratio above 16 would be a bug, not a bound to widen.

Layout these tests guard: the 80 columns of a head are not padded to 96. The q . k contraction ends in a K = 16
MFMA step on columns 64 .. 79, and the LDS images keep those 16 columns in a tail of their own. What can go wrong
is therefore an offset (h * 80 is no multiple of 64; a tail read landing in the neighbouring head, or in the k
section behind q), not a padding value: the strided case puts NaN in every column no kernel may read.
"""
import pytest
import torch

import attention_hd_ref as R

pytestmark = pytest.mark.gpu

HD = 80
C_FWD = 8.0     # worst ratio 2.15: forward, B=1 N=5 H=2
C_BWD = 16.0    # worst ratio 6.78: dv at B=1 N=1 H=1 (err 8.1e-7 against the eps floor; err_t = 0 there)
SCALE = HD ** -0.5
SHAPES = [(1, 1, 1), (1, 5, 2), (3, 33, 2), (1, 64, 3), (2, 257, 2), (1, 300, 1)]
EINVAL = -1


def _pad(t, dev, pad, fill=0.0):
    """Device copy of the 2-D tensor as a view of a buffer with `pad` extra columns per row (filled with `fill`)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=torch.float32, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf, buf[:, :t.shape[1]]


def run_fwd(dev, qkv, B, N, H, scale=SCALE, pad=0, in_fill=0.0, poison=float("nan")):
    """qvit_attention on the device: (out view, its whole buffer, the qkv view, in_scale)."""
    from quantized_vit_amd import _lib
    from quantized_vit_amd.vit_model import _pow2_scale
    _, q = _pad(qkv, dev, pad, in_fill)
    obuf = torch.full((B * N, H * HD + pad), poison, dtype=torch.float32, device=dev)
    out = obuf[:, :H * HD]
    in_scale = _pow2_scale(float(qkv.abs().max()))
    _lib.attention(q, B, N, H, HD, scale, out, _lib.ATT_F32, in_scale)
    torch.cuda.synchronize()
    return out, obuf, q, in_scale


def run_bwd(dev, qkv, dO, B, N, H, scale=SCALE, pad=0, in_fill=0.0, poison=float("nan")):
    """Forward then backward on the device, the workspace NaN-filled: (grad_qkv view, its whole buffer)."""
    from quantized_vit_amd import _lib
    from quantized_vit_amd.vit_model import _pow2_grad_scale
    out, _, q, in_scale = run_fwd(dev, qkv, B, N, H, scale, pad, in_fill)
    _, g = _pad(dO, dev, pad, in_fill)
    gbuf = torch.full((B * N, 3 * H * HD + pad), poison, dtype=torch.float32, device=dev)
    gq = gbuf[:, :3 * H * HD]
    lib = _lib.load()
    nb = int(lib.qvit_attention_backward_workspace_bytes(B, N, H))
    ws = torch.full((nb // 4,), float("nan"), dtype=torch.float32, device=dev)
    rc = lib.qvit_attention_backward(q.data_ptr(), out.data_ptr(), g.data_ptr(), B, N, H, HD, q.stride(0),
                                     out.stride(0), g.stride(0), scale, in_scale,
                                     _pow2_grad_scale(float(dO.abs().max())), gq.data_ptr(), gq.stride(0),
                                     ws.data_ptr(), nb, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return gq, gbuf


def check_fwd(name, o, o64, o32):
    err, errt = R.rel_err(o, o64), R.rel_err(o32, o64)
    ratio = err / max(errt, R.EPS32)
    print(f"{name}: fwd err = {err:.3e}  err_t = {errt:.3e}  ratio = {ratio:.2f}")
    assert bool(torch.isfinite(o).all()), name
    assert ratio <= C_FWD, (name, ratio)


def check_bwd(name, g, g64, g32, H, denoms=None):
    errs = R.section_errs(g, g64, H, HD, denoms)
    errt = R.section_errs(g32, g64, H, HD, denoms)
    ratios = [e / max(t, R.EPS32) for e, t in zip(errs, errt)]
    print(f"{name}: err dq/dk/dv = {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e}  err_t = {errt[0]:.3e} {errt[1]:.3e} "
          f"{errt[2]:.3e}  ratio = {ratios[0]:.2f} {ratios[1]:.2f} {ratios[2]:.2f}")
    assert bool(torch.isfinite(g).all()), name
    for sec, r in zip(("dq", "dk", "dv"), ratios):
        assert r <= C_BWD, (name, sec, r)


@pytest.mark.parametrize("B,N,H", SHAPES)
def test_forward_vs_float64(dev, B, N, H):
    qkv, _, o64, o32, _, _ = R.case(B, N, H, HD)
    o, _, _, _ = run_fwd(dev, qkv, B, N, H)
    check_fwd(f"forward B={B} N={N} H={H}", o, o64, o32)


@pytest.mark.parametrize("B,N,H", SHAPES)
def test_backward_vs_float64(dev, B, N, H):
    qkv, dO, _, _, g64, g32 = R.case(B, N, H, HD)
    g, _ = run_bwd(dev, qkv, dO, B, N, H)
    denoms = None
    if N == 1:   # dq = dk = 0 by cancellation of dP - D
        dq_s, dk_s = R.cancel_scales(qkv, dO, B, N, H, SCALE, HD)
        denoms = (dq_s, dk_s, None)
        assert float(g64[:, :2 * H * HD].abs().max()) == 0.0
    check_bwd(f"backward B={B} N={N} H={H}", g, g64, g32, H, denoms)


def test_row_strides_and_untouched_padding(dev):
    """qkv, out, grad_out and grad_qkv are views with 4 extra columns per row. The inputs' extra columns hold NaN
    (no read may leave a row's 3 H 80, resp. H 80, columns: a tail read one head or one section too far would
    show), the outputs' extra columns keep their poison, and the results are the contiguous call's bits."""
    B, N, H = 3, 33, 2
    qkv, dO, o64, o32, g64, g32 = R.case(B, N, H, HD)
    o, obuf, _, _ = run_fwd(dev, qkv, B, N, H, pad=4, in_fill=float("nan"), poison=-77.0)
    assert obuf.stride(0) == H * HD + 4
    check_fwd("padded strides", o, o64, o32)
    assert bool((obuf[:, H * HD:] == -77.0).all())
    g, gbuf = run_bwd(dev, qkv, dO, B, N, H, pad=4, in_fill=float("nan"), poison=-77.0)
    assert gbuf.stride(0) == 3 * H * HD + 4
    check_bwd("padded strides", g, g64, g32, H)
    assert bool((gbuf[:, 3 * H * HD:] == -77.0).all())
    assert torch.equal(o, run_fwd(dev, qkv, B, N, H)[0])
    assert torch.equal(g, run_bwd(dev, qkv, dO, B, N, H)[0])


def test_wider_qkv_gets_zero_gradient_columns(dev):
    from quantized_vit_amd.vit_model import _AttentionCore
    B, N, H = 3, 33, 2
    qkv, dO, _, _, g64, g32 = R.case(B, N, H, HD)
    wide = torch.cat([qkv, torch.full((B * N, 4), 3.0)], 1).to(dev).requires_grad_(True)
    out = _AttentionCore.apply(wide, B, N, H, SCALE, HD)
    assert out.shape == (B * N, H * HD)
    out.backward(dO.to(dev))
    assert wide.grad.shape == wide.shape and bool((wide.grad[:, 3 * H * HD:] == 0).all())
    check_bwd("wider qkv", wide.grad[:, :3 * H * HD], g64, g32, H)


# logits of std ~ 36 from |qkv| up to ~3e4 (in_scale = 1/2): q . k sums 80 products of std PEAK_STD^2
PEAK_STD = 6000.0
PEAK_SCALE = 36.0 / (PEAK_STD * PEAK_STD * HD ** 0.5)
PEAK = dict(B=1, N=70, H=2)


@pytest.mark.parametrize("log2_alpha", [-33, 20])   # dO scaled by ~1e-10 and ~1e6
def test_peaked_softmax_and_grad_scaling(dev, log2_alpha):
    from quantized_vit_amd.vit_model import _pow2_scale
    B, N, H = PEAK["B"], PEAK["N"], PEAK["H"]
    qkv, dO, o64, o32, g64, g32 = R.case(B, N, H, HD, 1, PEAK_STD, PEAK_STD, 1.0, PEAK_SCALE)
    assert 16384.0 < float(qkv.abs().max()) <= 32768.0 and _pow2_scale(float(qkv.abs().max())) == 0.5
    check_fwd("peaked", run_fwd(dev, qkv, B, N, H, PEAK_SCALE)[0], o64, o32)
    g1, _ = run_bwd(dev, qkv, dO, B, N, H, PEAK_SCALE)
    check_bwd("peaked alpha=1", g1, g64, g32, H)
    alpha = 2.0 ** log2_alpha
    ga, _ = run_bwd(dev, qkv, dO * alpha, B, N, H, PEAK_SCALE)
    check_bwd(f"peaked alpha=2^{log2_alpha}", ga, g64 * alpha, g32 * alpha, H)
    assert torch.equal(ga, g1 * alpha)    # grad(a dO) == a grad(dO) bit for bit (qvit_hip.h)


def test_deterministic(dev):
    """Two calls on NaN-filled outputs and workspaces (run_bwd fills both) give the same bits."""
    B, N, H = 2, 257, 2
    qkv, dO, _, _, _, _ = R.case(B, N, H, HD)
    a, _ = run_bwd(dev, qkv, dO, B, N, H)
    b, _ = run_bwd(dev, qkv, dO, B, N, H)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_argument_validation_launches_nothing(dev):
    from quantized_vit_amd import _lib
    lib = _lib.load()
    B, N, H = 1, 5, 2
    C = H * HD
    qkv = torch.zeros(B * N, 3 * C, device=dev)
    out = torch.full((B * N, C), 7.0, device=dev)
    codes = torch.full((B * N, C), 7, dtype=torch.int8, device=dev)
    go = torch.ones(B * N, C, device=dev)
    gq = torch.full((B * N, 3 * C), 5.0, device=dev)
    one = torch.ones(1, device=dev)
    nb = lib.qvit_attention_backward_workspace_bytes(B, N, H)
    ws = torch.full((nb // 4,), 9.0, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fwd(hd=HD, ldq=3 * C, mode=_lib.ATT_F32, o=out):
        return lib.qvit_attention(qkv.data_ptr(), B, N, H, hd, ldq, 0.125, 1.0, mode, o.data_ptr(), C,
                                  _lib.QT_LINEAR, one.data_ptr(), one.data_ptr(), None, 0, stream)

    def bwd(hd=HD, ldq=3 * C):
        return lib.qvit_attention_backward(qkv.data_ptr(), out.data_ptr(), go.data_ptr(), B, N, H, hd, ldq, C, C,
                                           0.125, 1.0, 1.0, gq.data_ptr(), 3 * C, ws.data_ptr(), nb, stream)
    # every buffer is large enough for head_dim <= 80; 96 is rejected for what it is, not for a bound
    assert fwd(hd=32) == EINVAL and fwd(hd=96, ldq=3 * H * 96) == EINVAL
    assert bwd(hd=32) == EINVAL and bwd(hd=96, ldq=3 * H * 96) == EINVAL
    assert fwd(ldq=3 * C - 4) == EINVAL and bwd(ldq=3 * C - 4) == EINVAL
    assert fwd(mode=_lib.ATT_I8, o=codes) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((codes == 7).all())
    assert bool((gq == 5.0).all()) and bool((ws == 9.0).all())   # nothing ran
