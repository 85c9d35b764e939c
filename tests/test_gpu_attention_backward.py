"""qvit_attention_backward against the float64 restatement of the reference attention (attention_backward_ref.py).

Metric, per section (dq, dk, dv) of grad_qkv: err = max |g - g64| / max |g64|; err_t is the same figure for the
fp32 CPU evaluation of the same expression, floored at fp32's eps (on trivial shapes the yardstick is exact by
luck, which the fp16 hi/lo operand split, 22 bits per operand, cannot be). The assertion is err <= C max(err_t, eps).
Where the true dq, dk vanish by cancellation (one key; dO constant along the rows of P) the denominator is the size
of the cancelling terms, scale max|dP| max|k| (max|q| for dk), for both err and err_t.

C: the worst err / max(err_t, eps) measured on an MI355X over the parity shapes below is recorded in DESIGN.md
section 12; C is the next power of two at or above twice that figure (the hi/lo split alone allows 4x per product
over two chained products, so a ratio above 16 would be a bug, not a bound to widen).
"""
import pytest
import torch

import attention_backward_ref as R

pytestmark = pytest.mark.gpu

C_BOUND = 8.0
SCALE = R.HD ** -0.5
SHAPES = [(1, 1, 1), (1, 5, 2), (2, 33, 2), (1, 64, 1), (2, 197, 2), (1, 257, 1), (1, 577, 2)]


def _pad(t, dev, pad, fill=0.0):
    """Device copy of the 2-D tensor as a view of a buffer with `pad` extra columns per row."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=torch.float32, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf, buf[:, :t.shape[1]]


def run_hip(dev, qkv, dO, B, N, H, scale=SCALE, pad=0, poison=None):
    """Forward (qvit_attention) then backward on the device; returns (grad_qkv view, its whole buffer)."""
    from quantized_vit_amd import _lib
    from quantized_vit_amd.vit_model import _pow2_grad_scale, _pow2_scale
    _, q = _pad(qkv, dev, pad)
    _, g = _pad(dO, dev, pad)
    obuf = torch.zeros((B * N, H * 64 + pad), dtype=torch.float32, device=dev)
    out = obuf[:, :H * 64]
    in_scale = _pow2_scale(float(qkv.abs().max()))
    _lib.attention(q, B, N, H, 64, scale, out, _lib.ATT_F32, in_scale)
    gbuf = torch.full((B * N, 3 * H * 64 + pad), float("nan") if poison is None else poison, dtype=torch.float32,
                      device=dev)
    gq = gbuf[:, :3 * H * 64]
    _lib.attention_backward(q, out, g, B, N, H, 64, scale, in_scale, _pow2_grad_scale(float(dO.abs().max())), gq)
    torch.cuda.synchronize()
    return gq, gbuf


def check(name, g, g64, g32, H, denoms=None):
    errs = R.section_errs(g, g64, H, denoms)
    errt = R.section_errs(g32, g64, H, denoms)
    ratios = [e / max(t, R.EPS32) for e, t in zip(errs, errt)]
    print(f"{name}: err dq/dk/dv = {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e}  err_t = {errt[0]:.3e} {errt[1]:.3e} "
          f"{errt[2]:.3e}  ratio = {ratios[0]:.2f} {ratios[1]:.2f} {ratios[2]:.2f}")
    assert bool(torch.isfinite(g).all()), name
    for sec, r in zip(("dq", "dk", "dv"), ratios):
        assert r <= C_BOUND, (name, sec, r)
    return ratios


@pytest.mark.parametrize("B,N,H", SHAPES)
def test_parity_vs_float64(dev, B, N, H):
    qkv, dO, g64, g32 = R.case(B, N, H)
    g, _ = run_hip(dev, qkv, dO, B, N, H)
    denoms = None
    if N == 1:   # dq = dk = 0 by cancellation of dP - D
        dq_s, dk_s = R.cancel_scales(qkv, dO, B, N, H, SCALE)
        denoms = (dq_s, dk_s, None)
        assert float(g64[:, :2 * H * 64].abs().max()) == 0.0
    check(f"parity B={B} N={N} H={H}", g, g64, g32, H, denoms)


# logits of std ~ 36 (the forward test's regime) from |qkv| up to ~3e4: in_scale = 1/2
PEAK_STD = 6000.0
PEAK_SCALE = 36.0 / (PEAK_STD * PEAK_STD * 8.0)
PEAK = dict(B=1, N=70, H=2)


@pytest.mark.parametrize("log2_alpha", [-33, 20])   # dO scaled by ~1e-10 and ~1e6
def test_peaked_softmax_and_grad_scaling(dev, log2_alpha):
    B, N, H = PEAK["B"], PEAK["N"], PEAK["H"]
    qkv, dO, g64, g32 = R.case(B, N, H, 1, PEAK_STD, PEAK_STD, 1.0, PEAK_SCALE)
    assert 16384.0 < float(qkv.abs().max()) <= 32768.0
    g1, _ = run_hip(dev, qkv, dO, B, N, H, PEAK_SCALE)
    check("peaked alpha=1", g1, g64, g32, H)
    alpha = 2.0 ** log2_alpha
    ga, _ = run_hip(dev, qkv, dO * alpha, B, N, H, PEAK_SCALE)
    check(f"peaked alpha=2^{log2_alpha}", ga, g64 * alpha, g32 * alpha, H)
    assert torch.equal(ga, g1 * alpha)


def test_row_strides_and_untouched_padding(dev):
    B, N, H = 2, 33, 2
    qkv, dO, g64, g32 = R.case(B, N, H)
    g, gbuf = run_hip(dev, qkv, dO, B, N, H, pad=64, poison=-77.0)
    assert gbuf.stride(0) == 3 * H * 64 + 64
    check("padded strides", g, g64, g32, H)
    assert bool((gbuf[:, 3 * H * 64:] == -77.0).all())
    g0, _ = run_hip(dev, qkv, dO, B, N, H)
    assert torch.equal(g, g0)


def test_deterministic(dev):
    B, N, H = 2, 197, 2
    qkv, dO, _, _ = R.case(B, N, H)
    a, _ = run_hip(dev, qkv, dO, B, N, H)
    b, _ = run_hip(dev, qkv, dO, B, N, H)
    assert torch.equal(a, b)


def test_zero_grad_out_gives_zero(dev):
    B, N, H = 2, 33, 2
    qkv, dO, _, _ = R.case(B, N, H)
    g, _ = run_hip(dev, qkv, torch.zeros_like(dO), B, N, H)
    assert bool((g == 0).all())


def test_grad_of_sum_has_no_dq_dk(dev):
    """Zero and linear: with dO = 1 (the gradient of sum(O)) dP_ij = sum_c v_jc. Where every value row has the same
    sum (here: every key carries the same value row, so O does not depend on P) dP is constant along each row of
    P, and since the rows of P sum to 1, dS = P (dP - D) = 0: dq = dk = 0."""
    B, N, H = 2, 33, 2
    qkv = R.case(B, N, H)[0].clone()
    C = H * 64
    qkv[:, 2 * C:] = qkv[0, 2 * C:]
    dO = torch.ones(B * N, C)
    g64 = R.grads(qkv, dO, B, N, H, SCALE, torch.float64)
    g32 = R.grads(qkv, dO, B, N, H, SCALE, torch.float32)
    dq_s, dk_s = R.cancel_scales(qkv, dO, B, N, H, SCALE)
    assert float(g64[:, :2 * C].abs().max()) <= 1e-12 * dq_s
    g, _ = run_hip(dev, qkv, dO, B, N, H)
    check("sum(O)", g, g64, g32, H, (dq_s, dk_s, None))


def test_argument_validation_launches_nothing(dev):
    from quantized_vit_amd import _lib
    lib = _lib.load()
    B, N, H = 1, 5, 2
    C = H * 64
    qkv = torch.zeros(B * N, 3 * C, device=dev)
    out = torch.zeros(B * N, C, device=dev)
    go = torch.ones(B * N, C, device=dev)
    gq = torch.full((B * N, 3 * C), 5.0, device=dev)
    nb = lib.qvit_attention_backward_workspace_bytes(B, N, H)
    ws = torch.full((nb // 4,), 9.0, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(hd=64, gqp=gq.data_ptr(), ldg=3 * C, wsb=nb):
        return lib.qvit_attention_backward(qkv.data_ptr(), out.data_ptr(), go.data_ptr(), B, N, H, hd, 3 * C, C, C,
                                           0.125, 1.0, 1.0, gqp, ldg, ws.data_ptr(), wsb, stream)
    assert call(hd=32) == -1
    assert call(gqp=None) == -3
    assert call(ldg=3 * C - 4) == -1
    assert call(wsb=nb - 1) == -1
    torch.cuda.synchronize()
    assert bool((gq == 5.0).all()) and bool((ws == 9.0).all())   # nothing ran


# ---- module level ----------------------------------------------------------------------------------------
MB, MN, MDIM, MH = 2, 40, 128, 2


def _module(dev, drop=0.0):
    from quantized_vit_amd.vit_model import ViTAttention
    torch.manual_seed(0)
    return ViTAttention(MDIM, num_heads=MH, qkv_bias=True, attn_drop_ratio=drop).to(dev)


def test_core_under_autograd_is_the_no_grad_kernel(dev):
    from quantized_vit_amd.vit_model import _AttentionCore
    attn = _module(dev).eval()
    qkv_c, dO_c, g64, g32 = R.case(MB, MN, MH, 2)
    qkv = qkv_c.reshape(MB, MN, -1).to(dev)
    with torch.no_grad():
        y0 = attn.core(qkv, MB, MN)
    x = qkv.clone().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        y = attn.core(x, MB, MN)
    assert torch.equal(y, y0)
    fn = y.grad_fn
    while fn is not None and "AttentionCore" not in type(fn).__name__:
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert fn is not None and type(fn).__name__.startswith(_AttentionCore.__name__)
    # nothing N x N is kept for the backward (the torch branch keeps the [B, H, N, N] softmax output)
    assert saved, "the Function saves qkv and the output"
    for shp in saved:
        assert not (len(shp) >= 2 and shp[-1] == MN and shp[-2] == MN), shp
        n = 1
        for d in shp:
            n *= d
        assert n != MB * MH * MN * MN and n <= MB * MN * 3 * MDIM, shp
    y.backward(dO_c.reshape(MB, MN, -1).to(dev))
    check("module core", x.grad.reshape(MB * MN, -1), g64, g32, MH)


def test_attention_dropout_keeps_the_torch_branch(dev):
    attn = _module(dev, drop=0.1).train()
    qkv_c, _, _, _ = R.case(MB, MN, MH, 2)
    x = qkv_c.reshape(MB, MN, -1).to(dev).requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(tuple(t.shape)), t)[1], lambda t: t):
        y = attn.core(x, MB, MN)
    assert "AttentionCore" not in type(y.grad_fn).__name__
    assert any(len(s) == 4 and s[-1] == MN and s[-2] == MN for s in saved)


def test_tiny_vit_gradients_match_the_torch_branch(dev, monkeypatch):
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType
    from quantized_vit_amd.quant_model import model_to_quantize_model
    from quantized_vit_amd.vit_model import ViTAttention, VisionTransformer
    torch.manual_seed(0)
    model = VisionTransformer(img_size=32, patch_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10)
    model = model_to_quantize_model(model.to(dev), num_bits=4, quant_type=QuantizationType.SYMMETRIC_LINEAR,
                                    quant_mode=QuantizationMode.WEIGHT_ONLY).eval()
    x = torch.randn(2, 3, 32, 32, device=dev)
    w = torch.randn(2, 10, device=dev)

    def run():
        model.zero_grad(set_to_none=True)
        (model(x) * w).sum().backward()
        return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}

    hip = run()
    monkeypatch.setattr(ViTAttention, "hip_ok", lambda self, qkv: False)
    ref = run()
    worst = 0.0
    for n in ref:
        den = float(ref[n].abs().max())
        err = float((hip[n] - ref[n]).abs().max()) / den if den > 0 else float(hip[n].abs().max())
        worst = max(worst, err)
        print(f"tiny ViT {n}: err = {err:.3e}")
        # both sides are fp32-class evaluations of the same graph: each is within err_t-class distance of the truth,
        # so their distance is bounded by (C + 1) yardstick errors; eps 64 is the fp32 yardstick's own scale for
        # sums over head_dim = 64 products
        assert err <= (C_BOUND + 1) * 64 * R.EPS32, n
    print(f"tiny ViT worst err = {worst:.3e}")
