"""qvit_im2col_quant_i8 and QuantizeConv2d where the two axes differ: kh != kw, sh != sw, ph != pw, dh != dw and
H != W, on the kernel's patchify fast path, just off it, and on the generic arm; the int64_t instantiation; the
module on each of its four forward paths.

Bars: im2col codes are compared byte for byte (the inputs of tests/conv_geometry_ref.py are free of rounding ties:
tests/test_conv_geometry_ref_cpu.py); module outputs to the module bar of tests/test_gpu_model.py, 1e-5 relative."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_geometry_ref as G
import quant_backward_ref as R
from oracle import quant_oracle as O
from quantized_vit_amd import _lib
from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeConv2d

pytestmark = pytest.mark.gpu

FILL = 99


def _p(v, dev):
    return None if v is None else torch.tensor([float(v)], dtype=torch.float32, device=dev)


def _quantizer_args(quantizer, dev):
    """(qtype, d, q_m, t, levels) as the wrappers take them."""
    if quantizer == G.ULTRA_ACT:
        return _lib.QT_ULTRA_ACT, None, None, None, G.ULTRA_LEVELS
    d, q_m, t = G.quant_params(quantizer)
    qtype = _lib.QT_LINEAR if quantizer == G.LINEAR else _lib.QT_NONLINEAR
    return qtype, _p(d, dev), _p(q_m, dev), _p(t, dev), 0


def _to_device(x, case, dev):
    if not case.shifted:
        xd = x.to(dev)
        assert xd.data_ptr() % 16 == 0
        return xd
    base = torch.empty(x.numel() + 1, dtype=torch.float32, device=dev)
    xd = base[1:].view(x.shape)
    xd.copy_(x)
    assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    return xd


def _im2col(xd, case, q, out):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case.k, case.s, case.p, case.d
    _lib.im2col_quant_i8(xd, kh, kw, sh, sw, ph, pw, dh, dw, *q, out, case.kpad)
    torch.cuda.synchronize()


@pytest.mark.parametrize("quantizer", G.QUANTIZERS)
@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_im2col_geometry(dev, case, quantizer):
    x = G.make_input(case, quantizer)
    xd = _to_device(x, case, dev)
    q = _quantizer_args(quantizer, dev)
    rows, K, kpad, ldc = case.rows, case.K, case.kpad, case.ldc
    buf = torch.full((rows, ldc), FILL, dtype=torch.int8, device=dev)
    _im2col(xd, case, q, buf[:, :kpad])
    got = buf.cpu()
    ref = G.ref_codes(x, case, quantizer)
    assert torch.equal(got[:, :K], ref.to(torch.int8))
    assert (got[:, K:kpad] == 0).all()
    assert (got[:, kpad:] == FILL).all()      # nothing written past kpad
    # the same quantizer function through qvit_quantize_act_i8, gathered on the host
    B, C, H, W = case.xshape
    wpad = (W + 15) // 16 * 16
    own = torch.empty((B * C * H, wpad), dtype=torch.int8, device=dev)
    _lib.quantize_act_i8(xd.view(B * C * H, W), *q, own, wpad)
    torch.cuda.synchronize()
    own = own[:, :W].cpu().float().view(B, C, H, W)
    assert torch.equal(got[:, :K].float(), G.unfold_rows(own, case))


def test_im2col_int64_arm(dev):
    """rows * ldc = 2^31 takes im2col_quant_kernel<int64_t>; the same call into a compact buffer takes the int
    arm. Both give the reference."""
    case, ldc = G.INT64_CASE, G.INT64_LDC
    x = G.make_input(case, G.LINEAR)
    xd = _to_device(x, case, dev)
    q = _quantizer_args(G.LINEAR, dev)
    rows, K, kpad = case.rows, case.K, case.kpad
    compact = torch.full((rows, kpad), FILL, dtype=torch.int8, device=dev)
    _im2col(xd, case, q, compact)
    big = torch.empty((rows - 1) * ldc + kpad, dtype=torch.int8, device=dev)   # 2 GiB, never initialised
    wide = torch.as_strided(big, (rows, kpad), (ldc, 1))
    try:
        assert wide.stride(0) * rows == 2 ** 31 and wide.data_ptr() % 16 == 0
        _im2col(xd, case, q, wide)
        got = wide.contiguous().cpu()
    finally:
        del wide, big
        torch.cuda.empty_cache()
    ref = G.ref_codes(x, case, G.LINEAR).to(torch.int8)
    assert torch.equal(got, compact.cpu())
    assert torch.equal(got[:, :K], ref) and (got[:, K:] == 0).all()


# ---- the module -------------------------------------------------------------------------------------------------
MODULES = {
    "M1": (lambda: nn.Conv2d(5, 20, (2, 5), stride=(2, 3), padding=(3, 1), dilation=(3, 2), bias=True), (2, 5, 13, 22)),
    "M2": (lambda: nn.Conv2d(3, 24, (3, 16), stride=(1, 16), bias=True), (2, 3, 16, 48)),   # the im2col fast path
}
PATHS = ["wa4-int", "wonly4", "wonly16", "wa32-library"]


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _build_module(dev, geometry, path):
    make, xshape = MODULES[geometry]
    torch.manual_seed(PATHS.index(path) + 10 * list(MODULES).index(geometry))
    conv = make()
    mode = QuantizationMode.WEIGHT_AND_ACTIVATION if path.startswith("wa") else QuantizationMode.WEIGHT_ONLY
    bits = {"wa4-int": 4, "wonly4": 4, "wonly16": 16, "wa32-library": 32}[path]
    q = QuantizeConv2d.from_module(conv, quant_type=QuantizationType.SYMMETRIC_NONLINEAR, quant_mode=mode,
                                   num_bits=bits).to(dev).eval()
    assert (q.kernel_size, q.stride, q.padding, q.dilation) == (conv.kernel_size, conv.stride, conv.padding,
                                                                conv.dilation)
    plan = q.quant_plan()
    if path == "wa4-int":
        with torch.no_grad():
            q.q_m_act.fill_(1.0)
            q.d_quant_act.fill_(1.0 / 127)
        q.invalidate()
        plan = q.quant_plan()
        assert plan.int_path
        # activation codes off every rounding tie: the int8 codes of both sides are the same integers
        x = R.tie_free_values(xshape, R.NONLINEAR, 1.0 / 127, 1.0, 1.0, seed=5)
    elif path == "wonly4":
        assert not plan.int_path and plan.extra.get("wonly") and plan.wfmt == _lib.W4
        x = torch.randn(xshape)
    elif path == "wonly16":
        assert not plan.int_path and plan.extra.get("wonly") and plan.wfmt in (_lib.W16, _lib.W24)
        x = torch.randn(xshape)
    else:
        assert not plan.int_path and not plan.extra.get("wonly")
        x = (torch.rand(xshape) * 2 - 1) * 0.05
    return q, conv, x


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("geometry", list(MODULES))
def test_quantize_conv2d_geometry(dev, geometry, path):
    q, conv, x = _build_module(dev, geometry, path)
    with torch.no_grad():
        y = q(x.to(dev))
    y_grad = q(x.to(dev))
    assert y_grad.grad_fn is not None
    sd = {k: v.detach().cpu() for k, v in q.state_dict().items()}
    lq = O.LayerQ.from_state(sd, "", q.quant_type.value, q.quant_mode.value)
    ref = O.quantize_conv2d(x, sd["weight"], sd["bias"], lq, conv.stride, conv.padding, conv.dilation)
    assert ref.shape == F.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation).shape
    assert y.shape == ref.shape and y.is_contiguous()
    err = _rel(y, ref)
    print(f"{geometry} {path}: rel err {err:.3e}")
    assert err < 1e-5
    assert torch.equal(y_grad.detach(), y)       # the same forward under autograd, bit for bit
