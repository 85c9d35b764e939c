"""qvit_im2col_u8_i8 and qvit_u8_normalize_f32 on the device: every geometry of tests/u8_input_ref.py (the
conv-geometry table plus the cases on and just off the two 16-byte arms) in both image layouts, the int64_t
instantiations, and the table route against the library's own fp32 route.

Bars: everything is compared byte for byte (bit for bit for the fp32 image). The parameter sets of the oracle
comparison are free of rounding ties (tests/test_u8_input_ref_cpu.py), so the oracle's float32 codes are the only
correct answer; the tie set runs only where both sides are the library's quantizer."""
import functools

import pytest
import torch

import conv_geometry_ref as G
import u8_input_ref as U
from quantized_vit_amd import _lib

pytestmark = pytest.mark.gpu

FILL = 99
LAYOUTS = [U.NCHW, U.NHWC]
LAYOUT_IDS = ["nchw", "nhwc"]
CASES = {c.id: c for c in U.U8_CASES}
SETS = {p.id: p for p in U.PARAM_SETS + (U.TIE_SET,)}


def _p(v, dev):
    return None if v is None else torch.tensor([float(v)], dtype=torch.float32, device=dev)


def _quantizer_args(ps, dev):
    """(qtype, d, q_m, t, levels) as the wrappers take them."""
    qtype = _lib.QT_LINEAR if ps.quantizer == G.LINEAR else _lib.QT_NONLINEAR
    return qtype, _p(ps.d, dev), _p(ps.q_m, dev), _p(ps.t, dev), 0


def _device_image(img, case, layout, dev):
    """The [B, C, H, W] uint8 view the wrappers take, over NCHW or NHWC bytes, on a 16-byte aligned base or (a
    shifted case) 4 bytes past one."""
    B, C, H, W = img.shape
    flat = (img if layout == U.NCHW else img.permute(0, 2, 3, 1)).contiguous().reshape(-1)
    n = flat.numel()
    if case.shifted:
        base = torch.empty(n + 4, dtype=torch.uint8, device=dev)
        buf = base[4:]
    else:
        buf = torch.empty(n, dtype=torch.uint8, device=dev)
    buf.copy_(flat)
    assert buf.data_ptr() % 16 == (4 if case.shifted else 0)
    view = buf.view(B, C, H, W) if layout == U.NCHW else buf.view(B, H, W, C).permute(0, 3, 1, 2)
    assert _lib.u8_image_layout(view)[1] == layout or C == 1       # (one channel: the two layouts are the same bytes)
    assert _lib.u8_image_layout(view)[0].data_ptr() == buf.data_ptr()      # read in place
    return view


def _tables(ps, C, dev):
    """(V, T) on the device as the module builds them: V from the CPU, T = qvit_quantize_act_i8(V)."""
    V = U.value_table(*ps.channels(C)).contiguous().to(dev)
    T = torch.empty((C, 256), dtype=torch.int8, device=dev)
    _lib.quantize_act_i8(V, *_quantizer_args(ps, dev), T, 256)
    return V, T


def _im2col_u8(xd, case, T, out):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case.k, case.s, case.p, case.d
    _lib.im2col_u8_i8(xd, kh, kw, sh, sw, ph, pw, dh, dw, T, out, case.kpad)
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _reference(case_id, set_id):
    """(image, oracle rows) of a case under a parameter set, computed once for both layouts."""
    case, ps = CASES[case_id], SETS[set_id]
    img = U.make_image(case)
    return img, U.ref_rows(img, case, U.oracle_code_image(ps)).to(torch.int8)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("set_id", U.PARAM_IDS)
@pytest.mark.parametrize("case_id", U.U8_CASE_IDS)
def test_im2col_u8_vs_oracle(dev, case_id, set_id, layout):
    case, ps = CASES[case_id], SETS[set_id]
    img, ref = _reference(case_id, set_id)
    xd = _device_image(img, case, layout, dev)
    _, T = _tables(ps, case.C, dev)
    rows, K, kpad, ldc = case.rows, case.K, case.kpad, case.ldc
    buf = torch.full((rows, ldc), FILL, dtype=torch.int8, device=dev)
    _im2col_u8(xd, case, T, buf[:, :kpad])
    got = buf.cpu()
    assert torch.equal(got[:, :K], ref)
    assert (got[:, K:kpad] == 0).all()
    assert (got[:, kpad:] == FILL).all()      # nothing written past kpad


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("set_id", list(SETS))
@pytest.mark.parametrize("case_id", U.U8_CASE_IDS)
def test_im2col_u8_equals_fp32_route(dev, case_id, set_id, layout):
    """The table route against qvit_im2col_quant_i8 on qvit_u8_normalize_f32's image: the same bytes, ties included."""
    case, ps = CASES[case_id], SETS[set_id]
    img = U.make_image(case)
    if set_id == U.TIE_SET.id:
        img[0, :, 0, :2] = torch.tensor([0, 255], dtype=torch.uint8)     # the two bytes on the tie are there
    xd = _device_image(img, case, layout, dev)
    V, T = _tables(ps, case.C, dev)
    via_table = torch.full((case.rows, case.kpad), FILL, dtype=torch.int8, device=dev)
    _im2col_u8(xd, case, T, via_table)
    x32 = _lib.u8_normalize_f32(xd, V)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case.k, case.s, case.p, case.d
    via_fp32 = torch.full((case.rows, case.kpad), FILL, dtype=torch.int8, device=dev)
    _lib.im2col_quant_i8(x32, kh, kw, sh, sw, ph, pw, dh, dw, *_quantizer_args(ps, dev), via_fp32, case.kpad)
    torch.cuda.synchronize()
    assert torch.equal(via_table, via_fp32)


def test_im2col_u8_int64_arm(dev):
    """rows * ldc = 2^31 takes im2col_u8_kernel<int64_t>; the same call into a compact buffer takes the int arm.
    Both give the reference, in both layouts."""
    case, ldc = G.INT64_CASE, G.INT64_LDC
    ps = U.PARAM_SETS[2]
    img = U.make_image(case, seed=7099)
    ref = U.ref_rows(img, case, U.oracle_code_image(ps)).to(torch.int8)
    _, T = _tables(ps, case.C, dev)
    rows, K, kpad = case.rows, case.K, case.kpad
    big = torch.empty((rows - 1) * ldc + kpad, dtype=torch.int8, device=dev)   # 2 GiB, never initialised
    wide = torch.as_strided(big, (rows, kpad), (ldc, 1))
    try:
        assert wide.stride(0) * rows == 2 ** 31 and wide.data_ptr() % 16 == 0
        for layout in LAYOUTS:
            xd = _device_image(img, case, layout, dev)
            compact = torch.full((rows, kpad), FILL, dtype=torch.int8, device=dev)
            _im2col_u8(xd, case, T, compact)
            wide.fill_(FILL)
            _im2col_u8(xd, case, T, wide)
            got = wide.contiguous().cpu()
            assert torch.equal(got, compact.cpu()), layout
            assert torch.equal(got[:, :K], ref) and (got[:, K:] == 0).all(), layout
    finally:
        del wide, big
        torch.cuda.empty_cache()


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("case_id", U.U8_CASE_IDS)
def test_u8_normalize_is_the_table_gather(dev, case_id, layout):
    case, ps = CASES[case_id], U.PARAM_SETS[2]
    img = U.make_image(case)
    table = U.value_table(*ps.channels(case.C))
    xd = _device_image(img, case, layout, dev)
    out = _lib.u8_normalize_f32(xd, table.contiguous().to(dev))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == case.xshape
    assert torch.equal(out.cpu(), U.value_image(img, table))


def test_u8_normalize_int64_arm(dev):
    """B C H W = 2^31 takes u8_normalize_kernel<int64_t> (an 8 GiB image out, compared on the device one batch
    element at a time); NHWC, the layout whose source index is the longer product."""
    B, C, H, W = 8, 16, 4096, 4096
    ps = U.PARAM_SETS[2]
    V = U.value_table(*ps.channels(C)).contiguous().to(dev)
    g = torch.Generator(device=dev).manual_seed(11)
    buf = xd = out = None
    try:
        buf = torch.randint(0, 256, (B, H, W, C), dtype=torch.uint8, device=dev, generator=g)
        xd = buf.permute(0, 3, 1, 2)
        out = _lib.u8_normalize_f32(xd, V)
        torch.cuda.synchronize()
        assert out.numel() == 2 ** 31
        cidx = torch.arange(C, device=dev).view(C, 1, 1)
        for b in range(B):
            assert torch.equal(out[b], V[cidx, xd[b].long()]), b
    finally:
        del buf, xd, out
        torch.cuda.empty_cache()
