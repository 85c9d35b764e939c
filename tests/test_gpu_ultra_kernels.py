"""Kernel-level tests of csrc/ultra_conv.hip on every path include/qvit_hip.h admits: each entry point against the
float64 / int64 restatements of tests/ultra_ref.py at small edge shapes, other bit widths than 4, both load arms of
layer 0, the staged and unstaged integer-accumulator arms, the multi-tile walk with a ragged tile count, and the
stand-alone decode, BN fold and weight quantizer. Code comparisons are tie-proven (ultra_ref.assert_codes_tie_proven:
equal outside the possible ties derived from the kernels' fp32 rounding, whose share tests/test_ultra_ref_cpu.py holds
under its cap on the reference alone); integer-deploy comparisons are exact."""
import numpy as np
import pytest
import torch

import ultra_ref as R
from oracle import ultranet_oracle as U
from quantized_vit_amd import _lib
from quantized_vit_amd._lib import _stream

pytestmark = pytest.mark.gpu

MODES = {"codes": _lib.ULTRA_CODES, "pool": _lib.ULTRA_CODES_POOL, "f32": _lib.ULTRA_F32}


def _ok(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _misaligned(t, dev, off):
    """t on the device `off` elements past a 16-byte boundary (a contiguous view of a larger buffer)."""
    esize = t.element_size()
    buf = torch.empty(t.numel() + 32, dtype=t.dtype, device=dev)
    start = ((16 - buf.data_ptr() % 16) % 16) // esize + off
    v = buf[start:start + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off * esize and v.is_contiguous()
    return v


def _conv(dev, c, cin, ks, cout, w_bit, a_bit, mode, pad=0):
    """qvit_ultra_conv with ldo = cout + pad; the pad columns must come back untouched."""
    B, H, W, _ = c.x.shape
    OH, OW = (H // 2, W // 2) if mode == "pool" else (H, W)
    f32 = mode == "f32"
    out = torch.full((B * OH * OW, cout + pad), 77, dtype=torch.float32 if f32 else torch.int8, device=dev)
    x, wc, al, sh = c.x.to(dev), c.wc.to(dev), c.alpha.to(dev), c.shift.to(dev)
    _ok(_lib.load().qvit_ultra_conv(x.data_ptr(), B, H, W, cin, ks, wc.data_ptr(), wc.shape[1], cout, w_bit, a_bit,
                                    None if f32 else al.data_ptr(), sh.data_ptr(), MODES[mode], out.data_ptr(),
                                    cout + pad, _stream(dev)), "qvit_ultra_conv")
    out = out.cpu()
    assert (out[:, cout:] == 77).all()
    return out[:, :cout].reshape(B, OH, OW, cout)


def _conv_int(dev, c, cin, cout, sbits, out_bit, pool, pad=0):
    B, H, W, _ = c.x.shape
    OH, OW = (H // 2, W // 2) if pool else (H, W)
    out = torch.full((B * OH * OW, cout + pad), 77, dtype=torch.int8, device=dev)
    x, wc, inc, bias = c.x.to(dev), c.wc.to(dev), c.inc.to(dev), c.bias.to(dev)
    _ok(_lib.load().qvit_ultra_conv_int(x.data_ptr(), B, H, W, cin, 3, wc.data_ptr(), wc.shape[1], cout,
                                        inc.data_ptr(), bias.data_ptr(), sbits, out_bit, 1 if pool else 0,
                                        out.data_ptr(), cout + pad, _stream(dev)), "qvit_ultra_conv_int")
    out = out.cpu()
    assert (out[:, cout:] == 77).all()
    return out[:, :cout].reshape(B, OH, OW, cout)


# ---- layer 0, float ------------------------------------------------------------------------------------------------
def _run_conv0(dev, c, a_bit, img_dev):
    return _lib.ultra_conv0(img_dev, c.wvals.to(dev), c.alpha.to(dev), c.shift.to(dev), a_bit).cpu()


@pytest.mark.parametrize("a_bit", R.CONV0_ABITS)
@pytest.mark.parametrize("size", R.CONV0_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_conv0(dev, size, a_bit):
    """Both load arms: W % 4 != 0 takes the scalar halo loads; at W % 4 == 0 the aligned image takes the 16-B quads
    and a copy 4 bytes off alignment the scalar loads, and the two must agree byte for byte. Odd H / W (floor
    pooling), images below one 16 x 32 tile, exactly one tile, several tiles; every other channel decreasing."""
    B, H, W = size
    c = R.conv0_case(B, H, W, a_bit)
    got = _run_conv0(dev, c, a_bit, c.img.to(dev))
    assert got.shape == (B, H // 2, W // 2, 16)
    R.assert_codes_tie_proven(got, c.codes, c.tie, R.CAP_CONV0)
    if W % 4 == 0:
        off = _run_conv0(dev, c, a_bit, _misaligned(c.img, dev, 1))
        assert torch.equal(off, got)
    else:
        assert size != R.CONV0_MISALIGNED


@pytest.mark.parametrize("H,W", R.CONV0_WALK_MAPS)
def test_conv0_walk(dev, H, W):
    """ntiles >= 2 * 8 * CUs (above any resident grid, so every block walks several tiles with the halo of the next
    one in flight) and ntiles % 8 != 0 (the XCD ranges of tile_walk differ in length); every image checked."""
    B = R.conv0_walk_batch(_cus(dev), H, W)
    c = R.conv0_case(B, H, W, 4)
    got = _run_conv0(dev, c, 4, c.img.to(dev))
    R.assert_codes_tie_proven(got, c.codes, c.tie, R.CAP_CONV0)


# ---- layer 0, integer ----------------------------------------------------------------------------------------------
def _run_conv0_int(dev, c, sbits, out_bit, img_dev):
    return _lib.ultra_conv0_int(img_dev, c.w.to(dev), c.inc.to(dev), c.bias.to(dev), sbits, out_bit).cpu()


@pytest.mark.parametrize("out_bit,sbits", R.CONV0_INT_BITS)
@pytest.mark.parametrize("size", R.CONV0_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_conv0_int(dev, size, out_bit, sbits):
    """Exact: pixels 0 and 255 (the x - 128 staging and the 128 sum(w) correction), inc_q of both signs (max / min
    pool), acc * inc_q beyond 32 bits in part of the elements, both load arms as in test_conv0."""
    B, H, W = size
    c = R.conv0_int_case(B, H, W, out_bit, sbits)
    assert R.product_overflows(c.acc, c.inc).any() and (c.inc < 0).any() and (c.inc > 0).any()
    got = _run_conv0_int(dev, c, sbits, out_bit, c.img.to(dev))
    assert torch.equal(got.to(torch.int64), c.codes)
    if W % 4 == 0:
        img = _misaligned(c.img, dev, 1)
        assert img.data_ptr() & 3
        assert torch.equal(_run_conv0_int(dev, c, sbits, out_bit, img), got)


@pytest.mark.parametrize("H,W", R.CONV0_WALK_MAPS)
def test_conv0_int_walk(dev, H, W):
    """The walk of test_conv0_walk on both integer load arms: scalar bytes (W % 4 = 2) and 4-B quads (W % 4 = 0)."""
    out_bit, sbits = R.WALK_INT_BITS
    B = R.conv0_walk_batch(_cus(dev), H, W)
    c = R.conv0_int_case(B, H, W, out_bit, sbits)
    got = _run_conv0_int(dev, c, sbits, out_bit, c.img.to(dev))
    assert torch.equal(got.to(torch.int64), c.codes)


# ---- layers 1..8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w_bit,a_bit", R.CONV_BITS)
@pytest.mark.parametrize("cin,ks,cout,mode,pad", R.CONV_CASES)
def test_conv(dev, cin, ks, cout, mode, pad, w_bit, a_bit):
    """Every (cin, ks) class at cout == COUT and below it, staged (pad 0) and unstaged (ldo = cout + 4) pooled arms,
    maps of one pixel / one pool window, ragged two-tile maps, den and levels of four bit-width pairs; a third of
    the channels decreasing (the bytewise weight negation of the staged arms, the min pool of the others)."""
    for shape in R.CONV_MAPS[mode]:
        c = R.conv_case(cin, ks, cout, mode, shape, w_bit, a_bit)
        got = _conv(dev, c, cin, ks, cout, w_bit, a_bit, mode, pad)
        if mode == "f32":                                     # zero bias: the quotient alone (test_acc_div_all_dens)
            c0 = R.Case(**{**c.__dict__, "shift": torch.zeros(cout)})
            q = _conv(dev, c0, cin, ks, cout, w_bit, a_bit, mode, pad)
            want = c.acc.double() / c.den
            assert ((q.double() - want).abs() <= 2.0 ** -23 * want.abs()).all(), shape
            assert torch.equal(q, c.acc.float() / torch.tensor(float(c.den))), shape
            assert _rel(got, want + c.shift.double()) <= 1e-5
        else:
            R.assert_codes_tie_proven(got, c.codes, c.tie, R.CAP_INT_ACC)


@pytest.mark.parametrize("mode", ["codes", "pool"])
def test_conv_max_accumulator(dev, mode):
    """8/7 bits on a constant full-scale map: accumulators of +-576 * 127 * 127 (near 2^23, the largest the ABI admits)
    through acc_div and the quantizer, unsaturated, on the CIN 64 unpooled and pooled (max / min) arms."""
    c = R.conv_max_case(mode)
    got = _conv(dev, c, 64, 3, 64, 8, 7, mode)
    R.assert_codes_tie_proven(got, c.codes, c.tie, R.CAP_INT_ACC)


def test_acc_div_all_dens(dev):
    """acc / den of the f32 epilogue for all 49 legal den on a (64, 1, 48) map whose accumulators run from 0 to
    64 * a_levels * w_levels: within one ulp of the quotient (the most an fp32 division may miss by). The count of
    quotients that are not the correctly rounded fp32 value was measured as 0 of 602112, so equality with
    the IEEE fp32 division is asserted."""
    B, H, W, cout = 1, 16, 16, 48
    g = torch.Generator().manual_seed(49)
    total = inexact = 0
    for w_bit in range(2, 9):
        for a_bit in range(1, 8):
            n, L = R.w_levels(w_bit), R.a_levels(a_bit)
            x = torch.randint(0, L + 1, (B, H, W, 64), generator=g)
            x[:, :, :4] = L                                   # columns of full-scale pixels
            x[:, :, 4:8] *= torch.rand((B, H, 4, 64), generator=g) < 0.1          # and of sparse ones
            w = torch.randint(-n, n + 1, (cout, 1, 1, 64), generator=g)
            w[0], w[1] = n, -n                                 # the largest accumulators of both signs
            w[2:6] *= torch.rand((4, 1, 1, 64), generator=g) < 0.05
            acc = R.conv_acc(x, w)
            c = R.Case(x=x.to(torch.int8), wc=R.pad_wcodes(w), alpha=torch.zeros(cout), shift=torch.zeros(cout))
            got = _conv(dev, c, 64, 1, cout, w_bit, a_bit, "f32")
            den = R.den_of(w_bit, a_bit)
            want = acc.double() / den
            assert int(acc.abs().max()) == 64 * n * L and (acc == 0).any()
            assert ((got.double() - want).abs() <= 2.0 ** -23 * want.abs()).all(), (w_bit, a_bit)
            exact = acc.float() / torch.tensor(float(den))    # IEEE fp32 division: the correctly rounded quotient
            inexact += int((got != exact).sum())
            total += acc.numel()
    print(f"acc_div: {inexact} of {total} quotients differ from the correctly rounded fp32 value")
    assert inexact == 0


@pytest.mark.parametrize("mode,pad,shape", [("codes", 0, (1, 1, 4)), ("pool", 0, (1, 2, 8)), ("pool", 4, (1, 2, 8))])
def test_round_half_to_even_known_answer(dev, mode, pad, shape):
    """w_bit 2, a_bit 1: den = levels = 1. alpha = 0.5, shift = 0 and acc = 1 give y = 0.5 exactly in fp32: the code
    is 0 (round half to even; half up would give 1); acc = 3 gives the clamped code 1, acc = 2 the code 1."""
    cin, cout = 16, 32
    counts = [1, 3, 2, 0]
    x = torch.zeros((*shape, cin), dtype=torch.int8)
    step = 2 if mode == "pool" else 1
    for j, k in enumerate(counts):
        x[0, :, step * j:step * (j + 1), :k] = 1              # k ones per pixel, the same in a whole pool window
    w = torch.zeros((cout, 3, 3, cin), dtype=torch.int64)
    w[:, 1, 1, :] = 1                                         # centre tap: acc = the pixel's count
    c = R.Case(x=x, wc=R.pad_wcodes(w), alpha=torch.full((cout,), 0.5), shift=torch.zeros(cout))
    got = _conv(dev, c, cin, 3, cout, 2, 1, mode, pad)
    assert got.shape == (1, 1, 4, cout)
    assert torch.equal(got[0, 0].to(torch.int64), torch.tensor([0, 1, 1, 0]).view(4, 1).expand(4, cout))


@pytest.mark.parametrize("cin,ks,cout,mode", R.CONV_WALK)
def test_conv_walk(dev, cin, ks, cout, mode):
    """2100 tiles on the 2048-block grid (2100 % 8 = 4: XCD ranges of 263 and 262 tiles, blocks with one and with two
    tiles, the second halo in flight under the first on the staged arms); every image checked."""
    c = R.conv_case(cin, ks, cout, mode, R.WALK_MAP, 4, 4, torch.float32)
    got = _conv(dev, c, cin, ks, cout, 4, 4, mode)
    R.assert_codes_tie_proven(got, c.codes, c.tie, R.CAP_INT_ACC)


# ---- integer layers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_bit,sbits", R.CONV_INT_BITS)
@pytest.mark.parametrize("cin,cout,pool,pad", R.CONV_INT_CASES)
def test_conv_int(dev, cin, cout, pool, pad, out_bit, sbits):
    """Exact against int_threshold (+ maxpool2): the staged arm and the unstaged one (cout below COUT or
    ldo = cout + 4) of every cin class, inc_q of both signs (min pool), acc * inc_q far beyond 32 bits."""
    c = R.conv_int_case(cin, cout, pool, R.CONV_INT_MAP, out_bit, sbits)
    assert int((c.acc * c.inc.to(torch.int64)).abs().max()) >= 2 ** 32
    got = _conv_int(dev, c, cin, cout, sbits, out_bit, pool, pad)
    assert torch.equal(got.to(torch.int64), c.codes)


@pytest.mark.parametrize("cin,cout", R.CONV_INT_WALK)
def test_conv_int_walk(dev, cin, cout):
    out_bit, sbits = R.WALK_INT_BITS
    c = R.conv_int_case(cin, cout, True, R.WALK_MAP, out_bit, sbits, torch.float32)
    got = _conv_int(dev, c, cin, cout, sbits, out_bit, True)
    assert torch.equal(got.to(torch.int64), c.codes)


# ---- the fused tail ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.TAIL_CASES, ids=lambda c: "-".join(map(str, c[:6])))
def test_tail(dev, case):
    """Maps of one row / column / pixel, the 26 x 26 maximum, more images than CUs, other bit widths, hout below and
    at 48. Layer by layer: the reference chain feeds each codes_ref the reference codes of the layer before, and an
    image counts when no layer of it holds a possible tie (at least half must). Head 1e-5 relative; with decode,
    p is the head and io is held at 1e-6 per element class to yolo_ref of the chain's head and of the kernel's own p."""
    B, H, W, w_bit, a_bit, hout, dec, gain = case
    B = _cus(dev) + 44 if B is None else B
    c = R.tail_case(B, H, W, w_bit, a_bit, hout, gain)
    assert 2 * int(c.clean.sum()) >= B
    dW = [l[1].to(dev) for l in c.layers]
    dA, dS = [l[2].to(dev) for l in c.layers], [l[3].to(dev) for l in c.layers]
    args = (c.x.to(dev), dW, dA, dS, c.hwc.to(dev), c.hbias.to(dev), hout, w_bit, a_bit)
    if dec is None:
        head = _lib.ultra_tail(*args).cpu()
    else:
        na, no = dec
        anchors = torch.rand((na, 2), generator=torch.Generator().manual_seed(na)) * 40 + 5
        io, p = _lib.ultra_tail(*args, decode=(anchors.to(dev), na, no, 16.0))
        io, p = io.cpu(), p.cpu()
        head = p.permute(0, 2, 3, 1, 4).reshape(B, H, W, hout)
        wio, _ = R.yolo_ref(head, na, no, anchors, 16.0)
        worst = max(_rel(io[c.clean][..., s], wio[c.clean][..., s]) for s in (slice(0, 2), slice(2, 4), slice(4, None)))
        cio, _ = R.yolo_ref(c.head, na, no, anchors, 16.0)    # and against the decode of the reference chain's head
        chain = max(_rel(io[c.clean][..., s], cio[c.clean][..., s]) for s in (slice(0, 2), slice(2, 4), slice(4, None)))
        print(f"tail decode {case}: worst class deviation {worst:.2e} (own p), {chain:.2e} (chain head)")
        assert worst <= 1e-6 and chain <= 1e-6
    dev_head = _rel(head[c.clean], c.head[c.clean])
    print(f"tail head {case}: {int(c.clean.sum())} of {B} images, deviation {dev_head:.2e}")
    assert dev_head <= 1e-5


# ---- the stand-alone decode ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ny,nx,na,no,pad", R.YOLO_CASES)
def test_yolo_decode(dev, B, ny, nx, na, no, pad):
    """ny != nx, na / no other than 6, ldh above na * no with NaN pad columns (never read), and a count above twice
    the capped grid's 256 * 16 * 256 threads, so every thread takes the grid-stride step."""
    head, anchors, stride = R.gen_head(B, ny, nx, na, no, na * no + pad, R.case_seed("yolo", B, ny, nx))
    if B == max(c[0] for c in R.YOLO_CASES):
        assert B * ny * nx * na * no >= 2 * 256 * 16 * 256
    io, p = _lib.yolo_decode(head.to(dev), na, no, anchors.to(dev), stride)
    io, p = io.cpu(), p.cpu()
    wio, wp = R.yolo_ref(head, na, no, anchors, stride)
    assert torch.isfinite(io).all() and torch.isfinite(p).all()
    assert torch.equal(p.double(), wp)
    worst = max(_rel(io[..., s], wio[..., s]) for s in (slice(0, 2), slice(2, 4), slice(4, None)))
    print(f"yolo_decode {(B, ny, nx, na, no)}: worst class deviation {worst:.2e}")
    assert worst <= 1e-6


# ---- BN fold and the weight quantizer ----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_gamma,with_beta", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("n", [1, 16, 257])
def test_bn_fold(dev, n, with_gamma, with_beta):
    g = torch.Generator().manual_seed(n)
    eps = float(np.float32(1e-5))
    var = torch.tensor([0.0, 1e-8, 1.0, 1e6])[(torch.arange(n) + n) % 4]
    mean = torch.randn(n, generator=g)
    gamma = (torch.rand(n, generator=g) + 0.5) * torch.where(torch.arange(n) % 3 == 2, -1.0, 1.0)
    beta = torch.randn(n, generator=g) * 0.3
    alpha, shift = torch.empty(n, device=dev), torch.empty(n, device=dev)
    dg, db, dm, dv = gamma.to(dev), beta.to(dev), mean.to(dev), var.to(dev)
    _ok(_lib.load().qvit_ultra_bn_fold(dg.data_ptr() if with_gamma else None, db.data_ptr() if with_beta else None,
                                       dm.data_ptr(), dv.data_ptr(), eps, n, alpha.data_ptr(), shift.data_ptr(),
                                       _stream(dev)), "qvit_ultra_bn_fold")
    ga = gamma.double() if with_gamma else torch.ones(n, dtype=torch.float64)
    be = beta.double() if with_beta else torch.zeros(n, dtype=torch.float64)
    wa = ga / torch.sqrt(var.double() + eps)
    ws = be - mean.double() * wa
    assert ((alpha.cpu().double() - wa).abs() <= 2.0 ** -22 * wa.abs()).all()
    assert ((shift.cpu().double() - ws).abs() <= 2.0 ** -22 * (be.abs() + (mean.double() * wa).abs())).all()


def _weight_codes(dev, w, w_bit, kpad, cout_pad):
    """qvit_ultra_weight_codes -> (codes [cout_pad][kpad], values, max |tanh| from the workspace)."""
    cout, cin, ks, _ = w.shape
    wd = w.to(dev).contiguous()
    codes = torch.full((cout_pad, kpad), 99, dtype=torch.int8, device=dev)
    vals = torch.empty_like(wd)
    ws = torch.zeros(1, dtype=torch.int32, device=dev)
    _ok(_lib.load().qvit_ultra_weight_codes(wd.data_ptr(), cout, cin, ks, w_bit, codes.data_ptr(), kpad, cout_pad,
                                            vals.data_ptr(), ws.data_ptr(), _stream(dev)), "qvit_ultra_weight_codes")
    return codes.cpu(), vals.cpu(), ws.cpu().view(torch.float32).item()


def _assert_weight_codes(codes, vals, w, w_bit):
    cout, cin, ks, _ = w.shape
    K, n = ks * ks * cin, R.w_levels(w_bit)
    _, tie = R.weight_ratio_ties(w, w_bit)
    want = U.weight_codes(w, w_bit).to(torch.int64)
    got = codes[:cout, :K].reshape(cout, ks, ks, cin).permute(0, 3, 1, 2).to(torch.int64)   # K order (ky, kx, c)
    R.assert_codes_tie_proven(got, want, tie, R.CAP_WEIGHT)
    assert (codes[cout:] == 0).all() and (codes[:, K:] == 0).all()
    assert torch.equal(vals, got.float() / float(n))
    assert int(got.abs().max()) == n


@pytest.mark.parametrize("w_bit", range(2, 9))
def test_weight_codes(dev, w_bit):
    """Against oracle.ultranet_oracle.weight_codes, tie-proven with the margin (2^(w_bit-1) - 1) 2^-21 on the scaled
    tanh ratio (the device tanh and the division are each within a few ulp; test_device_tanh_error): a random
    tensor, one with saturating weights (>= 10: tanh == 1.0f), one with a single non-zero element; padding zero."""
    cases = R.weight_cases(w_bit)
    w, sat, one = cases["random"], cases["saturating"], cases["single"]
    _assert_weight_codes(*_weight_codes(dev, w, w_bit, 192, 32)[:2], w, w_bit)
    codes, vals, m = _weight_codes(dev, sat, w_bit, 192, 32)
    assert m == 1.0
    _assert_weight_codes(codes, vals, sat, w_bit)
    codes, vals, m = _weight_codes(dev, one, w_bit, 64, 16)
    want = torch.zeros((16, 64), dtype=torch.int8)
    want[4, 37] = -R.w_levels(w_bit)
    assert torch.equal(codes, want) and vals[4, 37, 0, 0] == -1.0


def test_device_tanh_error(dev):
    """max |tanh| of a one-element tensor is the device tanhf of that element (read back from the workspace): its
    worst error over 512 points in ulps. The weight-code margin assumes a few ulp: at most 2 here."""
    xs = torch.cat([torch.linspace(-4, 4, 384), torch.logspace(-6, 1.2, 128)])
    worst = 0.0
    for x in xs.tolist():
        w = torch.tensor([[[[x]]]])
        _, _, m = _weight_codes(dev, w, 4, 16, 1)
        want = abs(np.tanh(np.float64(np.float32(x))))
        ulp = float(np.spacing(np.float32(want)))
        worst = max(worst, abs(m - want) / ulp)
    print(f"device tanhf: worst error {worst:.2f} ulp over {len(xs)} points")
    assert worst <= 2.0
