"""Reference restatements of the UltraNet kernels (csrc/ultra_conv.hip) on the CPU, in float64 / int64, the input
generators of tests/test_gpu_ultra_kernels.py and the tie-proven comparison. Nothing here imports the package.

Tie-proven comparison (as oracle/ties.py does for the ViT quantizers): the conv accumulators are exact integers, so
the only place the kernel and the reference can disagree is the rounding of v = clamp(y, 0, 1) * levels to a code
when v sits within the kernel's own fp32 rounding error of a half-integer. Every reference returns, beside the
codes, the mask of those *possible ties*, from a margin that is derived (below), not measured. Elements outside the
mask must be equal, elements inside may differ by one, and the mask must stay a small share of the elements
(`cap`), which the CPU test checks on the reference alone.

Margins:
  codes_ref   m = levels * 2^-22 * (|alpha * acc / den| + |shift|): the kernel does four fp32 roundings (acc_div,
              * alpha, + shift, * levels), each at most 2^-24 of a magnitude bounded by that sum.
  conv0_ref   m = levels * (|alpha| * S * 2^-21 + 2^-22 * (|alpha * conv| + |shift|)), S = sum |x w| over the 27
              taps: 2^-22 for the fp16 hi / lo split the header states, and as much again for the fp32
              accumulation, whose order differs from the reference's.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import quantization_np as Q

CAP_INT_ACC = 1e-3   # possible-tie share allowed for the integer-accumulator kernels
CAP_CONV0 = 1e-2     # and for the float layer 0
CAP_WEIGHT = 1e-3    # weight codes: 2 n 2^-21 <= 1.3e-4 of the ratios are possible ties by the margin


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def w_levels(w_bit: int) -> int:
    return 2 ** (w_bit - 1) - 1


def a_levels(a_bit: int) -> int:
    return 2 ** a_bit - 1


def den_of(w_bit: int, a_bit: int) -> int:
    return w_levels(w_bit) * a_levels(a_bit)


# ---- references --------------------------------------------------------------------------------------------
def conv_acc(x_codes_nhwc: torch.Tensor, w_codes_ohwi: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """Exact integer accumulators of the 'same'-padded conv: x [B][H][W][cin], w [cout][ks][ks][cin] -> int64
    [B][H][W][cout]. A float conv on integer data: every partial sum is an integer below 2^24, so exact in fp32 too."""
    cout, ks, ks2, cin = w_codes_ohwi.shape
    assert ks == ks2 and x_codes_nhwc.shape[3] == cin
    K = ks * ks * cin
    assert K * int(x_codes_nhwc.abs().max()) * int(w_codes_ohwi.abs().max()) < 2 ** 24
    y = F.conv2d(x_codes_nhwc.permute(0, 3, 1, 2).to(dtype), w_codes_ohwi.permute(0, 3, 1, 2).to(dtype), padding=ks // 2)
    return y.permute(0, 2, 3, 1).round().to(torch.int64).contiguous()


def _pool(t: torch.Tensor, reduce: str) -> torch.Tensor:
    """MaxPool2d(2, 2) of NHWC (floor: an odd last row / column is dropped); reduce = 'max' or 'any'."""
    B, H, W, C = t.shape
    v = t[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C)
    return v.amax(dim=(2, 4)) if reduce == "max" else v.any(dim=4).any(dim=2)


def _codes_and_ties(y: torch.Tensor, levels: int, margin: torch.Tensor, pool: bool):
    v = y.clamp(0, 1) * levels
    codes = torch.round(v).to(torch.int64)                   # torch.round: half to even
    tie = (v - (torch.floor(v) + 0.5)).abs() <= margin
    if pool:
        codes, tie = _pool(codes, "max"), _pool(tie, "any")
    return codes, tie


def codes_ref(acc: torch.Tensor, den: int, alpha: torch.Tensor, shift: torch.Tensor, levels: int, pool: bool):
    """code = rne(clamp(alpha * (acc / den) + shift, 0, 1) * levels) in float64 (+ 2x2 max pool on the codes) and
    the possible-tie mask (a pooled element is one if any element of its window is)."""
    a, s = alpha.double(), shift.double()
    t = a * (acc.double() / den)
    margin = levels * 2.0 ** -22 * (t.abs() + s.abs())
    return _codes_and_ties(t + s, levels, margin, pool)


def conv0_ref(img: torch.Tensor, wvals: torch.Tensor, alpha: torch.Tensor, shift: torch.Tensor, levels: int):
    """Layer 0: float64 conv of the fp32 image NCHW with the fake-quant weight values [16][3][3][3], BN, quantizer,
    2x2 max pool -> (codes NHWC [B][H/2][W/2][16], possible-tie mask)."""
    conv = F.conv2d(img.double(), wvals.double(), padding=1).permute(0, 2, 3, 1)
    S = F.conv2d(img.double().abs(), wvals.double().abs(), padding=1).permute(0, 2, 3, 1)
    a, s = alpha.double(), shift.double()
    margin = levels * (a.abs() * S * 2.0 ** -21 + 2.0 ** -22 * ((a * conv).abs() + s.abs()))
    return _codes_and_ties(a * conv + s, levels, margin, True)


def int_codes_ref(acc: torch.Tensor, inc: torch.Tensor, bias: torch.Tensor, sbits: int, out_bit: int, pool: bool):
    """Integer deploy stage on accumulators NHWC int64: quantization_np.int_threshold per channel (+ maxpool2)."""
    B, H, W, C = acc.shape
    a = acc.permute(3, 0, 1, 2).reshape(C, B * H, W).numpy()
    codes = Q.int_threshold(a, inc.numpy(), bias.numpy(), sbits, out_bit).reshape(C, B, H, W)
    if pool:
        codes = codes[:, :, :H // 2 * 2, :W // 2 * 2]        # floor pooling; rows pair up inside an image
        codes = Q.maxpool2(codes.reshape(C, B * (H // 2 * 2), W // 2 * 2)).reshape(C, B, H // 2, W // 2)
    return torch.from_numpy(np.ascontiguousarray(codes.transpose(1, 2, 3, 0)))


def conv0_int_acc(img_u8: torch.Tensor, wcodes: torch.Tensor) -> torch.Tensor:
    """Layer 0 of the integer deploy: uint8 pixels NCHW, weight codes [16][3][3][3] -> int64 NHWC accumulators."""
    assert 27 * 255 * int(wcodes.abs().max()) < 2 ** 24
    y = F.conv2d(img_u8.double(), wcodes.double(), padding=1)
    return y.permute(0, 2, 3, 1).round().to(torch.int64).contiguous()


def conv0_int_ref(img_u8, wcodes, inc, bias, sbits: int, out_bit: int) -> torch.Tensor:
    return int_codes_ref(conv0_int_acc(img_u8, wcodes), inc, bias, sbits, out_bit, True)


def yolo_ref(head_nhwc: torch.Tensor, na: int, no: int, anchors: torch.Tensor, stride: float):
    """YOLOLayer eval decode in float64 of the head output NHWC [B][ny][nx][>= na * no] (channel a * no + o) ->
    (io [B][na * ny * nx][no], p [B][na][ny][nx][no])."""
    B, ny, nx, _ = head_nhwc.shape
    p = head_nhwc[..., :na * no].double().reshape(B, ny, nx, na, no).permute(0, 3, 1, 2, 4).contiguous()
    yv, xv = torch.meshgrid(torch.arange(ny), torch.arange(nx), indexing="ij")
    grid = torch.stack((xv, yv), 2).double().view(1, 1, ny, nx, 2)
    anchor_vec = (anchors.double() / stride).view(1, na, 1, 1, 2)
    io = p.clone()
    io[..., :2] = (torch.sigmoid(p[..., :2]) + grid) * stride
    io[..., 2:4] = torch.exp(p[..., 2:4]) * anchor_vec * stride
    io[..., 4:] = torch.sigmoid(p[..., 4:])
    return io.view(B, -1, no), p


def tie_share(tie: torch.Tensor) -> float:
    return tie.double().mean().item() if tie.numel() else 0.0


def assert_codes_tie_proven(got: torch.Tensor, ref: torch.Tensor, possible_tie: torch.Tensor, cap: float) -> None:
    """Every element that is not a possible tie is equal, a possible tie differs by at most 1, and the possible ties
    are at most `cap` of the elements (otherwise the comparison would be vacuous)."""
    got, ref = got.cpu().to(torch.int64), ref.to(torch.int64)
    assert got.shape == ref.shape == possible_tie.shape, (got.shape, ref.shape, possible_tie.shape)
    share = tie_share(possible_tie)
    assert share <= cap, f"vacuous: possible ties are {share:.3e} of the elements, cap {cap:.1e}"
    d = (got - ref).abs()
    bad = (d > 0) & ~possible_tie
    assert not bad.any(), (f"{int(bad.sum())} of {d.numel()} codes differ outside possible ties; first at "
                           f"{bad.nonzero()[0].tolist()}: got {int(got[bad][0])}, want {int(ref[bad][0])}")
    assert int(d.max()) <= 1 if d.numel() else True, f"a possible tie is off by {int(d.max())}"


# ---- input generators (shared with tests/test_ultra_ref_cpu.py, which checks the caps on the reference alone) ----
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _second_moment_uniform(lo: int, hi: int) -> float:
    k = np.arange(lo, hi + 1, dtype=np.float64)
    return float((k * k).mean())


def pad_wcodes(w: torch.Tensor) -> torch.Tensor:
    """w [cout][ks][ks][cin] -> int8 [round_up(cout, 16)][round_up(K, 64)] in K order (ky, kx, c), zero padded."""
    cout = w.shape[0]
    K = w[0].numel()
    wc = torch.zeros((round_up(cout, 16), round_up(K, 64)), dtype=torch.int8)
    wc[:cout, :K] = w.reshape(cout, K).to(torch.int8)
    return wc


def gen_codes(shape, a_bit: int, seed: int) -> torch.Tensor:
    """Input codes NHWC uniform in 0 .. 2^a_bit - 1."""
    return torch.randint(0, a_levels(a_bit) + 1, shape, generator=_gen(seed), dtype=torch.int8)


def gen_conv_layer(cin: int, ks: int, cout: int, w_bit: int, a_bit: int, seed: int, gain: float = 1.0):
    """Weight codes uniform in +-(2^(w_bit-1) - 1) and random non-dyadic BN constants, scaled for this den so that
    the codes spread: y = alpha acc / den + shift has a per-channel spread of 0.15 .. 0.45 (x gain) around a shift
    in 0.1 .. 0.9. A third of the channels decrease in the accumulator (alpha < 0).
    Returns (w [cout][ks][ks][cin] int64, wc int8 padded, alpha fp32, shift fp32)."""
    g = _gen(seed)
    n = w_levels(w_bit)
    w = torch.randint(-n, n + 1, (cout, ks, ks, cin), generator=g)
    acc_std = math.sqrt(ks * ks * cin * _second_moment_uniform(0, a_levels(a_bit)) * _second_moment_uniform(-n, n))
    ystd = acc_std / den_of(w_bit, a_bit)
    alpha = (gain * 0.3 / ystd) * (torch.rand(cout, generator=g) + 0.5)
    alpha[2::3] *= -1
    shift = torch.rand(cout, generator=g) * 0.8 + 0.1
    return w, pad_wcodes(w), alpha.float(), shift.float()


def gen_conv0(B: int, H: int, W: int, seed: int):
    """Layer 0: an image in [0, 1) with exact 0 and 1 pixels, fake-quant weight values k / 7 and BN constants that
    spread the codes; every other channel has alpha < 0. Returns (img NCHW, wvals [16][3][3][3], alpha, shift)."""
    g = _gen(seed)
    img = torch.rand((B, 3, H, W), generator=g)
    r = torch.rand((B, 3, H, W), generator=g)
    img[r < 0.02] = 0.0
    img[r > 0.98] = 1.0
    wvals = torch.randint(-7, 8, (16, 3, 3, 3), generator=g).float() / 7
    ystd = math.sqrt(27 * (1.0 / 3) * _second_moment_uniform(-7, 7) / 49)
    alpha = (0.3 / ystd) * (torch.rand(16, generator=g) + 0.5)
    alpha[1::2] *= -1
    shift = torch.rand(16, generator=g) * 0.8 + 0.1
    return img, wvals, alpha.float(), shift.float()


I32_MAX = 2 ** 31 - 1


def gen_int_params(cout: int, acc_std: float, sbits: int, out_bit: int, g: torch.Generator):
    """inc_q / bias_q (int32) of the integer deploy with mixed signs. Channels 4k + 2 carry |inc| near 2^31 so that
    acc * inc leaves 32 bits by far (their codes saturate on the sign of the 64-bit sum); the others are scaled so
    that (acc inc + bias) >> sbits spreads over the codes, as far as int32 parameters can at this sbits."""
    L = a_levels(out_bit)
    mag = (0.3 * L * 2.0 ** sbits / acc_std) * (torch.rand(cout, generator=g).double() + 0.5)
    inc = mag.round().clamp(1, I32_MAX)
    inc[1::2] *= -1
    huge = torch.randint(2 ** 30, I32_MAX, (cout,), generator=g).double()
    inc[2::4] = huge[2::4] * torch.where(torch.arange(cout)[2::4] % 8 == 2, -1.0, 1.0)
    bias = ((torch.rand(cout, generator=g).double() * 0.8 + 0.1) * L * 2.0 ** sbits).round().clamp(-I32_MAX, I32_MAX)
    return inc.to(torch.int32), bias.to(torch.int32)


def _int_ranges(sbits: int):
    """(largest input code, largest |weight code|, taps kept per channel or None) by shift: small accumulators for a
    small shift (inc_q is an integer >= 1), the widest for shift_bits 40 (inc_q is at most 2^31)."""
    if sbits < 8:
        return 15, 1, 6
    if sbits < 32:
        return 15, 7, None
    return 127, 127, None


def _int_weights(shape, wmax: int, keep, g: torch.Generator) -> torch.Tensor:
    w = torch.randint(-wmax, wmax + 1, shape, generator=g)
    if keep is not None:                                      # sparse +-1: about `keep` taps per output channel
        K = w[0].numel()
        w = w * (torch.rand(shape, generator=g) < keep / K)
    return w


def gen_conv_int(cin: int, cout: int, sbits: int, out_bit: int, xshape, seed: int):
    """Integer layers 1..7: (x codes NHWC int8, w [cout][3][3][cin], wc padded, inc, bias)."""
    g = _gen(seed)
    xmax, wmax, keep = _int_ranges(sbits)
    x = torch.randint(0, xmax + 1, xshape, generator=g, dtype=torch.int8)
    w = _int_weights((cout, 3, 3, cin), wmax, keep, g)
    taps = 9 * cin if keep is None else keep
    acc_std = math.sqrt(taps * _second_moment_uniform(0, xmax) * _second_moment_uniform(-wmax, wmax) *
                        (1.0 if keep is None else 1.5))
    inc, bias = gen_int_params(cout, acc_std, sbits, out_bit, g)
    return x, w, pad_wcodes(w), inc, bias


def gen_conv0_int(B: int, H: int, W: int, sbits: int, out_bit: int, seed: int):
    """Integer layer 0: (uint8 image NCHW with pixels 0 and 255 present, weight codes [16][3][3][3] int8, inc, bias)."""
    g = _gen(seed)
    _, wmax, keep = _int_ranges(sbits)
    img = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    r = torch.rand(img.shape, generator=g)
    img[r < 0.03] = 0
    img[r > 0.97] = 255
    flat = img.view(-1)
    flat[0], flat[-1] = 255, 0
    w = _int_weights((16, 3, 3, 3), wmax, None if keep is None else 4, g)
    taps = 27 if keep is None else 4
    acc_std = math.sqrt(taps * _second_moment_uniform(0, 255) * _second_moment_uniform(-wmax, wmax) *
                        (1.0 if keep is None else 1.5))
    inc, bias = gen_int_params(16, acc_std, sbits, out_bit, g)
    return img, w.to(torch.int8), inc, bias


def gen_tail(H: int, W: int, B: int, w_bit: int, a_bit: int, hout: int, seed: int, gain: float = 1.0):
    """qvit_ultra_tail: input codes [B][H][W][64], four (64, 3, 64) layers and the 1x1 head (weights, padded codes
    [48][64], bias)."""
    x = gen_codes((B, H, W, 64), a_bit, seed)
    layers = [gen_conv_layer(64, 3, 64, w_bit, a_bit, seed + 1 + l, gain) for l in range(4)]
    hw, hwc, _, hbias = gen_conv_layer(64, 1, hout, w_bit, a_bit, seed + 9)
    hwc48 = torch.zeros((48, 64), dtype=torch.int8)
    hwc48[:hwc.shape[0]] = hwc[:48]
    return x, layers, hw, hwc48, hbias


def tail_ref(x, layers, hw, hbias, w_bit: int, a_bit: int):
    """The chain of four codes_ref (each fed the reference codes of the one before) and the float64 head.
    Returns (head [B][H][W][hout] float64, clean [B] bool: no possible tie in any layer of that image,
    the last layer's codes)."""
    den, L = den_of(w_bit, a_bit), a_levels(a_bit)
    h = x.to(torch.int64)
    clean = torch.ones(x.shape[0], dtype=torch.bool)
    for w, _, alpha, shift in layers:
        h, tie = codes_ref(conv_acc(h, w), den, alpha, shift, L, False)
        clean &= ~tie.flatten(1).any(dim=1)
    head = conv_acc(h, hw).double() / den + hbias.double()
    return head, clean, h


def gen_head(B: int, ny: int, nx: int, na: int, no: int, ldh: int, seed: int):
    """A head output NHWC [B][ny][nx][ldh] (pad columns NaN: they must not be read), anchors [na][2] and a stride."""
    g = _gen(seed)
    head = torch.full((B, ny, nx, ldh), float("nan"))
    head[..., :na * no] = torch.randn((B, ny, nx, na * no), generator=g) * 1.5
    anchors = torch.rand((na, 2), generator=g) * 40 + 5
    return head, anchors, 16.0


# ---- the parametrisations of tests/test_gpu_ultra_kernels.py -----------------------------------------------------
CONV0_SIZES = [(2, 2, 2), (1, 2, 6), (3, 18, 34), (2, 17, 33), (2, 33, 70), (1, 20, 36), (2, 16, 32), (2, 48, 64)]
CONV0_MISALIGNED = (1, 20, 36)            # run with the image at a misaligned address (VEC = false at W % 4 == 0)
CONV0_ABITS = [1, 4, 7]
CONV0_INT_BITS = [(1, 1), (4, 15), (7, 40), (4, 40), (7, 1)]    # (out_bit, shift_bits)
CONV0_WALK_MAPS = [(35, 70), (34, 68)]    # 9 ragged tiles each (the last one not empty), W % 4 = 2 and 0; B from the CU count


def conv0_walk_batch(cus: int, H: int, W: int) -> int:
    """The smallest B with ntiles >= 2 * 8 * cus and ntiles % 8 != 0 (16 x 32 tiles)."""
    per = ((H + 15) // 16) * ((W + 31) // 32)
    B = -(-2 * 8 * cus // per)
    while (B * per) % 8 == 0:
        B += 1
    return B

CONV_BITS = [(2, 1), (4, 4), (8, 7), (3, 5)]
# (cin, ks, cout, mode, ldo - cout): the staged arm needs cout == COUT and ldo % 16 == 0
CONV_CASES = [
    (16, 3, 32, "codes", 0), (16, 3, 32, "pool", 0), (16, 3, 32, "pool", 4),
    (16, 3, 20, "codes", 0), (16, 3, 20, "pool", 4),
    (32, 3, 64, "codes", 0), (32, 3, 64, "pool", 0), (32, 3, 64, "pool", 4),
    (32, 3, 52, "codes", 0), (32, 3, 52, "pool", 4),
    (64, 3, 64, "codes", 0), (64, 3, 64, "pool", 0),
    (64, 1, 36, "f32", 0), (64, 1, 48, "f32", 0),
]
CONV_MAPS = {"codes": [(2, 10, 14), (1, 1, 1), (3, 18, 34)], "f32": [(2, 10, 14), (1, 1, 1), (3, 18, 34)],
             "pool": [(2, 10, 14), (1, 2, 2), (3, 18, 34)]}
CONV_WALK = [(16, 3, 32, "pool"), (32, 3, 64, "pool"), (64, 3, 64, "pool"), (64, 3, 64, "codes")]
WALK_MAP = (350, 40, 24)                  # 6 ragged tiles each: 2100 tiles > the 2048-block grid, 2100 % 8 = 4

# (cin, cout, pool, ldo - cout)
CONV_INT_CASES = [(16, 32, True, 0), (16, 32, True, 4), (16, 32, False, 0), (16, 20, True, 4), (16, 20, False, 4),
                  (32, 64, True, 0), (32, 64, True, 4), (32, 64, False, 0), (32, 52, True, 4), (32, 52, False, 4),
                  (64, 64, True, 0), (64, 64, False, 0)]
CONV_INT_BITS = [(1, 1), (4, 15), (7, 40)]
CONV_INT_MAP = (3, 18, 34)
CONV_INT_WALK = [(16, 32), (32, 64)]
WALK_INT_BITS = (4, 15)                   # (out_bit, shift_bits) of the integer walk tests

NOMINAL_CUS = 256                         # the CPU test's stand-in for multi_processor_count
# (B or None = CUs + 44, H, W, w_bit, a_bit, hout, decode (na, no) or None, gain)
TAIL_CASES = [
    (2, 1, 1, 4, 4, 36, None, 1.0),
    (2, 1, 26, 8, 7, 48, None, 1.0),
    (2, 26, 1, 8, 7, 36, (3, 12), 1.0),
    (1, 26, 26, 4, 4, 36, (6, 6), 2.0),
    (1, 26, 26, 2, 1, 5, None, 1.0),
    (3, 13, 20, 4, 4, 5, None, 1.0),
    (3, 13, 20, 2, 1, 36, (6, 6), 1.0),
    (3, 13, 20, 8, 7, 36, None, 8.0),
    (None, 4, 3, 8, 7, 36, (6, 6), 1.0),
]

YOLO_CASES = [(1, 1, 1, 1, 5, 0), (2, 13, 20, 6, 6, 0), (3, 7, 5, 3, 12, 4), (17, 52, 52, 6, 8, 0)]  # ..., ldh - na no


def case_seed(*key) -> int:
    """A stable seed from a parametrisation (no hash(): it is salted per process)."""
    s = 17
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % 1000003
    return s


# ---- one parametrisation's inputs and reference (the same objects in the CPU and the GPU test) ---------------------
class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def conv_case(cin, ks, cout, mode, shape, w_bit, a_bit, dtype=torch.float64) -> Case:
    """qvit_ultra_conv: inputs, exact accumulators and (code modes) reference codes + possible ties."""
    seed = case_seed("conv", cin, ks, cout, mode, shape, w_bit, a_bit)
    w, wc, alpha, shift = gen_conv_layer(cin, ks, cout, w_bit, a_bit, seed)
    x = gen_codes((*shape, cin), a_bit, seed + 1)
    acc = conv_acc(x, w, dtype)
    c = Case(x=x, w=w, wc=wc, alpha=alpha, shift=shift, acc=acc, den=den_of(w_bit, a_bit), levels=a_levels(a_bit))
    if mode != "f32":
        c.codes, c.tie = codes_ref(acc, c.den, alpha, shift, c.levels, mode == "pool")
    return c


def conv0_case(B, H, W, a_bit) -> Case:
    img, wvals, alpha, shift = gen_conv0(B, H, W, case_seed("conv0", H, W))
    codes, tie = conv0_ref(img, wvals, alpha, shift, a_levels(a_bit))
    return Case(img=img, wvals=wvals, alpha=alpha, shift=shift, codes=codes, tie=tie)


def conv0_int_case(B, H, W, out_bit, sbits) -> Case:
    img, w, inc, bias = gen_conv0_int(B, H, W, sbits, out_bit, case_seed("conv0int", H, W, out_bit, sbits))
    acc = conv0_int_acc(img, w)
    return Case(img=img, w=w, inc=inc, bias=bias, acc=acc, codes=int_codes_ref(acc, inc, bias, sbits, out_bit, True))


def conv_int_case(cin, cout, pool, shape, out_bit, sbits, dtype=torch.float64) -> Case:
    x, w, wc, inc, bias = gen_conv_int(cin, cout, sbits, out_bit, (*shape, cin),
                                       case_seed("convint", cin, cout, shape, out_bit, sbits))
    acc = conv_acc(x, w, dtype)
    return Case(x=x, w=w, wc=wc, inc=inc, bias=bias, acc=acc, codes=int_codes_ref(acc, inc, bias, sbits, out_bit, pool))


def tail_case(B, H, W, w_bit, a_bit, hout, gain) -> Case:
    x, layers, hw, hwc, hbias = gen_tail(H, W, B, w_bit, a_bit, hout, case_seed("tail", H, W, w_bit, a_bit, hout), gain)
    head, clean, last = tail_ref(x, layers, hw, hbias, w_bit, a_bit)
    return Case(x=x, layers=layers, hw=hw, hwc=hwc, hbias=hbias, head=head, clean=clean, last=last)


def product_overflows(acc: torch.Tensor, inc: torch.Tensor) -> torch.Tensor:
    """Elements whose acc * inc_q does not fit 32 bits (the reason int_code is 64-bit)."""
    return (acc * inc.to(torch.int64)).abs() >= 2 ** 31


def conv_max_case(mode) -> Case:
    """(64, 3, 64) at 8/7 bits on a constant full-scale map: channels 0 and 1 have all weights +127 / -127, so the
    interior accumulators are +-576 * 127 * 127 (the largest the ABI admits, near 2^23) and the border ones 4/9
    and 6/9 of that; their BN maps the full-scale quotient 576 to 0.713, inside the code range. The other channels
    are a generated layer."""
    seed = case_seed("convmax", mode)
    w, _, alpha, shift = gen_conv_layer(64, 3, 64, 8, 7, seed)
    w[0], w[1] = 127, -127
    alpha[0], alpha[1], shift[0], shift[1] = 0.613 / 576, -0.613 / 576, 0.1, 0.1
    x = torch.full((2, 18, 20, 64), 127, dtype=torch.int8)
    acc = conv_acc(x, w)
    c = Case(x=x, w=w, wc=pad_wcodes(w), alpha=alpha, shift=shift, acc=acc, den=den_of(8, 7), levels=a_levels(7))
    c.codes, c.tie = codes_ref(acc, c.den, alpha, shift, c.levels, mode == "pool")
    return c


def weight_cases(w_bit: int) -> dict:
    """Float weights [cout][cin][ks][ks] for qvit_ultra_weight_codes: a random tensor, the same with saturating
    elements (>= 10: tanh == 1.0f), and one with a single non-zero element."""
    w = torch.randn((20, 16, 3, 3), generator=_gen(w_bit)) * 0.4
    sat = w.clone()
    sat[3, 2, 1, 0], sat[7, 5, 0, 2], sat[0, 0, 0, 0] = 10.0, -12.5, 40.0
    one = torch.zeros((5, 64, 1, 1))
    one[4, 37, 0, 0] = -0.3
    return {"random": w, "saturating": sat, "single": one}


def weight_ratio_ties(w: torch.Tensor, w_bit: int):
    """The scaled tanh ratio in float64 and its possible ties: margin (2^(w_bit-1) - 1) 2^-21."""
    n = w_levels(w_bit)
    t = torch.tanh(w.double())
    v = t / t.abs().max() * n
    return v, (v - (torch.floor(v) + 0.5)).abs() <= n * 2.0 ** -21
