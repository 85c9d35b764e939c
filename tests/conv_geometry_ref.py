"""Case table and CPU reference for the per-axis geometry of qvit_im2col_quant_i8 and QuantizeConv2d: kernels,
strides, paddings and dilations that differ between the two axes, on images with H != W. Imports nothing from
the library, so the table and the reference can be judged on their own (tests/test_conv_geometry_ref_cpu.py).

Reference: ref_codes = F.unfold(codes(x), (kh, kw), (dh, dw), (ph, pw), (sh, sw)) as [B*OH*OW, K] rows, column
c*kh*kw + ih*kw + iw. codes is the oracle's quant_codes (LINEAR, NONLINEAR) or round(clamp(x, 0, 1) * levels)
(ULTRA_ACT); zero padding gives code 0 in all three.

Inputs sit 0.05 of a quantizer step away from every rounding tie and run past saturation on both sides, so the
float32 and the float64 evaluation of codes agree on every element and a device result has to match exactly.

gather_codes is the same gather written as index arithmetic (the kernel's: row r = (b, oh, ow), column
kk = (ci, ih, iw), y = oh*sh - ph + ih*dh, xx = ow*sw - pw + iw*dw, element ((b*C + ci)*H + y)*W + xx). Unmutated
it equals ref_codes; with one MUTATIONS entry it computes what a kernel with that fault would, the output shape
held (OH, OW and K come from the true geometry, as the host passes them). The CPU tests use it to show that the
table tells each fault from the correct result.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import quant_backward_ref as R
from oracle import quant_oracle as O

LINEAR, NONLINEAR, ULTRA_ACT = "linear", "nonlinear", "ultra_act"
QUANTIZERS = (LINEAR, NONLINEAR, ULTRA_ACT)
Q_M, T_NONLINEAR, ULTRA_LEVELS = 1.0, 0.8, 15


def quant_params(quantizer: str) -> Tuple[Optional[float], Optional[float], Optional[float]]:
    """(d, q_m, t) of the quantizer: 127 levels, d = q_m**t / 127."""
    if quantizer == ULTRA_ACT:
        return None, None, None
    t = None if quantizer == LINEAR else T_NONLINEAR
    return float(np.float32(Q_M ** (t or 1.0) / 127)), Q_M, t


@dataclass(frozen=True)
class Case:
    id: str
    C: int
    H: int
    W: int
    k: Tuple[int, int]
    s: Tuple[int, int]
    p: Tuple[int, int]
    d: Tuple[int, int]
    B: int = 2
    shifted: bool = False   # x starts 4 bytes into a larger buffer: its base is not 16-byte aligned
    fast: bool = False      # takes the kernel's patchify fast path (kw % 16 == 0, dw == 1, no padding, W % 4 == 0,
                            # sw % 4 == 0, an aligned base)

    @property
    def xshape(self):
        return (self.B, self.C, self.H, self.W)

    @property
    def K(self) -> int:
        return self.C * self.k[0] * self.k[1]

    @property
    def kpad(self) -> int:
        return (self.K + 15) // 16 * 16

    @property
    def ldc(self) -> int:
        return self.kpad + 16

    @property
    def out_hw(self) -> Tuple[int, int]:
        return out_hw(self.H, self.W, self.k, self.s, self.p, self.d)

    @property
    def rows(self) -> int:
        oh, ow = self.out_hw
        return self.B * oh * ow


def out_hw(H, W, k, s, p, d) -> Tuple[int, int]:
    return ((H + 2 * p[0] - d[0] * (k[0] - 1) - 1) // s[0] + 1, (W + 2 * p[1] - d[1] * (k[1] - 1) - 1) // s[1] + 1)


# The fast path's inner scalar fallback (y >= H or xx + 16 > W) is not in the table: a chunk of the fast path
# starts at y = oh*sh + ih*dh <= (OH-1)*sh + (kh-1)*dh < H and ends at xx + 16 <= (OW-1)*sw + kw <= W for every
# OH, OW the geometry admits, so no valid call reaches it.
CASES = (
    Case("F1", 3, 16, 48, (3, 16), (1, 16), (0, 0), (1, 1), fast=True),    # kh != kw
    Case("F2", 2, 9, 40, (2, 16), (2, 4), (0, 0), (3, 1), fast=True),      # dh > 1, patches overlap (sw < kw)
    Case("F3", 1, 5, 76, (1, 32), (1, 20), (0, 0), (1, 1), fast=True),     # two chunks per kernel row, gaps, a tail
    Case("F4", 3, 32, 52, (16, 16), (16, 16), (0, 0), (1, 1), fast=True),  # patch embed, 4 trailing columns
    Case("G1", 3, 16, 50, (3, 16), (1, 16), (0, 0), (1, 1)),               # just off the fast path: W % 4 != 0
    Case("G2", 3, 16, 48, (3, 16), (1, 6), (0, 0), (1, 1)),                # sw % 4 != 0
    Case("G3", 3, 16, 48, (3, 16), (1, 16), (0, 0), (1, 1), shifted=True),  # F1 on a base that is not aligned
    Case("G4", 3, 16, 48, (3, 16), (1, 16), (1, 0), (1, 1)),               # ph != 0
    Case("G5", 3, 16, 48, (3, 16), (1, 16), (0, 4), (1, 1)),               # pw != 0
    Case("G6", 3, 16, 64, (3, 16), (1, 16), (0, 0), (1, 2)),               # dw != 1
    Case("A1", 3, 13, 22, (2, 5), (2, 3), (3, 1), (3, 2)),   # all asymmetric; K = 30 straddles a chunk; top taps outside
    Case("A2", 4, 6, 19, (1, 7), (1, 2), (0, 3), (1, 1)),    # one-row kernel
    Case("A3", 4, 17, 5, (5, 1), (3, 1), (2, 0), (2, 1)),    # one-column kernel
    Case("A4", 1, 4, 9, (1, 3), (1, 1), (0, 1), (1, 1)),     # K = 3 < 16: kpad 16, ldc 32
    Case("A5", 2, 6, 6, (3, 3), (2, 2), (4, 4), (1, 1)),     # padding past the kernel's reach: whole rows are zero
    Case("A6", 5, 7, 11, (1, 1), (2, 3), (0, 0), (1, 1)),    # 1 x 1 with sh != sw
)
CASE_IDS = [c.id for c in CASES]

# the int64_t instantiation: OH = OW = 32, 2048 rows of K = 30 (kpad 32); the test gives it a row pitch of 2^20
INT64_CASE = Case("I64", 3, 29, 38, (2, 5), (1, 1), (3, 1), (3, 2))
INT64_LDC = 2 ** 20


def make_input(case: Case, quantizer: str, seed: Optional[int] = None) -> torch.Tensor:
    """Tie-free float32 values of the case's shape for the quantizer."""
    if seed is None:
        seed = 100 * (1 + QUANTIZERS.index(quantizer)) + (CASE_IDS.index(case.id) if case.id in CASE_IDS else 99)
    if quantizer == ULTRA_ACT:
        rng = np.random.default_rng(seed)
        n = int(np.prod(case.xshape))
        k = rng.integers(-2, 18, size=n).astype(np.float64)       # below 0 and above `levels`: both clamps occur
        f = rng.uniform(-0.45, 0.45, size=n)
        return torch.from_numpy(((k + f) / ULTRA_LEVELS).astype(np.float32)).reshape(case.xshape)
    d, q_m, t = quant_params(quantizer)
    kind = R.LINEAR if quantizer == LINEAR else R.NONLINEAR
    return R.tie_free_values(case.xshape, kind, d, q_m, t, seed)


def codes(x: torch.Tensor, quantizer: str, dtype=torch.float32) -> torch.Tensor:
    """The quantizer's integer codes of x, evaluated in `dtype` (the parameters are float32 values either way)."""
    x = x.to(dtype)
    if quantizer == ULTRA_ACT:
        return torch.round(torch.clamp(x, 0.0, 1.0) * ULTRA_LEVELS)
    d, q_m, t = quant_params(quantizer)
    return O.quant_codes(x, O.LINEAR if quantizer == LINEAR else O.NONLINEAR, d, q_m, t)


def unfold_rows(c: torch.Tensor, case: Case) -> torch.Tensor:
    """[B, C, H, W] codes -> [B*OH*OW, K] im2col rows."""
    return F.unfold(c, case.k, case.d, case.p, case.s).transpose(1, 2).reshape(case.rows, case.K)


def ref_codes(x: torch.Tensor, case: Case, quantizer: str, dtype=torch.float32) -> torch.Tensor:
    return unfold_rows(codes(x, quantizer, dtype), case)


# ---- the same gather as index arithmetic, with one fault at a time -------------------------------------------------
MUTATIONS = ("kh<->kw", "sh<->sw", "ph<->pw", "dh<->dw", "H<->W", "dilation ignored")
FAST_PATH_MUTATIONS = ("kh<->kw", "sh<->sw", "H<->W", "dilation ignored")   # what the fast path's arithmetic holds


def gather_codes(c: torch.Tensor, case: Case, mutation: Optional[str] = None) -> torch.Tensor:
    """[B*OH*OW, K] rows gathered from the codes c by the kernel's index arithmetic; `mutation` swaps one pair in
    that arithmetic (or drops the dilation). An index outside the image gives 0, as the kernel's bounds check does."""
    assert mutation is None or mutation in MUTATIONS
    B, C, H, W = case.xshape
    OH, OW = case.out_hw
    K = case.K
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case.k, case.s, case.p, case.d
    if mutation == "kh<->kw":
        kh, kw = kw, kh
    elif mutation == "sh<->sw":
        sh, sw = sw, sh
    elif mutation == "ph<->pw":
        ph, pw = pw, ph
    elif mutation == "dh<->dw":
        dh, dw = dw, dh
    elif mutation == "H<->W":
        H, W = W, H
    elif mutation == "dilation ignored":
        dh = dw = 1
    r = torch.arange(B * OH * OW).view(-1, 1)
    kk = torch.arange(K).view(1, -1)
    b, rem = r // (OH * OW), r % (OH * OW)
    oh, ow = rem // OW, rem % OW
    ci, r2 = kk // (kh * kw), kk % (kh * kw)
    ih, iw = r2 // kw, r2 % kw
    y = oh * sh - ph + ih * dh
    xx = ow * sw - pw + iw * dw
    inside = (y >= 0) & (y < H) & (xx >= 0) & (xx < W)
    idx = ((b * C + ci) * H + y) * W + xx
    flat = c.reshape(-1)
    assert int(idx[inside].max()) < flat.numel() and int(idx[inside].min()) >= 0
    return torch.where(inside, flat[idx.clamp(0, flat.numel() - 1)], torch.zeros((), dtype=c.dtype))
