"""Case table and CPU reference for the uint8 image input (qvit_im2col_u8_i8, qvit_u8_normalize_f32 and
QuantizeConv2d.set_uint8_input). Imports nothing from the library, so the table and the reference can be judged on
their own (tests/test_u8_input_ref_cpu.py).

The normaliser is torchvision's ToTensor then Normalize in float32: V[c][v] = (float32(v) / 255 - mean_c) / std_c,
mean_c and std_c rounded to float32 first. A byte has 256 values, so V is a [C][256] table, and the layer's activation
codes of a uint8 image are the oracle's quant_codes of V[c][img]. Reference rows: ref_rows = the F.unfold of those
per-pixel codes (conv_geometry_ref.unfold_rows), zero padding giving code 0.

PARAM_SETS are (mean, std, quantizer) combinations whose 768 table values all sit at least 5e-4 of a quantizer step
from a rounding tie, so the float32 and the float64 evaluation of the codes agree and a device result has to match
exactly (test_u8_input_ref_cpu.py shows it). TIE_SET has bytes 0 and 255 on a tie ((255 / 255 - 0.5) / 0.5 = 1.0 =
3.5 steps of 2 / 7, missed only by the rounding of d to float32); it is used only where both sides run the library's
own quantizer.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Callable, Optional, Tuple

import numpy as np
import torch

import conv_geometry_ref as G
from oracle import quant_oracle as O

HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


@dataclass(frozen=True)
class ParamSet:
    id: str
    mean: Tuple[float, ...]
    std: Tuple[float, ...]
    quantizer: str          # G.LINEAR / G.NONLINEAR
    q_m: float
    L: int                  # saturation code: d = float32(q_m**t / L)
    t: Optional[float] = None

    @property
    def d(self) -> float:
        return float(np.float32(self.q_m ** (self.t or 1.0) / self.L))

    def channels(self, C: int):
        """(mean, std) for C channels: the three values repeated in turn."""
        return tuple(self.mean[c % 3] for c in range(C)), tuple(self.std[c % 3] for c in range(C))


PARAM_SETS = (
    ParamSet("half-lin127", *HALF, G.LINEAR, 1.0, 127),
    ParamSet("half-nl7", *HALF, G.NONLINEAR, 1.0, 7, 0.8),
    ParamSet("inet-lin127", *IMAGENET, G.LINEAR, 2.0, 127),
    ParamSet("inet-nl7", *IMAGENET, G.NONLINEAR, 2.0, 7, 0.8),
    ParamSet("inet-nl127", *IMAGENET, G.NONLINEAR, 2.64, 127, 0.8),
)
TIE_SET = ParamSet("half-lin7-tie", *HALF, G.LINEAR, 2.0, 7)
PARAM_IDS = [p.id for p in PARAM_SETS]
MIN_TIE_DISTANCE = 5e-4    # quantizer steps


def value_table(mean, std) -> torch.Tensor:
    """V [C][256] float32: ToTensor (v / 255) then Normalize ((x - mean) / std), every operation in float32."""
    m = torch.tensor(mean, dtype=torch.float32)
    s = torch.tensor(std, dtype=torch.float32)
    v = torch.arange(256, dtype=torch.float32).div(255)
    return (v[None, :] - m[:, None]) / s[:, None]


def value_image(img_u8: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """table[c][img[b, c, y, x]] for a [B, C, H, W] uint8 image: the float32 NCHW image (the V-image)."""
    B, C, H, W = img_u8.shape
    idx = img_u8.permute(1, 0, 2, 3).reshape(C, -1).long()
    return torch.gather(table, 1, idx).view(C, B, H, W).permute(1, 0, 2, 3).contiguous()


def codes(x: torch.Tensor, ps: ParamSet, dtype=torch.float32) -> torch.Tensor:
    """The oracle's integer codes of x under ps's quantizer, evaluated in `dtype`."""
    kind = O.LINEAR if ps.quantizer == G.LINEAR else O.NONLINEAR
    return O.quant_codes(x.to(dtype), kind, ps.d, ps.q_m, ps.t)


def oracle_code_image(ps: ParamSet, dtype=torch.float32) -> Callable[[torch.Tensor], torch.Tensor]:
    """uint8 [B, C, H, W] -> per-pixel codes [B, C, H, W]: the oracle's codes of the V-image."""
    def fn(img_u8):
        return codes(value_image(img_u8, value_table(*ps.channels(img_u8.shape[1]))), ps, dtype)
    return fn


def ref_rows(img_u8: torch.Tensor, case: G.Case, code_image: Callable[[torch.Tensor], torch.Tensor]) -> torch.Tensor:
    """[B*OH*OW, K] im2col rows of the per-pixel codes code_image(img_u8)."""
    return G.unfold_rows(code_image(img_u8).float(), case)


def tie_distance(v: torch.Tensor, ps: ParamSet) -> torch.Tensor:
    """float64 distance, in steps, of every unsaturated non-zero value from the nearest rounding tie."""
    a = v.double().abs().reshape(-1)
    a = a[(a > 0) & (a < ps.q_m)]
    q = (a if ps.quantizer == G.LINEAR else torch.exp(ps.t * torch.log(a))) / float(np.float32(ps.d))
    return (q - torch.floor(q) - 0.5).abs()


# ---- cases ---------------------------------------------------------------------------------------------------------
_F1 = next(c for c in G.CASES if c.id == "F1")
_F4 = next(c for c in G.CASES if c.id == "F4")
U8_CASES = G.CASES + (
    replace(_F1, id="U1"),                                   # the 16-byte arms of both layouts
    replace(_F4, id="U2", fast=False),                       # W = 52: W % 16 != 0, just off the arm
    replace(_F1, id="U3", shifted=True, fast=False),         # U1 on a base shifted by 4 bytes
    replace(_F1, id="U4", C=4),                              # NCHW stays on its arm, NHWC misses C == 3
    G.Case("U5", 3, 28, 28, (14, 14), (14, 14), (0, 0), (1, 1)),   # the ViT-H/14 class: kw = 14, the scalar arm
)
U8_CASE_IDS = [c.id for c in U8_CASES]
NCHW, NHWC = 0, 1


def takes_vector_arm(case: G.Case, layout: int) -> bool:
    """Whether the call takes a 16-byte arm of qvit_im2col_u8_i8 (its header's conditions)."""
    ok = (case.k[1] % 16 == 0 and case.d[1] == 1 and case.p == (0, 0) and case.W % 16 == 0 and case.s[1] % 16 == 0
          and not case.shifted)
    return ok and (layout == NCHW or case.C == 3)


def make_image(case: G.Case, seed: Optional[int] = None) -> torch.Tensor:
    """uint8 [B, C, H, W]. Where a channel has at least 256 pixels, image 0 starts every channel with a permutation
    of all 256 byte values (a different one per channel), so each table entry is read; the rest is random."""
    if seed is None:
        seed = 7000 + U8_CASE_IDS.index(case.id)
    rng = np.random.default_rng(seed)
    B, C, H, W = case.xshape
    img = rng.integers(0, 256, size=(B, C, H * W), dtype=np.uint8)
    if H * W >= 256:
        for c in range(C):
            img[0, c, :256] = rng.permutation(256).astype(np.uint8)
    return torch.from_numpy(img).view(B, C, H, W)


def nhwc_bytes_as_nchw(img_u8: torch.Tensor) -> torch.Tensor:
    """The image a kernel sees that reads NHWC memory as NCHW: the layout swapped."""
    B, C, H, W = img_u8.shape
    return img_u8.permute(0, 2, 3, 1).contiguous().view(B, C, H, W)
