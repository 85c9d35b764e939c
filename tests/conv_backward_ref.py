"""CPU reference for the col2im (fold) behind QuantizeConv2d's input gradient: the adjoint of the im2col that
tests/conv_geometry_ref.py states, on the same 16-case table. Imports nothing from the library.

  fold_ref     F.fold in float64 on [B, K, L] (K = C kh kw in the weight's flattening order, L = OH OW).
  fold_gather  the same sum as index arithmetic, the kernel's: element (b, c, y, x) adds, ky ascending and inside it
               kx ascending, P[(b OH + oy) OW + ox][(c kh + ky) kw + kx] for the taps with
               (y + ph - ky dh) % sh == 0, oy = (y + ph - ky dh) / sh in [0, OH), and the x axis alike.
               With one MUTATIONS entry it computes what a kernel with that pair swapped would, OH and OW held.
  tap_counts   how many taps each image element has (0: no output position reads it).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from conv_geometry_ref import CASES, CASE_IDS, Case   # noqa: F401  (the table is shared by import)

MUTATIONS = ("kh<->kw", "sh<->sw", "ph<->pw", "dh<->dw")


def make_rows(case: Case, seed: int, integer: bool = False, dtype=torch.float32) -> torch.Tensor:
    """P [rows, K]: N(0, 1) values, or integers with |v| <= 1024 (every partial sum of at most kh kw <= 1024 of
    them is below 2^24, so an fp32 sum in any order is exact)."""
    gen = torch.Generator().manual_seed(seed)
    if integer:
        return torch.randint(-1024, 1025, (case.rows, case.K), generator=gen, dtype=torch.int64).to(dtype)
    return torch.randn((case.rows, case.K), generator=gen, dtype=torch.float64).to(dtype)


def fold_ref(P: torch.Tensor, case: Case) -> torch.Tensor:
    """[rows, K] -> [B, C, H, W] in float64 through F.fold."""
    B, OHW = case.B, case.out_hw[0] * case.out_hw[1]
    cols = P.double().reshape(B, OHW, case.K).transpose(1, 2)
    return F.fold(cols, (case.H, case.W), case.k, case.d, case.p, case.s)


def _taps(case: Case, mutation: Optional[str] = None):
    """For every image element and every (ky, kx): the row and column of P it adds, and whether the tap exists."""
    assert mutation is None or mutation in MUTATIONS
    B, C, H, W = case.xshape
    OH, OW = case.out_hw
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = case.k, case.s, case.p, case.d
    if mutation == "kh<->kw":
        kh, kw = kw, kh
    elif mutation == "sh<->sw":
        sh, sw = sw, sh
    elif mutation == "ph<->pw":
        ph, pw = pw, ph
    elif mutation == "dh<->dw":
        dh, dw = dw, dh
    e = torch.arange(B * C * H * W).view(-1, 1, 1)
    x, r = e % W, e // W
    y, bc = r % H, r // H
    c, b = bc % C, bc // C
    ky = torch.arange(kh).view(1, -1, 1)
    kx = torch.arange(kw).view(1, 1, -1)
    ry, rx = y + ph - ky * dh, x + pw - kx * dw
    oy, ox = torch.div(ry, sh, rounding_mode="floor"), torch.div(rx, sw, rounding_mode="floor")
    ok = (ry >= 0) & (ry % sh == 0) & (oy < OH) & (rx >= 0) & (rx % sw == 0) & (ox < OW)
    row = (b * OH + oy) * OW + ox
    col = (c * kh + ky) * kw + kx
    return row, col, ok


def fold_gather(P: torch.Tensor, case: Case, mutation: Optional[str] = None) -> torch.Tensor:
    """The fold as the kernel's gather, in float64, taps added in ascending (ky, kx). A mutated tap that leaves P
    contributes 0, as a kernel that bounds its reads would."""
    row, col, ok = _taps(case, mutation)
    ok = ok & (row >= 0) & (row < P.shape[0]) & (col < P.shape[1])
    Pd = P.double()
    vals = torch.where(ok, Pd[row.clamp(0, P.shape[0] - 1), col.clamp(0, P.shape[1] - 1)],
                       torch.zeros((), dtype=torch.float64))
    acc = torch.zeros(vals.shape[0], dtype=torch.float64)
    for i in range(vals.shape[1]):          # the fixed order (it matters to a float32 evaluation only)
        for j in range(vals.shape[2]):
            acc = acc + vals[:, i, j]
    return acc.view(case.xshape)


def tap_counts(case: Case) -> torch.Tensor:
    return _taps(case)[2].sum((1, 2)).view(case.xshape)


def tap_elements(case: Case, r: int, k: int) -> torch.Tensor:
    """Flat indices of the image elements that add P[r][k] (one, or none when the tap lies on the padding)."""
    row, col, ok = _taps(case)
    return (ok & (row == r) & (col == k)).any(2).any(1).nonzero().reshape(-1)
