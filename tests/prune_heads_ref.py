"""Head-geometry groups on tests/prune_step_ref.py's forms, by permutation and nothing else.

A head group's members have 3 * H * hd rows and unit h is the rows s * H * hd + h * hd + j (s in [0, 3), j in [0, hd)):
head h of a qkv projection as the forward's reshape(B, N, 3, H, hd) reads it. to_units permutes such a member
[3, H, hd, K] -> [H, 3 hd K]; on the permuted copy a head is row h, so the group is by construction one of
prune_step_ref's BASIC groups and its float64 / fp32 forms run on it unchanged: no second statement of the arithmetic
exists. The quantizer helpers and the per-element steps do not look at a tensor's shape, and every sum over a unit is a
sum over the same elements. from_units brings a result back.

HeadSpec names the members of one head group; permute / unpermute apply it to a whole dict of parameters or
gradients (NumPy arrays or torch tensors)."""
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np
import torch


@dataclass
class HeadSpec:
    members: List[str]
    heads: int
    head_dim: int


def _swap(x):
    return x.transpose(1, 0, 2, 3) if isinstance(x, np.ndarray) else x.permute(1, 0, 2, 3)


def to_units(x, heads: int, head_dim: int):
    """[3 * H * hd, ...] -> [H, 3 * hd * K] (a copy)."""
    assert x.shape[0] == 3 * heads * head_dim, (tuple(x.shape), heads, head_dim)
    y = _swap(x.reshape(3, heads, head_dim, -1)).reshape(heads, -1)
    return y.copy() if isinstance(y, np.ndarray) else y.clone()


def from_units(u, heads: int, head_dim: int, tail: Tuple[int, ...] = ()):
    """The inverse: [H, 3 * hd * K] -> [3 * H * hd, *tail]."""
    y = _swap(u.reshape(heads, 3, head_dim, -1)).reshape((3 * heads * head_dim,) + tuple(tail))
    return y.copy() if isinstance(y, np.ndarray) else y.clone()


def unit_rows(h: int, heads: int, head_dim: int) -> np.ndarray:
    """The physical rows of head h in the order to_units lays them out."""
    s = np.arange(3).reshape(3, 1)
    return ((s * heads + h) * head_dim + np.arange(head_dim).reshape(1, -1)).reshape(-1)


def permute(tensors: Dict[str, object], specs: List[HeadSpec]) -> Dict[str, object]:
    """A copy of the dict with every head member in unit form."""
    out = dict(tensors)
    for sp in specs:
        for m in sp.members:
            if m in out:
                out[m] = to_units(out[m], sp.heads, sp.head_dim)
    return out


def unpermute(tensors: Dict[str, object], specs: List[HeadSpec], shapes: Dict[str, Tuple[int, ...]]):
    """The inverse of permute; `shapes`: the members' original shapes."""
    out = dict(tensors)
    for sp in specs:
        for m in sp.members:
            if m in out:
                out[m] = from_units(out[m], sp.heads, sp.head_dim, tuple(shapes[m][1:]))
    return out


def rows_of_units(units, heads: int, head_dim: int) -> List[int]:
    """Sorted physical rows of the listed heads."""
    return sorted(int(r) for h in units for r in unit_rows(h, heads, head_dim))
