"""The group-lasso penalty of the reference's training drivers (QViT_with_GETA/utils.py:157-194) and gl_scale
(base_hybrid_sparse_optimizer.py:293-333), restated over the units of quantized_vit_amd.qat_prune.units_view: in
float64 numpy, and as the literal fp32 torch form (torch.norm per unit, the multiply, the sum, autograd.grad). A
group is (members, sections, unit_rows); a unit's norm runs over all its members, as the device's does."""
import numpy as np
import torch

from quantized_vit_amd.qat_prune import units_view


def _units(members, sections, unit_rows):
    """[units, elements of a unit] over the members, and each member's columns in it."""
    n = members[0].shape[0] // (sections * unit_rows)
    views = [units_view(p, n, sections, unit_rows) for p in members]
    return torch.cat(views, dim=1), np.cumsum([0] + [v.shape[1] for v in views])


def penalty_f64(groups, scale, lam):
    """(sumsq per unit, loss, terms): terms[g][k] = lam scale_u p / ||unit u|| in member k's shape, 0 for a unit of
    norm 0. `scale`: one float64 per unit over the groups in order, or None."""
    sumsq, terms, u0 = [], [], 0
    for members, sections, unit_rows in groups:
        U, cols = _units([p.detach().cpu().double() for p in members], sections, unit_rows)
        U = U.numpy()
        n = U.shape[0]
        sc = np.ones(n) if scale is None else np.asarray(scale, dtype=np.float64)[u0:u0 + n]
        ss = (U * U).sum(axis=1)
        norm = np.sqrt(ss)
        T = np.where(norm[:, None] > 0, lam * sc[:, None] * U / np.where(norm > 0, norm, 1.0)[:, None], 0.0)
        back = []
        for k, p in enumerate(members):   # undo units_view's permutation
            t = torch.from_numpy(T[:, cols[k]:cols[k + 1]]).reshape(n, sections, unit_rows, -1).permute(1, 0, 2, 3)
            back.append(t.reshape(p.shape).numpy())
        sumsq.append(ss)
        terms.append(back)
        u0 += n
    sumsq = np.concatenate(sumsq)
    sc = np.ones_like(sumsq) if scale is None else np.asarray(scale, dtype=np.float64)
    return sumsq, float((sc * np.sqrt(sumsq)).sum()), terms


def penalty_torch(groups, scale, lam):
    """The literal form on the members' own device and dtype: returns gl_loss and adds lam * d gl_loss / dp into
    every member's .grad that exists (what loss.backward() leaves there)."""
    members = [p for g in groups for p in g[0]]
    leaves = [p.detach().requires_grad_(True) for p in members]
    loss, u0, i = torch.zeros(1, device=members[0].device), 0, 0
    for ms, sections, unit_rows in groups:
        U, _ = _units(leaves[i:i + len(ms)], sections, unit_rows)
        norm = torch.norm(U, dim=1)
        loss = loss + (norm if scale is None else norm * scale[u0:u0 + U.shape[0]]).sum()
        u0, i = u0 + U.shape[0], i + len(ms)
    for p, g in zip(members, torch.autograd.grad(lam * loss, leaves)):
        if p.grad is not None:
            p.grad.add_(g)
    return loss.detach()


def gl_scale_f64(scores, elems):
    """gl_scale from one score and one group_cost per unit."""
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.abs(np.asarray(scores, dtype=np.float64))
        inv = np.sqrt(np.maximum(np.asarray(elems, dtype=np.float64), 1.0)) / np.where(s < 1e-8, 1e-8, s)
        inv = np.where(np.isnan(inv), 1.0, np.clip(inv, 0.1, 10.0))   # torch.clamp keeps a NaN; nan_to_num: 1
    return inv / max(inv.mean(), 1e-8)
