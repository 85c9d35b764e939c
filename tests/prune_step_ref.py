"""Two restatements of the pruning stages of the reference's GETA optimizer for declared row groups, written from the
formulas of OTO/optimizer/geta.py:132-147 (the period schedule), :167-248 (identify_redundant_groups,
commit_redundant_idxes), :281-521 (compute_gamma_d), :806-850 (the quantize, clip and residual helpers), :873-1026
(the step) and OTO/optimizer/base_hybrid_sparse_optimizer.py:118-131, :194-211, :221-291 with importance_score/*.py,
on top of tests/qat_step_ref.py's two forms of the quantization-aware stages:

  (a) PruneF64    float64 NumPy;
  (b) PruneTorch  a per-parameter fp32 torch-CPU loop with .item() where the reference has one.

A group is (name, layer, members): `members` are parameter names sliced along dim 0, "<layer>.weight" among them is
the quantized member and "<layer>.d_quant_wt" / "q_m_wt" / "t_quant_wt" are its quantizer scalars. The reference's
"param group" of such a layer holds its weight, bias and all its quantizer scalars, so the layer's activation-side
scalars take the joint branch's activation pass with it.

Stated differences from the reference: gl_scale is computed there but read by nothing and is left out; the loop
`while d_quant < d_quant_lower` is cut after LOOP_CAP turns (the reference never ends for d_quant == 0), giving
d = d_quant_upper and gamma = 0; d is stored in the fp32 parameter in both forms.
"""
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from qat_step_ref import FIX, RANGE, WARMUP, Hyper, StepF64, StepTorch, d_of_bits, is_scalar, layer_of

SAFE_GUARD = 1e-8
LOOP_CAP = 861   # ceil(ln(FLT_MAX / FLT_TRUE_MIN) / ln(1.25))
DEFAULT_CRITERIA = {"magnitude": 0.2, "avg_magnitude": 0.2, "cosine_similarity": 0.2, "taylor_first_order": 0.2,
                    "taylor_second_order": 0.2}
CRITERIA_ORDER = tuple(DEFAULT_CRITERIA)
# gamma branches (bits 0..2 of the info word) and flags
MEAN_ZERO, NON_FINITE, SCHEDULE, NEGATIVE, CLAMP_POS, CLAMP_NEG = range(6)
D_UPPER, LOOPED, MIN_UPPER, CAPPED = 8, 16, 32, 64


@dataclass
class PruneHyper(Hyper):
    target_group_sparsity: float = 0.5
    start_pruning_step: int = 1
    pruning_steps: int = 1
    pruning_periods: int = 1
    group_divisible: int = 1
    criteria: Optional[Dict[str, float]] = None


@dataclass
class Group:
    name: str
    layer: str
    members: List[str]
    num_groups: int = 0
    prunable: bool = True
    start: int = 0
    important: List[int] = field(default_factory=list)
    active: List[int] = field(default_factory=list)
    pruned: List[int] = field(default_factory=list)


def active_num_redundant_groups(target: int, periods: int) -> List[int]:
    """geta.py:132-144."""
    out, total = [], 0
    for p in range(periods):
        if p == periods - 1:
            out.append(target - total)
        else:
            out.append(target // periods)
            total += out[p]
    return out


def select(scores: np.ndarray, pruned_global: List[int], n: int) -> List[int]:
    """geta.py:172-177: the curr_K lowest scores, minus those already taken; setdiff1d returns them sorted by index,
    so a surplus is cut by index and not by score."""
    k = len(pruned_global) + n
    top = torch.topk(-torch.as_tensor(scores), k)[1].numpy()
    return np.setdiff1d(top, pruned_global)[:n].tolist()


def refine(g: Group, group_divisible: int) -> int:
    """geta.py:188-236 on one group whose `active` holds the fresh selection; returns the change of
    target_num_redundant_groups."""
    delta = 0
    if g.num_groups < group_divisible:
        g.active.clear()
        g.pruned.clear()
    else:
        trial = len(g.important) - len(g.active)
        if trial % group_divisible != 0 or trial <= 0:
            ratio = trial // group_divisible + 1
            if ratio <= 1 or trial == 0:
                refined = max(int(group_divisible), 1)
            else:
                refined = max(int(ratio * group_divisible), int(group_divisible))
            refined = min(g.num_groups, refined)
            n_active = g.num_groups - len(g.pruned) - refined
            delta = n_active - len(g.active)
            g.active = g.active[:n_active]
    g.important = [i for i in g.important if i not in g.active and i not in g.pruned]
    return delta


def gamma_d_scalar(cg, cc, gg, rg, rr, csum, count, lr, period, t, q_m, t_quant, min_bit, max_bit):
    """compute_gamma_d's scalar part (geta.py:373-499) from the six sums, on Python floats. Returns (gamma, d, info):
    info = branch | flags."""
    eps, eta, zeta = 1e-8, 0.999, 0.9
    nc, ng, nr = math.sqrt(cc), math.sqrt(gg), math.sqrt(rr)

    def div(a, b):
        if b == 0.0 or math.isnan(b):
            return math.nan if (a == 0.0 or math.isnan(a) or math.isnan(b)) else math.copysign(math.inf, a)
        return a / b
    cos_clip, cos_res = div(cg, max(nc, eps) * ng), div(rg, max(nr, eps) * ng)
    schedule = 1.0 - (period - t - 1.0) / (period - t)
    if csum / count < 1e-8:
        rate, info = 0.0, MEAN_ZERO
    elif math.isinf(cos_clip) or math.isnan(cos_clip):
        rate, info = 0.0, NON_FINITE
    elif 0.0 <= cos_clip <= 1.0:
        rate, info = schedule, SCHEDULE
    elif -1.0 <= cos_clip < 0.0:
        rate, info = -(1 - eta) * lr * ng / (cos_clip * nc), NEGATIVE
    elif cos_clip > 1.0:
        rate, info = schedule, CLAMP_POS
    else:
        rate, info = -(1 - eta) * lr * ng / (-1.0 * nc), CLAMP_NEG
    upper, lower = d_of_bits(min_bit, q_m, t_quant), d_of_bits(max_bit, q_m, t_quant)
    if cos_res >= 0.0 or rate == 0.0:
        return rate, upper, info | D_UPPER
    d = div(-zeta * eta * lr * ng, rate * cos_res * nr)
    turns = 0
    while turns < LOOP_CAP and d < lower:
        rate, d, turns = rate * 0.8, d / 0.8, turns + 1
    if turns:
        info |= LOOPED
    if d < lower:
        return 0.0, upper, info | CAPPED
    if not d < upper:
        return rate, upper, info | MIN_UPPER
    return rate, d, info


def margins(cg, cc, gg, rg, rr, csum, count):
    """Relative distances of cos_clip, cos_res and mean(clip) from their branch thresholds (0, +-1; 0; 1e-8): the
    smallest must stay above 1e-3 for an input whose branch may not flip on rounding."""
    nc, ng, nr = math.sqrt(cc), math.sqrt(gg), math.sqrt(rr)
    out = [abs(csum / count - 1e-8) / max(abs(csum / count), 1e-8)]
    if ng > 0:
        for dot, n in ((cg, nc), (rg, nr)):
            c = dot / (max(n, 1e-8) * ng)
            out += [abs(c), abs(abs(c) - 1.0)]
    return min(out)


# ---- numerics, float64 ---------------------------------------------------------------------------------------------
def _pow64(a, t):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.exp(t * np.log(a))


def clip_res_quant_f64(w, d, q_m, t):
    """(_clip_helper, _residual_helper, _quantize_helper) of geta.py:806-850 on a float64 array."""
    t = 1.0 if t is None else t
    a = np.abs(w)
    rp = math.exp(t * math.log(abs(q_m)))
    pw = np.where(a >= q_m, rp, _pow64(a, t))
    pw = np.where(a <= 0.0, 0.0, pw)
    q = pw / d
    s = np.sign(w)
    return s * pw, s * (np.round(q) - q), s * (d * np.round(q))


def criteria_f64(pp, gg, pg, elems):
    n_p, n_g = np.sqrt(pp), np.sqrt(gg)
    t1 = np.abs(pg)
    return {"magnitude": n_p, "avg_magnitude": n_p / float(elems + 1e-6),
            "cosine_similarity": pg / (n_p + 1e-8) / (n_g + 1e-8) + 1, "taylor_first_order": t1,
            "taylor_second_order": 0.5 * t1 ** 2}


def overall_scores(per_group: List[Dict[str, np.ndarray]], weights: Dict[str, float]) -> List[np.ndarray]:
    """base_hybrid_sparse_optimizer.py:230-271 over every prunable group."""
    denoms = {}
    for c in CRITERIA_ORDER:
        if c in weights:
            denoms[c] = math.sqrt(SAFE_GUARD + sum(float(np.sum(np.asarray(g[c], dtype=np.float64) ** 2))
                                                   for g in per_group)) + SAFE_GUARD
    return [sum(np.asarray(g[c]) * (weights[c] / denoms[c]) for c in CRITERIA_ORDER if c in weights)
            for g in per_group]


# ---- the machine both forms share: integers only ------------------------------------------------------------------
class _PruneMachine:
    def init_prune(self, groups: List[Group]):
        hp = self.hp
        self.groups = groups
        self.total_num_groups = 0
        for g in groups:
            g.num_groups = int(self.p[g.members[0]].shape[0])
            assert all(self.p[m].shape[0] == g.num_groups for m in g.members)
            g.prunable = g.num_groups > hp.group_divisible
            if g.prunable:
                g.start = self.total_num_groups
                self.total_num_groups += g.num_groups
            g.important = list(range(g.num_groups))
        self.target = int(self.total_num_groups * min(hp.target_group_sparsity, 0.999))
        self.pruning_periods = int(max(1, hp.pruning_periods))
        self.pruning_period = hp.pruning_steps // self.pruning_periods
        self.curr_period = 0
        self.pruned_global: List[int] = []
        self.per_period = active_num_redundant_groups(self.target, self.pruning_periods)
        self.weights = dict(DEFAULT_CRITERIA if hp.criteria is None else hp.criteria)
        self.last: Dict[str, Tuple[float, float, int]] = {}   # group name -> (gamma, d, info) of the last joint step

    def advance(self) -> int:
        hp = self.hp
        self.num_steps += 1
        n = self.num_steps
        if hp.start_projection_step <= n <= hp.start_pruning_step and \
                hp.start_projection_step != hp.start_pruning_step:
            s = n - hp.start_projection_step - 1
            if s % self.period == 0 and s != 0:
                self.max_bit_wt = max(hp.min_bit_wt, 6, self.max_bit_wt - hp.bit_reduction)
                self.max_bit_act = max(hp.min_bit_act, 6, self.max_bit_act - hp.bit_reduction)
        if n <= hp.start_projection_step:
            return WARMUP
        return FIX if n > hp.start_pruning_step + hp.pruning_steps else RANGE

    def is_boundary(self) -> bool:
        n, hp = self.num_steps, self.hp
        return (n >= hp.start_pruning_step and self.curr_period < self.pruning_periods and self.pruning_period != 0
                and (n - hp.start_pruning_step - 1) % self.pruning_period == 0)

    def commit(self):
        for g in self.groups:
            if g.prunable:
                g.pruned.extend(g.active)
                g.active = []
                g.important = [i for i in range(g.num_groups) if i not in g.pruned]

    def identify(self, scores: np.ndarray):
        chosen = select(scores, self.pruned_global, self.per_period[self.curr_period])
        self.pruned_global.extend(chosen)
        for g in self.groups:
            if g.prunable:
                ids = np.arange(g.start, g.start + g.num_groups)
                g.active = (np.intersect1d(chosen, ids) - g.start).tolist()
                self.target += refine(g, self.hp.group_divisible)
        self.curr_period += 1

    def pruned_rows(self):
        return {g.name: sorted(g.pruned) for g in self.groups}

    def joint_groups(self):
        return [g for g in self.groups if g.prunable and g.active]

    def owned(self, joint):
        """Names of the parameters in the param groups of the joint layers: members and the layers' scalars."""
        names = set()
        for g in joint:
            names.update(g.members)
            names.update(k for k in self.p if is_scalar(k) and layer_of(k) == g.layer)
        return names

    def state(self):
        return {"pruned_idxes": {g.name: list(g.pruned) for g in self.groups},
                "active_redundant_idxes": {g.name: list(g.active) for g in self.groups},
                "curr_pruning_period": self.curr_period, "target_num_redundant_groups": self.target}

    def metrics(self, norms: Dict[str, np.ndarray]):
        """compute_metrics (geta.py:1028-1071) from each group's row norms."""
        m = dict(norm_params=0.0, norm_important_groups=0.0, norm_redundant_groups=0.0, num_zero_groups=0,
                 num_important_groups=0, num_redundant_groups=0)
        for g in self.groups:
            if not g.prunable:
                continue
            n = norms[g.name]
            red = g.active + g.pruned
            m["num_zero_groups"] += int(np.sum(n == 0))
            m["norm_params"] += float(np.sum(n))
            m["norm_important_groups"] += float(np.sum(n[g.important]))
            m["norm_redundant_groups"] += float(np.sum(n[red]))
            m["num_important_groups"] += len(g.important)
            m["num_redundant_groups"] += len(red)
        m["group_sparsity"] = m["num_zero_groups"] / float(self.total_num_groups + SAFE_GUARD)
        return m


# ---- (a) float64 ----------------------------------------------------------------------------------------------------
class PruneF64(_PruneMachine, StepF64):
    def __init__(self, params, hp: PruneHyper, groups: List[Group]):
        StepF64.__init__(self, params, hp)
        self.init_prune(groups)

    def _rows(self, a):
        return a.reshape(a.shape[0], -1)

    def scores(self, gv):
        per_group = []
        for g in self.groups:
            if not g.prunable:
                continue
            pp = gg = pg = 0.0
            elems = 0
            for m in g.members:
                p = self._rows(self.p[m])
                elems += p.shape[1]
                pp = pp + np.sum(p * p, axis=1)
                if m in gv:
                    gr = self._rows(gv[m])
                    gg = gg + np.sum(gr * gr, axis=1)
                    pg = pg + np.sum(p * gr, axis=1)
            self.last_sums = getattr(self, "last_sums", {})
            self.last_sums[g.name] = (pp, gg, pg)
            per_group.append(criteria_f64(pp, gg, pg, elems))
        self.last_scores = np.concatenate(overall_scores(per_group, self.weights))
        return self.last_scores

    def _wt_scalars(self, L):
        d = float(self.p[f"{L}.d_quant_wt"].reshape(-1)[0])
        q = float(self.p[f"{L}.q_m_wt"].reshape(-1)[0])
        t = self.p.get(f"{L}.t_quant_wt")
        return d, q, (None if t is None else float(t.reshape(-1)[0]))

    def six_sums(self, g, gv):
        """The six sums of compute_gamma_d over g's active rows and their element count."""
        d, q, t = self._wt_scalars(g.layer)
        s = np.zeros(6)
        count = 0
        for m in g.members:
            p = self.p[m]
            if m == f"{g.layer}.weight":
                clip, res, _ = clip_res_quant_f64(p, d, q, t)
            else:
                clip, res = p, np.zeros_like(p)
            c, r, gr = (x[g.active].ravel() for x in (clip, res, gv[m]))
            s += [c @ gr, c @ c, gr @ gr, r @ gr, r @ r, c.sum()]
            count += c.size
        return s, count

    def joint(self, g, gv, t_in_period):
        hp, L = self.hp, g.layer
        for s in ("d_quant_act", "q_m_act", "t_quant_act"):
            if f"{L}.{s}" in gv:
                self._descend(f"{L}.{s}", gv[f"{L}.{s}"], hp.lr_quant)
        if f"{L}.d_quant_act" in self.p:
            lo, hi = self.bounds(L, "act")
            self.p[f"{L}.d_quant_act"] = np.clip(self.p[f"{L}.d_quant_act"], float(np.float32(lo)),
                                                 float(np.float32(hi)))
        for s in ("t_quant_wt", "q_m_wt"):
            if f"{L}.{s}" in gv:
                self.p[f"{L}.{s}"] = self.p[f"{L}.{s}"] - hp.lr_quant * gv[f"{L}.{s}"]
        sums, count = self.six_sums(g, gv)
        self.last_six = getattr(self, "last_six", {})
        self.last_six[g.name] = (sums, count)
        _, q, t = self._wt_scalars(L)
        gamma, d, info = gamma_d_scalar(*sums, count, hp.lr, self.pruning_period, t_in_period, q, t,
                                        hp.min_bit_wt, self.max_bit_wt)
        d = float(np.float32(d))   # the parameter is fp32
        self.p[f"{L}.d_quant_wt"] = np.full_like(self.p[f"{L}.d_quant_wt"], d)
        self.last[g.name] = (gamma, d, info)
        for m in g.members:
            if m not in gv:
                continue
            p = self.p[m]
            if m == f"{L}.weight":
                p[g.active] = p[g.active] - gamma * clip_res_quant_f64(p, d, q, t)[2][g.active]
            else:
                p[g.active] = p[g.active] - gamma * p[g.active]
            self.p[m] = p - hp.lr * gv[m]

    def step(self, grads):
        stage = self.advance()
        hp = self.hp
        gv = self._variant(grads)
        self.last_gv = gv
        if self.is_boundary():
            self.commit()
            self.identify(self.scores(gv))
        t_in = (self.num_steps - hp.start_pruning_step) % self.pruning_period if self.pruning_period else 0
        joint = self.joint_groups()
        owned = self.owned(joint)
        if stage == FIX and not self.bits:
            from qat_step_ref import bit_width
            for layer in self.layers(self.p):
                self.bits[layer] = {}
                for side, key in (("wt", "weight"), ("act", "activation")):
                    if f"{layer}.d_quant_{side}" in self.p:
                        q, t = self._scalars(layer, side)
                        d = float(self.p[f"{layer}.d_quant_{side}"].reshape(-1)[0])
                        self.bits[layer][key] = round(bit_width(d, q, t))
        for k in self.p:
            if k not in gv or k in owned:
                continue
            if stage == RANGE and is_scalar(k) and k.endswith("_act"):
                self._descend(k, gv[k], hp.lr)
                self._descend(k, gv[k], hp.lr_quant)
            else:
                self._descend(k, gv[k], hp.lr_quant if is_scalar(k) else hp.lr)
        if stage != WARMUP:
            joint_layers = {g.layer for g in joint}
            for layer in self.layers(self.p):
                if layer in joint_layers:
                    continue
                for side, key in (("wt", "weight"), ("act", "activation")):
                    dk = f"{layer}.d_quant_{side}"
                    if dk not in self.p:
                        continue
                    if stage == RANGE:
                        lo, hi = self.bounds(layer, side)
                    else:
                        q, t = self._scalars(layer, side)
                        lo = hi = d_of_bits(self.bits[layer][key], q, t)
                    self.p[dk] = np.clip(self.p[dk], float(np.float32(lo)), float(np.float32(hi)))
        for g in joint:
            self.joint(g, gv, t_in)
        for g in self.groups:
            if g.pruned:
                for m in g.members:
                    self.p[m][g.pruned] = 0.0
        if self.pruning_period and self.num_steps >= hp.start_pruning_step and t_in == self.pruning_period - 1:
            self.commit()
        return stage

    def prune_metrics(self):
        return self.metrics({g.name: np.sqrt(sum(np.sum(self._rows(self.p[m]) ** 2, axis=1) for m in g.members))
                             for g in self.groups})


# ---- (b) fp32 torch, per parameter, .item() in the reference's places ----------------------------------------------
def _pow32(a, t):
    return torch.exp(t * torch.log(a))


def clip_res_quant_torch(w, d, q_m, t):
    """geta.py:806-850 literally: d, q_m, t are one-element tensors (t None: 1.0)."""
    t = 1.0 if t is None else t
    a = torch.abs(w)
    rp = torch.exp(t * torch.log(abs(q_m)))
    ip = _pow32(a, t)
    clip = ip.clone()
    clip[a <= 0.0] = 0
    clip[a >= q_m] = rp
    res = torch.round(ip.div(d)) - ip.div(d)
    res[a <= 0.0] = 0
    res[a >= q_m] = torch.round(rp.div(d)) - rp.div(d)
    qt = d * torch.round(ip.div(d))
    qt[a <= 0.0] = 0
    qt[a >= q_m] = d * torch.round(rp.div(d))
    s = torch.sign(w)
    return s * clip, s * res, s * qt


class PruneTorch(_PruneMachine, StepTorch):
    def __init__(self, params, hp: PruneHyper, groups: List[Group]):
        StepTorch.__init__(self, params, hp)
        self.init_prune(groups)

    def scores(self, gv):
        per_group = []
        for g in self.groups:
            if not g.prunable:
                continue
            norm = norm_g = ip = None
            elems = 0
            for m in g.members:
                p = self.p[m].reshape(g.num_groups, -1)
                elems += p.shape[1]
                n2 = torch.norm(p, dim=1) ** 2
                norm = n2 if norm is None else norm + n2
                if m in gv:
                    gr = gv[m].reshape(g.num_groups, -1)
                    g2 = torch.norm(gr, dim=1) ** 2
                    norm_g = g2 if norm_g is None else norm_g + g2
                    dot = torch.sum(p * gr, dim=1)
                    ip = dot if ip is None else ip + dot
            n_p, n_g = torch.sqrt(norm), torch.sqrt(norm_g)
            t1 = torch.abs(ip)
            per_group.append({"magnitude": n_p, "avg_magnitude": n_p / float(elems + 1e-6),
                              "cosine_similarity": ip / (n_p + 1e-8) / (n_g + 1e-8) + 1,
                              "taylor_first_order": t1, "taylor_second_order": 0.5 * t1 ** 2})
        denoms = {}
        for c in CRITERIA_ORDER:
            if c in self.weights:
                denoms[c] = np.sqrt(SAFE_GUARD + sum(torch.sum(g[c] ** 2, dim=0).item() for g in per_group)) + \
                    SAFE_GUARD
        out = []
        for g in per_group:
            overall = None
            for c in CRITERIA_ORDER:
                if c in self.weights:
                    term = g[c] * (self.weights[c] / denoms[c])
                    overall = term.clone() if overall is None else overall + term
            out.append(overall)
        self.last_scores = torch.cat(out, dim=0).numpy()
        return self.last_scores

    def compute_gamma_d(self, g, gv, t_in_period):
        """geta.py:281-521 with the loop cap."""
        hp, L = self.hp, g.layer
        d, q_m, t = self.p[f"{L}.d_quant_wt"], self.p[f"{L}.q_m_wt"], self.p.get(f"{L}.t_quant_wt")
        clips, ress, grads = [], [], []
        for m in g.members:
            p = self.p[m]
            if m == f"{L}.weight":
                clip, res, _ = clip_res_quant_torch(p, d, q_m, t)
            else:
                clip, res = p, torch.tensor([0.0]).to(p.device).expand_as(p)
            clips.append(clip[g.active].flatten())
            ress.append(res[g.active].flatten())
            grads.append(gv[m][g.active].flatten())
        fc, fg, fr = torch.cat(clips), torch.cat(grads), torch.cat(ress)
        nc, ng, nr = torch.norm(fc, p=2), torch.norm(fg, p=2), torch.norm(fr, p=2)
        eps, eta, zeta = 1e-8, 0.999, 0.9
        cos_clip = torch.div(torch.dot(fc, fg), torch.max(nc, torch.tensor(eps).to(fc.device)) * ng)
        cos_res = torch.div(torch.dot(fr, fg), torch.max(nr, torch.tensor(eps).to(fr.device)) * ng)
        D = self.pruning_period
        schedule = 1.0 - (D - t_in_period - 1.0) / (D - t_in_period)
        if torch.mean(fc).item() < 1e-8:
            rate, info = 0.0, MEAN_ZERO
        elif torch.isinf(cos_clip) or torch.isnan(cos_clip):
            rate, info = 0.0, NON_FINITE
        elif cos_clip >= 0.0 and cos_clip <= 1.0:
            rate, info = schedule, SCHEDULE
        elif cos_clip >= -1.0 and cos_clip < 0.0:
            rate, info = -(1 - eta) * hp.lr * ng / (cos_clip * nc), NEGATIVE
        else:
            clamped = torch.clamp(cos_clip, -1.0, 1.0)
            if clamped >= 0.0:
                rate, info = schedule, CLAMP_POS
            else:
                rate, info = -(1 - eta) * hp.lr * ng / (clamped * nc), CLAMP_NEG
        tq = None if t is None else t.item()
        upper = d_of_bits(hp.min_bit_wt, q_m.abs().max().item(), tq)
        lower = d_of_bits(self.max_bit_wt, q_m.abs().max().item(), tq)
        if cos_res >= 0.0 or rate == 0.0:
            return float(rate), upper, info | D_UPPER
        dq = -zeta * eta * hp.lr * ng / (rate * cos_res * nr)
        turns = 0
        while turns < LOOP_CAP and dq < lower:
            rate, dq, turns = rate * 0.8, dq / 0.8, turns + 1
        if turns:
            info |= LOOPED
        if dq < lower:
            return 0.0, upper, info | CAPPED
        if not dq < upper:
            return float(rate), upper, info | MIN_UPPER
        return float(rate), float(dq), info

    def joint(self, g, gv, t_in_period):
        hp, L = self.hp, g.layer
        for s in ("d_quant_act", "q_m_act", "t_quant_act"):
            if f"{L}.{s}" in gv:
                self._descend(f"{L}.{s}", gv[f"{L}.{s}"], hp.lr_quant)
        if f"{L}.d_quant_act" in self.p:
            q, t = self._scalars(L, "act")
            self.p[f"{L}.d_quant_act"].clamp_(min=d_of_bits(self.max_bit_act, q, t),
                                               max=d_of_bits(hp.min_bit_act, q, t))
        for s in ("t_quant_wt", "q_m_wt"):
            if f"{L}.{s}" in gv:
                self.p[f"{L}.{s}"].add_(gv[f"{L}.{s}"], alpha=-hp.lr_quant)
        gamma, d, info = self.compute_gamma_d(g, gv, t_in_period)
        with torch.no_grad():
            self.p[f"{L}.d_quant_wt"].copy_(torch.as_tensor(d))
        self.last[g.name] = (gamma, self.p[f"{L}.d_quant_wt"].item(), info)
        q_m, t = self.p[f"{L}.q_m_wt"], self.p.get(f"{L}.t_quant_wt")
        for m in g.members:
            if m not in gv:
                continue
            p = self.p[m]
            if m == f"{L}.weight":
                qw = clip_res_quant_torch(p, self.p[f"{L}.d_quant_wt"], q_m, t)[2]
                p[g.active] = p[g.active] - gamma * qw[g.active]
            else:
                p[g.active] = p[g.active] - gamma * p[g.active]
            p.add_(gv[m], alpha=-hp.lr)

    def step(self, grads):
        stage = self.advance()
        hp = self.hp
        gv = self._variant(grads)
        self.last_gv = gv
        if self.is_boundary():
            self.commit()
            self.identify(self.scores(gv))
        t_in = (self.num_steps - hp.start_pruning_step) % self.pruning_period if self.pruning_period else 0
        joint = self.joint_groups()
        owned = self.owned(joint)
        if stage == FIX and not self.bits:
            from qat_step_ref import bit_width
            for layer in self.layers(self.p):
                self.bits[layer] = {}
                for side, key in (("wt", "weight"), ("act", "activation")):
                    if f"{layer}.d_quant_{side}" in self.p:
                        q, t = self._scalars(layer, side)
                        self.bits[layer][key] = round(bit_width(self.p[f"{layer}.d_quant_{side}"].item(), q, t))
        for k in self.p:
            if k not in gv or k in owned:
                continue
            if stage == RANGE and is_scalar(k) and k.endswith("_act"):
                self._descend(k, gv[k], hp.lr)
                self._descend(k, gv[k], hp.lr_quant)
            else:
                self._descend(k, gv[k], hp.lr_quant if is_scalar(k) else hp.lr)
        if stage != WARMUP:
            joint_layers = {g.layer for g in joint}
            for layer in self.layers(self.p):
                if layer in joint_layers:
                    continue
                for side, key in (("wt", "weight"), ("act", "activation")):
                    dk = f"{layer}.d_quant_{side}"
                    if dk not in self.p:
                        continue
                    q, t = self._scalars(layer, side)
                    if stage == RANGE:
                        lo_b, hi_b = (self.max_bit_wt, hp.min_bit_wt) if side == "wt" else \
                            (self.max_bit_act, hp.min_bit_act)
                        lo, hi = d_of_bits(lo_b, q, t), d_of_bits(hi_b, q, t)
                    else:
                        lo = hi = d_of_bits(self.bits[layer][key], q, t)
                    self.p[dk].clamp_(min=lo, max=hi)
        for g in joint:
            self.joint(g, gv, t_in)
        for g in self.groups:
            if g.pruned:
                for m in g.members:
                    self.p[m][g.pruned] = 0.0
        if self.pruning_period and self.num_steps >= hp.start_pruning_step and t_in == self.pruning_period - 1:
            self.commit()
        return stage

    def prune_metrics(self):
        return self.metrics({g.name: torch.sqrt(sum(torch.norm(self.p[m].reshape(g.num_groups, -1), dim=1) ** 2
                                                    for m in g.members)).numpy() for g in self.groups})
