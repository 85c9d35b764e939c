"""The pruning stages of QuantAwareOptimizer (qat_optim.py) for declared row groups: the groups and their unit
geometry, the host's selection (geta.py:132-248), the device tables of the qvit_prune_* entry points (arrays of
_lib's descriptor dtypes, filled by field name) and _PruneState, which drives the launches of a step."""
from __future__ import annotations

from typing import TYPE_CHECKING, Dict, List

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import QvitError
from .quant_layers import QuantizeLinear

if TYPE_CHECKING:
    from .qat_optim import QuantAwareOptimizer

# Reference behaviour kept as it is:
#   * selection (geta.py:172-177): topk(-scores, len(pruned) + n), then np.setdiff1d against the rows already taken,
#     which returns the rest sorted by index, so a surplus is cut by index and not by score; then [:n];
#   * the group_divisible refinement (:188-228) with its adjustment of target_num_redundant_groups; rows it gives
#     back stay in the global list of taken rows, as in the reference, and are never selected again;
#   * rows committed at a period's last step are written as zeros from the next step on (:1022 runs before :1026);
#   * the joint branch steps the members without adamw's decay (:1008).
# Left out: gl_scale (base_hybrid_sparse_optimizer.py:293-333) is computed by the reference and read by nothing.
# The one difference: `while d_quant < d_quant_lower` (:494) never ends for d_quant == 0; the device cuts it after 861
# turns (x 1.25 per turn crosses fp32's exponent range) with d = d_quant_upper and gamma = 0.
# Heads: the reference's multihead_numhead_transformation is view(num_groups, -1), which on a [3 dim, dim] qkv weight
# groups contiguous rows and mixes the q rows of several heads; here a head is what the forward's reshape(B, N, 3, H,
# hd) makes of it (PruneGroup's sections and unit_rows).
# Out of scope: head-dim pruning, TRANSPOSE members, auxiliary groups, LoRA scores, the graph tracer and the verbose
# log files.
_CRITERIA = ("magnitude", "avg_magnitude", "cosine_similarity", "taylor_first_order", "taylor_second_order")


class PruneGroup:
    """One prunable group set: `members` are parameters sliced along dim 0 (the reference's TensorTransform.BASIC),
    all of the same shape[0]; `layer` is the QuantizeLinear whose weight quantizer scalars belong to the group. The
    layer's weight is the quantized member, every other member (its bias) is unquantized.

    `sections` and `unit_rows` make the prunable unit a set of rows: a member has sections * units * unit_rows rows
    and unit h is the rows s * units * unit_rows + h * unit_rows + j, s in [0, sections), j in [0, unit_rows). Both 1:
    unit r is row r. sections = 3, unit_rows = head_dim: head h of a qkv projection as reshape(B, N, 3, H, hd) reads
    it."""

    def __init__(self, name: str, layer: nn.Module, members: List[nn.Parameter], sections: int = 1,
                 unit_rows: int = 1):
        self.name, self.layer, self.members = str(name), layer, list(members)
        self.sections, self.unit_rows = sections, unit_rows


def unit_rows_of(units, num_units: int, sections: int = 1, unit_rows: int = 1) -> np.ndarray:
    """The physical rows of the listed units, unit after unit, each section-major with its rows ascending: the order
    in which the device folds a unit's sums and the joint stage lists a redundant unit's rows."""
    h = np.asarray(units, dtype=np.int64).reshape(-1, 1, 1)
    s = np.arange(sections, dtype=np.int64).reshape(1, -1, 1)
    j = np.arange(unit_rows, dtype=np.int64).reshape(1, 1, -1)
    return ((s * num_units + h) * unit_rows + j).reshape(-1)


def units_view(p: torch.Tensor, num_units: int, sections: int = 1, unit_rows: int = 1) -> torch.Tensor:
    """[num_units, elements of a unit] of a member: a view for a one-row geometry, else a permuted copy."""
    if sections == 1 and unit_rows == 1:
        return p.reshape(num_units, -1)
    return p.reshape(sections, num_units, unit_rows, -1).permute(1, 0, 2, 3).reshape(num_units, -1)


class _GroupState:
    """A declared group with the optimizer's own state of it (a PruneGroup list may serve several optimizers)."""

    def __init__(self, g: PruneGroup):
        self.name, self.layer, self.members = g.name, g.layer, list(g.members)
        self.sections, self.unit_rows = int(g.sections), int(g.unit_rows)
        self.rows = int(self.members[0].shape[0])                         # physical rows: the device's items
        self.num_groups = self.rows // (self.sections * self.unit_rows)   # prunable units
        self.basic = self.sections == 1 and self.unit_rows == 1
        self.prunable = True
        self.start = 0                      # global index of row 0 among the prunable groups
        self.important: List[int] = list(range(self.num_groups))
        self.active: List[int] = []         # active_redundant_idxes
        self.pruned: List[int] = []         # pruned_idxes


def _check_prune_groups(groups: List[PruneGroup]) -> None:
    """What the constructor rejects with ValueError, before it looks at the rest of the model."""
    seen = set()
    for g in groups:
        if not isinstance(g.layer, QuantizeLinear) or getattr(g.layer, "d_quant_wt", None) is None or \
                getattr(g.layer, "q_m_wt", None) is None:
            # the reference's compute_gamma_d raises on an empty qm_list
            raise ValueError(f"group {g.name}: its layer must be a QuantizeLinear with a weight quantizer")
        if not g.members:
            raise ValueError(f"group {g.name} has no members")
        for what, n in (("sections", g.sections), ("unit_rows", g.unit_rows)):
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
                raise ValueError(f"group {g.name}: {what} must be an integer >= 1 (got {n!r})")
        for p in g.members:
            if not isinstance(p, torch.Tensor) or p.dim() < 1 or p.dtype != torch.float32:
                raise ValueError(f"group {g.name}: a member must be a float32 tensor sliced along dim 0 "
                                 f"(got {getattr(p, 'dtype', type(p))})")
            if not p.is_contiguous():
                raise ValueError(f"group {g.name}: a member must be contiguous along its rows "
                                 f"(strides {tuple(p.stride())})")
            if id(p) in seen:
                raise ValueError(f"group {g.name}: a parameter appears in two groups")
            seen.add(id(p))
        if len({p.shape[0] for p in g.members}) != 1:
            raise ValueError(f"group {g.name}: members differ in shape[0]: {[tuple(p.shape) for p in g.members]}")
        per_unit = int(g.sections) * int(g.unit_rows)
        if g.members[0].shape[0] % per_unit or g.members[0].shape[0] == 0:
            raise ValueError(f"group {g.name}: shape[0] = {g.members[0].shape[0]} is not sections * units * unit_rows "
                             f"= {g.sections} * units * {g.unit_rows} for a whole number of units")


def vit_mlp_prune_groups(model: nn.Module) -> List[PruneGroup]:
    """One PruneGroup per Block: the MLP hidden units, i.e. the rows of fc1.weight and fc1.bias (a zeroed row gives
    GELU(0) = 0 and an activation code 0, so the matching column of fc2 is inert). For vit_model.py's models and
    anything with the same blocks[i].mlp.fc1 / fc2 layout."""
    groups = []
    for i, blk in enumerate(model.blocks):
        fc1 = blk.mlp.fc1
        members = [fc1.weight] + ([fc1.bias] if fc1.bias is not None else [])
        groups.append(PruneGroup(f"blocks.{i}.mlp", fc1, members))
    return groups


def vit_head_prune_groups(model: nn.Module) -> List[PruneGroup]:
    """One PruneGroup per Block: the attention heads, i.e. head h's q, k and v rows of attn.qkv.weight and attn.qkv.bias
    as the forward's reshape(B, N, 3, H, hd) reads them (sections = 3, unit_rows = head_dim). A zeroed head has
    q = k = v = 0 exactly, so its output columns are 0 and its activation codes into proj are 0: the matching columns
    of proj are inert (compress_pruned_heads removes both)."""
    groups = []
    for i, blk in enumerate(model.blocks):
        a = blk.attn
        members = [a.qkv.weight] + ([a.qkv.bias] if a.qkv.bias is not None else [])
        groups.append(PruneGroup(f"blocks.{i}.attn", a.qkv, members, sections=3, unit_rows=int(a.head_dim)))
    return groups


def active_num_redundant_groups(target: int, periods: int) -> List[int]:
    """Rows to take in each pruning period (geta.py:132-144)."""
    out, total = [], 0
    for p in range(periods):
        if p == periods - 1:
            out.append(target - total)
        else:
            out.append(target // periods)
            total += out[p]
    return out


def select_redundant(scores: torch.Tensor, taken: List[int], n: int) -> List[int]:
    """geta.py:172-177, the setdiff1d ordering included."""
    top = torch.topk(-scores, len(taken) + n)[1].cpu().numpy()
    return np.setdiff1d(top, taken)[:n].tolist()


def refine_by_divisible(g: PruneGroup, group_divisible: int) -> int:
    """geta.py:188-236 for one group whose `active` holds the fresh selection; returns the adjustment of
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


def _items(group, row, state, link) -> np.ndarray:
    """PruneItem entries from four columns (or scalars), as many as `row` has."""
    out = np.empty(len(row), dtype=_lib.PRUNE_ITEM_DTYPE)
    out["group"], out["row"], out["state"], out["link"] = group, row, state, link
    return out


def prune_tables(groups: List["_GroupState"], order: List[int], folded: bool, grow: np.ndarray) -> dict:
    """The item tables of the qvit_prune_* entry points from the groups' unit lists, as PruneItem arrays, and the
    fields rows, joint, red_begin and red_count (the range of the redundant rows) of the PruneGroup rows `grow`,
    written in place:
      items  every physical row of every group in `order`, a group's rows ascending, each with its unit's state and,
             where a unit is several rows, its unit;
      red    the rows of the active redundant units of the joint groups, a group's rows contiguous, unit after unit in
             unit_rows_of's order;
      units  (folded only) one entry per unit of every prunable group: link = the index in items of the group's row 0;
      joint  the indices of the joint groups, in `order`."""
    items, red, units, joint_groups = [], [], [], []
    nitems = nred = 0
    for gi in order:
        g = groups[gi]
        state = np.zeros(g.num_groups, dtype=np.int32)
        state[g.active] = _lib.PRUNE_REDUNDANT
        state[g.pruned] = _lib.PRUNE_PRUNED
        rows = np.arange(g.rows)
        unit = np.zeros(g.rows, dtype=np.int64) if g.basic else (rows // g.unit_rows) % g.num_groups
        items.append(_items(gi, rows, state if g.basic else state[unit], unit))
        if folded and g.prunable:
            units.append(_items(gi, np.arange(g.num_groups), state, nitems))
        nitems += g.rows
        joint = g.prunable and len(g.active) > 0
        act = unit_rows_of(g.active, g.num_groups, g.sections, g.unit_rows) if joint else ()
        G = grow[gi]
        G["rows"], G["joint"], G["red_begin"], G["red_count"] = g.rows, joint, nred if joint else 0, len(act)
        if joint:
            link = 0 if g.basic else np.repeat(np.asarray(g.active, dtype=np.int64), g.sections * g.unit_rows)
            red.append(_items(gi, act, _lib.PRUNE_REDUNDANT, link))
            nred += len(act)
            joint_groups.append(gi)
    empty = np.zeros(0, dtype=_lib.PRUNE_ITEM_DTYPE)
    return {"items": np.concatenate(items) if items else empty, "red": np.concatenate(red) if red else empty,
            "units": np.concatenate(units) if units else empty, "joint": joint_groups}


class _PruneState:
    """The pruning half of QuantAwareOptimizer: the host bookkeeping of geta.py:904-919, :1024-1026 and the device
    tables of the qvit_prune_* entry points. The host's lists (important, active, pruned, the global ranking) count
    units; the device's items are physical rows, each with its unit's state. Per step: qvit_prune_joint_apply for the
    members of every group, and while any group has active redundant rows qvit_prune_joint_scalars, _reduce and
    _finish in front of it; at a period boundary qvit_prune_scores and its finish, followed by the step's one host
    synchronisation."""

    def __init__(self, opt: "QuantAwareOptimizer", groups: List[PruneGroup], sparsity: float, start: int, steps: int,
                 periods: int, divisible: int, criteria):
        self.opt = opt
        self.groups = groups = [_GroupState(g) for g in groups]
        self.start, self.steps, self.divisible, self.sparsity = start, steps, divisible, sparsity
        self.periods = int(max(1, periods))
        self.period = steps // self.periods
        weights = dict(zip(_CRITERIA, [0.2] * 5)) if criteria == "default" else dict(criteria)
        if set(weights) - set(_CRITERIA):
            raise ValueError(f"importance_score_criteria: unknown {sorted(set(weights) - set(_CRITERIA))}")
        self.weights = tuple(float(weights.get(c, 0.0)) for c in _CRITERIA)
        dense_index = {id(p): i for i, (_, p) in enumerate(opt._dense)}
        triple_index = {(id(ps[0]), side): i for i, (_, side, ps) in enumerate(opt._triples)}
        self.member_dense: List[int] = []       # index in opt._dense of every member, in table order
        self.joint_triples: List[List[int]] = []  # per group: rows of opt._qrow of its layer's sides
        for g in groups:
            wq = g.layer.d_quant_wt
            if (id(wq), 0) not in triple_index or any(id(p) not in dense_index for p in g.members):
                raise ValueError(f"group {g.name}: its layer and members must belong to the optimizer's model")
            self.joint_triples.append([triple_index[(id(wq), 0)]] +
                                      ([triple_index[(id(g.layer.d_quant_act), 1)]]
                                       if getattr(g.layer, "d_quant_act", None) is not None else []))
        # prunable groups first, in the given order: their rows are the global indices 0 .. total_num_groups - 1
        self.total_num_groups = 0
        for g in groups:
            g.prunable = g.num_groups > divisible       # base_hybrid_sparse_optimizer.py:118-125
            if g.prunable:
                g.start = self.total_num_groups
                self.total_num_groups += g.num_groups
        self.target = int(self.total_num_groups * min(sparsity, 0.999))
        self.per_period = active_num_redundant_groups(self.target, self.periods)
        self.curr_period = 0
        self.taken: List[int] = []          # the reference's pruned_group_idxes (global)
        self.order = [i for i, g in enumerate(groups) if g.prunable] + \
                     [i for i, g in enumerate(groups) if not g.prunable]

        dev, ng = opt.device, len(groups)
        self.nmembers = sum(len(g.members) for g in groups)
        self._grow = np.zeros(ng, dtype=_lib.PRUNE_GROUP_DTYPE)
        self._mrow = np.zeros(self.nmembers, dtype=_lib.PRUNE_MEMBER_DTYPE)
        for gi, g in enumerate(groups):
            ly, G = g.layer, self._grow[gi]
            G["d"], G["qm"] = ly.d_quant_wt.data_ptr(), ly.q_m_wt.data_ptr()
            G["t"] = _lib._ptr(getattr(ly, "t_quant_wt", None)) or 0
            G["member_begin"], G["member_count"] = len(self.member_dense), len(g.members)
            if not g.basic:
                G["sections"], G["unit_rows"] = g.sections, g.unit_rows
            for p in g.members:
                di, M = dense_index[id(p)], self._mrow[len(self.member_dense)]
                M["p"], M["width"], M["quantized"] = p.data_ptr(), p.numel() // g.rows, p is ly.weight
                M["m"], M["v"] = _lib._ptr(opt._m[di]) or 0, _lib._ptr(opt._v[di]) or 0   # 0: no such moment
                G["elems"] += M["width"] * g.sections * g.unit_rows
                self.member_dense.append(di)
        self.nrows = sum(g.rows for g in groups)
        self.nprunable_rows = sum(g.rows for g in groups if g.prunable)
        # some unit is a set of rows: the scores go through qvit_prune_scores_fold and a table of the units
        self.folded = any(not g.basic for g in groups if g.prunable)
        self._gtable = opt._table(ng, _lib.PRUNE_GROUP_DTYPE)
        self._mtable = opt._table(self.nmembers, _lib.PRUNE_MEMBER_DTYPE)
        self._itable = opt._table(self.nrows, _lib.PRUNE_ITEM_DTYPE)    # every row, prunable groups first
        self._rtable = opt._table(self.nrows, _lib.PRUNE_ITEM_DTYPE)    # the active redundant rows
        self._jtable = opt._table(2 * ng, _lib.QAT_QUANT_DTYPE)
        self._sums = torch.zeros((max(self.nrows, 1), 3), dtype=torch.float64, device=dev)
        self._scores = torch.zeros(max(self.nrows, 1), dtype=torch.float32, device=dev)
        if self.folded:
            self._utable = opt._table(self.total_num_groups, _lib.PRUNE_ITEM_DTYPE)   # the prunable units
            self._unit_sums = torch.zeros((max(self.total_num_groups, 1), 3), dtype=torch.float64, device=dev)
        self._partials = torch.zeros((max(self.nrows, 1), 6), dtype=torch.float64, device=dev)
        self.gamma = torch.zeros(ng, dtype=torch.float32, device=dev)
        self.info = torch.full((ng,), -1, dtype=torch.int32, device=dev)
        self._nred = 0
        self._jrow = np.zeros(2 * ng, dtype=_lib.QAT_QUANT_DTYPE)
        self._qsend = np.zeros_like(opt._qrow)
        self._member_group = np.repeat(np.arange(ng), [len(g.members) for g in groups])
        self._tables()

    # ---- tables ---------------------------------------------------------------------------------------------------
    def _tables(self) -> None:
        """The group, item and joint quantizer rows from the host lists (rebuilt when the lists change)."""
        t = prune_tables(self.groups, self.order, self.folded, self._grow)
        self._items, self._nred = t["items"], int(t["red"].shape[0])
        self._red = np.zeros(max(self.nrows, 1), dtype=_lib.PRUNE_ITEM_DTYPE)
        self._red[:self._nred] = t["red"]
        if self.folded:
            self._units = t["units"]
        self._joint_rows: List[int] = [r for gi in t["joint"] for r in self.joint_triples[gi]]
        self._dirty = True   # the row lists go to the device when they change, not every step

    def quant_rows(self, qrow: np.ndarray) -> np.ndarray:
        """qvit_qat_quant_step's table with the joint layers' triples struck out: qvit_prune_joint_scalars has them."""
        if not self._joint_rows:
            return qrow
        self._qsend[...] = qrow
        self._qsend["s"][self._joint_rows, 0] = 0
        return self._qsend

    # ---- the step -------------------------------------------------------------------------------------------------
    def _boundary(self, n: int) -> bool:
        return (n >= self.start and self.curr_period < self.periods and self.period != 0
                and (n - self.start - 1) % self.period == 0)

    def commit(self) -> None:
        """commit_redundant_idxes (geta.py:238-248)."""
        for g in self.groups:
            if g.prunable:
                g.pruned.extend(g.active)
                g.active = []
                g.important = [i for i in range(g.num_groups) if i not in g.pruned]

    def begin_step(self, n: int, grad_ptrs: np.ndarray, fresh: np.ndarray, hyper: _lib.Hyper) -> None:
        self._mrow["grad"] = grad_ptrs[self.member_dense]
        self._mrow["flags"] = fresh[self.member_dense]   # bit 0: the tensor's first step
        if self._boundary(n):
            self._select(hyper)
        # before any launch of this step: the joint stage reads every member's gradient (compute_gamma_d would raise)
        for gi, g in enumerate(self.groups):
            if g.prunable and g.active and (self._mrow["grad"][self._member_group == gi] == 0).any():
                raise QvitError(f"group {g.name}: every member needs a gradient in the joint stage")

    def _select(self, hyper: _lib.Hyper) -> None:
        # geta.py:905-919: commit, the scores (this step's grad_variant, the parameters before the update), selection
        self.commit()
        self._tables()
        self._send()
        # (without the fold every prunable unit is one row: nprunable_rows == total_num_groups)
        fold = dict(units=self._utable.dev, nunits=self.total_num_groups, unit_sums=self._unit_sums) \
            if self.folded else {}
        _lib.prune_scores(self._gtable.dev, len(self.groups), self._mtable.dev, self.nmembers, self._itable.dev,
                          self.nprunable_rows, self._sums, self.weights, self._scores, hyper, **fold)
        chosen = select_redundant(self._scores[:self.total_num_groups], self.taken, self.per_period[self.curr_period])
        self.taken.extend(chosen)
        for g in self.groups:
            if g.prunable:
                ids = np.arange(g.start, g.start + g.num_groups)
                g.active = (np.intersect1d(chosen, ids) - g.start).tolist()
                self.target += refine_by_divisible(g, self.divisible)
        self.curr_period += 1
        self._tables()

    def _send(self) -> None:
        self._mtable.send(self._mrow)
        if self._dirty:
            self._gtable.send(self._grow)
            self._itable.send(self._items)
            self._rtable.send(self._red)
            if self.folded:
                self._utable.send(self._units)
            self._dirty = False

    def finish_step(self, n: int, hyper: _lib.Hyper) -> None:
        opt = self.opt
        ng = len(self.groups)
        t_in = (n - self.start) % self.period if self.period else 0
        self._send()
        if self._nred:
            nj = len(self._joint_rows)
            self._jrow[:nj] = opt._qrow[self._joint_rows]
            self._jrow[nj:] = 0
            self._jtable.send(self._jrow)
            _lib.prune_joint_scalars(self._jtable.dev, nj, hyper, opt.min_bit_act, opt.max_bit_act)
            _lib.prune_joint_reduce(self._gtable.dev, ng, self._mtable.dev, self.nmembers, self._rtable.dev,
                                    self._nred, self._partials, hyper)
            _lib.prune_joint_finish(self._gtable.dev, ng, self._partials, self._nred, hyper.lr,
                                    self.period, t_in, opt.min_bit_wt, opt.max_bit_wt, self.gamma, self.info)
        _lib.prune_joint_apply(self._gtable.dev, ng, self._mtable.dev, self.nmembers, self._itable.dev, self.nrows,
                               self.gamma, hyper)
        if self.period and n >= self.start and t_in == self.period - 1:   # geta.py:1024-1026
            self.commit()
            self._tables()

    # ---- state and metrics ----------------------------------------------------------------------------------------
    def state(self) -> dict:
        return {"group_names": [g.name for g in self.groups],
                "pruned_idxes": [list(g.pruned) for g in self.groups],
                "active_redundant_idxes": [list(g.active) for g in self.groups],
                "important_idxes": [list(g.important) for g in self.groups],
                "pruned_group_idxes": list(self.taken), "curr_pruning_period": self.curr_period,
                "target_num_redundant_groups": self.target}

    def load(self, st: dict) -> None:
        if st["group_names"] != [g.name for g in self.groups]:
            raise ValueError("the pruning state belongs to other groups")
        for g, pr, ac, im in zip(self.groups, st["pruned_idxes"], st["active_redundant_idxes"],
                                 st["important_idxes"]):
            g.pruned, g.active, g.important = list(pr), list(ac), list(im)
        self.taken = list(st["pruned_group_idxes"])
        self.curr_period = int(st["curr_pruning_period"])
        self.target = int(st["target_num_redundant_groups"])
        self._tables()

    @torch.no_grad()
    def metrics(self) -> Dict[str, float]:
        m = dict(norm_params=0.0, norm_important_groups=0.0, norm_redundant_groups=0.0, num_zero_groups=0,
                 num_important_groups=0, num_redundant_groups=0)
        for g in self.groups:
            if not g.prunable:
                continue
            sq = sum(units_view(p.detach(), g.num_groups, g.sections, g.unit_rows).double().pow(2).sum(dim=1)
                     for p in g.members)
            norm = sq.sqrt().cpu().numpy()
            red = g.active + g.pruned
            m["num_zero_groups"] += int(np.sum(norm == 0))
            m["norm_params"] += float(np.sum(norm))
            m["norm_important_groups"] += float(np.sum(norm[g.important]))
            m["norm_redundant_groups"] += float(np.sum(norm[red]))
            m["num_important_groups"] += len(g.important)
            m["num_redundant_groups"] += len(red)
        m["group_sparsity"] = m["num_zero_groups"] / float(self.total_num_groups + 1e-8)
        return m
