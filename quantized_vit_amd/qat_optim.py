"""QuantAwareOptimizer: the reference's GETA optimizer on the device.

OTO/optimizer/geta.py (GETA.step, :873-943) with the pruning stages absent unless row groups are declared, over
OTO/optimizer/base_optimizer.py's grad_variant (:40-86): warm-up, bit-range projection with the reduction schedule,
and the final "fix" stage. A step is
two HIP launches (include/qvit_hip.h: qvit_qat_step for every dense tensor, qvit_qat_quant_step for every quantizer
scalar and its projection) and no device-to-host copy: the reference makes a few torch launches per parameter and
reads q_m and t_quant back with .item() per layer, side and step. The pruning stages (saliency scores, redundant
groups, the joint stage, geta.py:904-1026) run for row groups the user declares (PruneGroup; vit_mlp_prune_groups for
the MLP hidden units of a ViT, vit_head_prune_groups for its attention heads): the reference's optimizer takes
ready-made parameter groups and only its graph tracer, which is out of scope, produces them. They are qat_prune.py;
compress.py removes what they zeroed from a model. The host tables of both are arrays of _lib's descriptor dtypes.

Reference behaviour kept as it is (the trained scalars are the product's input):
  * a tensor's first step makes its moment buffers grad and grad^2 themselves, not scaled by 1 - beta
    (base_optimizer.py:20-21, :31-32), so adam's first update is g / (1 - b1) / (sqrt(g^2 / (1 - b2)) + 1e-8);
  * in the range stage the activation-side scalars are stepped twice from one grad_variant, at lr by the weight pass
    (decayed at lr too under adamw) and again at lr_quant by the activation pass (geta.py:598-630, then :667-697);
  * the reference finds a layer's scalars by the substring test `layer_name in p_name`; here a layer's scalars are
    those of that module object, which is what the test means without its accident ("blocks.1" also matching
    "blocks.10...").
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import QvitError
from .qat_prune import PruneGroup, _check_prune_groups, _PruneState
from .quant_layers import QuantizeMixin

_VARIANTS = {"sgd": _lib.QAT_SGD, "adam": _lib.QAT_ADAM, "adamw": _lib.QAT_ADAMW}
_SCALARS = ("d_quant", "q_m", "t_quant")
_SIDES = ("wt", "act")
HARD_MIN_MAX_BIT = 6   # geta.py:895-900: the schedule never lowers max_bit below 6


def bit_schedule_step(num_steps: int, start_projection_step: int, fix_after_step: int, period: int,
                      bit_reduction: int, min_bit: int, max_bit: int) -> int:
    """max_bit after the schedule's look at step `num_steps` (geta.py:885-900, with fix_after_step where the
    reference has start_pruning_step: with no pruning steps the two coincide)."""
    s = num_steps - start_projection_step - 1
    if start_projection_step <= num_steps <= fix_after_step and start_projection_step != fix_after_step \
            and period > 0 and s % period == 0 and s != 0:
        return max(min_bit, HARD_MIN_MAX_BIT, max_bit - bit_reduction)
    return max_bit


class _Upload:
    """A device table fed from two pinned staging buffers in turn: a buffer is rewritten only after the upload
    that last read it has finished (its event), so an upload in flight never sees a half-written table. `send` takes
    an array of `dtype` (one of _lib's descriptors, whole int64 words) and uploads its bytes as they are."""

    def __init__(self, rows: int, dtype: np.dtype, device: torch.device):
        shape = (max(rows, 1), dtype.itemsize // 8)
        self.dev = torch.zeros(shape, dtype=torch.int64, device=device)
        self.host = [torch.zeros(shape, dtype=torch.int64).pin_memory() for _ in range(2)]
        self.words = [h.numpy().reshape(-1) for h in self.host]   # the staging buffers as the tables' int64 view
        self.events: List[Optional[torch.cuda.Event]] = [None, None]
        self.turn = 0
        self.last: Optional[np.ndarray] = None

    def send(self, table: np.ndarray) -> None:
        words = table.view(np.int64)
        if self.last is not None and np.array_equal(self.last, words):
            return
        i = self.turn
        self.turn ^= 1
        if self.events[i] is not None and not self.events[i].query():
            self.events[i].synchronize()   # two uploads behind: practically never taken
        self.words[i][...] = words
        self.dev.copy_(self.host[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev.device))
        self.events[i] = ev
        self.last = words.copy()


class QuantAwareOptimizer(torch.optim.Optimizer):
    """GETA's quantization-aware training stages for a model built from this package's layers; see the module
    docstring for the stages, the kept quirks and what is out of scope.

    Steps <= start_projection_step are warm-up (every parameter stepped, the quantizer scalars at lr_quant). Then the
    range stage: after the update d_quant of every layer and side is clamped into [d(max_bit), d(min_bit)], d(b) =
    |q_m|^t / (2^(b-1) - 1), and at each boundary of a period of projection_steps // projection_periods steps
    max_bit_* = max(min_bit_*, 6, max_bit_* - bit_reduction). Steps > fix_after_step (the reference's
    start_pruning_step + pruning_steps) are the fix stage: the first of them rounds every layer's bit width to an
    integer, kept on the device, and d_quant = d(that width) from then on.

    A parameter whose grad is None is skipped and its moments stay untouched. `grad_clip=(lo, hi)` clamps every
    gradient as it is loaded (the reference's grad_clipping). After every step `invalidate()` is called on every
    module of the model that has one: the kernels write through raw pointers, which does not move the version
    counter the packed-weight plans key on. All parameters must be contiguous float32 ROCm tensors (QvitError)."""

    def __init__(self, model: nn.Module, variant: str = "sgd", lr: float = 1e-3, lr_quant: float = 1e-3,
                 first_momentum: Optional[float] = None, second_momentum: Optional[float] = None,
                 dampening: Optional[float] = None, weight_decay: Optional[float] = None,
                 start_projection_step: int = 0, projection_steps: int = 1, projection_periods: int = 1,
                 fix_after_step: Optional[int] = None, bit_reduction: int = 2, min_bit_wt: int = 4,
                 max_bit_wt: int = 16, min_bit_act: int = 4, max_bit_act: int = 16,
                 grad_clip: Optional[Tuple[float, float]] = None, prune_groups: Optional[List[PruneGroup]] = None,
                 target_group_sparsity: float = 0.5, start_pruning_step: int = 1, pruning_steps: int = 1,
                 pruning_periods: int = 1, group_divisible: int = 1, importance_score_criteria="default"):
        if variant not in _VARIANTS:
            raise ValueError(f"variant = {variant!r}: expected one of {sorted(_VARIANTS)}")
        for name, lo, hi in (("wt", min_bit_wt, max_bit_wt), ("act", min_bit_act, max_bit_act)):
            if not 2 <= lo <= hi <= 32:
                raise ValueError(f"bit range of {name}: need 2 <= min_bit <= max_bit <= 32 (got {lo}, {hi})")
        adam = variant != "sgd"
        if adam and (first_momentum is None or second_momentum is None):
            raise ValueError(f"{variant} needs first_momentum and second_momentum")
        if prune_groups is not None:
            prune_groups = list(prune_groups)
            _check_prune_groups(prune_groups)
        self.model = model
        self.variant = variant
        self.start_projection_step = int(start_projection_step)
        self.projection_steps = int(projection_steps)
        self.projection_periods = int(projection_periods)
        self.projection_period_duration = self.projection_steps // max(self.projection_periods, 1)
        if prune_groups is not None:
            # the fix stage begins after the pruning steps (geta.py:931)
            if fix_after_step is not None and int(fix_after_step) != int(start_pruning_step) + int(pruning_steps):
                raise ValueError(f"fix_after_step = {fix_after_step} disagrees with start_pruning_step + pruning_steps "
                                 f"= {int(start_pruning_step) + int(pruning_steps)}")
            fix_after_step = int(start_pruning_step) + int(pruning_steps)
        self.fix_after_step = 2 if fix_after_step is None else int(fix_after_step)
        # the bit schedule runs while num_steps <= start_pruning_step (geta.py:885-902)
        self._schedule_end = self.fix_after_step if prune_groups is None else int(start_pruning_step)
        self.bit_reduction = int(bit_reduction)
        self.min_bit_wt, self.max_bit_wt = int(min_bit_wt), int(max_bit_wt)
        self.min_bit_act, self.max_bit_act = int(min_bit_act), int(max_bit_act)
        self.grad_clip = None if grad_clip is None else (float(grad_clip[0]), float(grad_clip[1]))
        self.num_steps = 0
        self.fixed = False   # the fix stage has taken its bit widths

        named = list(model.named_parameters())
        if not named:
            raise ValueError("the model has no parameters")
        for name, p in named:
            if not p.is_cuda:
                raise QvitError(f"parameter {name} is on {p.device}: the optimizer step runs on a ROCm device only")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise QvitError(f"parameter {name}: the optimizer step takes contiguous float32 parameters "
                                f"(got {p.dtype}, strides {tuple(p.stride())})")
        self.device = named[0][1].device
        if any(p.device != self.device for _, p in named):
            raise QvitError("the optimizer step takes parameters of one device")
        name_of = {id(p): n for n, p in named}

        # the (layer, side) triples: the scalars of that module object
        self._triples: List[Tuple[str, int, List[Optional[nn.Parameter]]]] = []
        scalar_ids = set()
        for lname, mod in model.named_modules():
            if not isinstance(mod, QuantizeMixin):
                continue
            for side, tag in enumerate(_SIDES):
                ps = [getattr(mod, f"{s}_{tag}", None) for s in _SCALARS]
                if ps[0] is None or ps[1] is None:
                    continue
                if any(p is not None and (id(p) not in name_of or p.numel() != 1) for p in ps):
                    raise QvitError(f"{lname}: quantizer scalars must be registered parameters of one element")
                self._triples.append((lname, side, ps))
                scalar_ids.update(id(p) for p in ps if p is not None)
        self._dense: List[Tuple[str, nn.Parameter]] = [(n, p) for n, p in named if id(p) not in scalar_ids]
        self._invalidate = [m.invalidate for m in model.modules() if callable(getattr(m, "invalidate", None))]

        defaults = dict(lr=float(lr), lr_quant=float(lr_quant), first_momentum=first_momentum,
                        second_momentum=second_momentum, dampening=dampening, weight_decay=weight_decay)
        super().__init__([p for _, p in named], defaults)

        # moments: one buffer per dense tensor and kind, six floats per triple
        mom1 = (first_momentum or 0.0) > 0.0
        mom2 = adam and (second_momentum or 0.0) > 0.0
        self._m = [torch.zeros_like(p, memory_format=torch.contiguous_format) if mom1 else None
                   for _, p in self._dense]
        self._v = [torch.zeros_like(p, memory_format=torch.contiguous_format) if mom2 else None
                   for _, p in self._dense]
        nq = len(self._triples)
        self._qmom = torch.zeros((max(nq, 1), 6), dtype=torch.float32, device=self.device)
        self._bits = torch.zeros(max(nq, 1), dtype=torch.int32, device=self.device)
        self._seen = np.zeros(len(self._dense), dtype=bool)          # the tensor has had its first step
        self._qseen = np.zeros((max(nq, 1), 3), dtype=bool)

        # the constant fields of the two tables
        nd = len(self._dense)
        self._trow = np.zeros(max(nd, 1), dtype=_lib.QAT_TENSOR_DTYPE)
        for i, (_, p) in enumerate(self._dense):
            T = self._trow[i]
            T["p"], T["numel"] = p.data_ptr(), p.numel()
            T["m"], T["v"] = _lib._ptr(self._m[i]) or 0, _lib._ptr(self._v[i]) or 0   # 0: no such moment
        self._qrow = np.zeros(max(nq, 1), dtype=_lib.QAT_QUANT_DTYPE)
        for i, (_, side, ps) in enumerate(self._triples):
            Q = self._qrow[i]
            Q["s"] = [_lib._ptr(p) or 0 for p in ps]
            Q["mom"], Q["side"] = self._qmom.data_ptr() + 24 * i, side
        self._ttable = self._table(nd, _lib.QAT_TENSOR_DTYPE)
        self._qtable = self._table(nq, _lib.QAT_QUANT_DTYPE)
        self._prune: Optional[_PruneState] = None if prune_groups is None else \
            _PruneState(self, prune_groups, float(target_group_sparsity), int(start_pruning_step), int(pruning_steps),
                        int(pruning_periods), int(group_divisible), importance_score_criteria)
        # the chunk list (uploaded once), without the prune groups' members: qvit_prune_joint_apply steps those
        members = set() if self._prune is None else set(self._prune.member_dense)
        pairs = [(i, c) for i, (_, p) in enumerate(self._dense) if i not in members
                 for c in range(-(-p.numel() // _lib.QAT_CHUNK))]
        self._nchunks = len(pairs)
        chunks = np.array(pairs or [(0, 0)], dtype=_lib.QAT_CHUNK_DTYPE)
        self._chunks = torch.from_numpy(chunks.view(np.int32).reshape(-1, 2)).to(self.device)

    def _table(self, rows: int, dtype: np.dtype) -> _Upload:
        """A device table of `rows` descriptors (_PruneState makes its own through this: qat_prune.py cannot import
        _Upload from here, this module imports it)."""
        return _Upload(rows, dtype, self.device)

    # ---- the reference's small surface --------------------------------------------------------------------------
    def set_learning_rate(self, lr: float) -> None:
        for g in self.param_groups:
            g["lr"] = lr

    def get_learning_rate(self) -> float:
        return self.param_groups[-1]["lr"]

    def stage(self, num_steps: Optional[int] = None) -> int:
        """The stage of step `num_steps` (default: the next one), as GETA.step branches (geta.py:926-943)."""
        n = self.num_steps + 1 if num_steps is None else num_steps
        if n <= self.start_projection_step:
            return _lib.QAT_WARMUP
        return _lib.QAT_FIX if n > self.fix_after_step else _lib.QAT_RANGE

    def _scalars_host(self) -> np.ndarray:
        """[ntriples, 3] of (d, q_m, t) with t = 1 where a layer has none: one device-to-host copy."""
        one = torch.ones(1, device=self.device)
        flat = [(p.detach().reshape(1) if p is not None else one) for _, _, ps in self._triples for p in ps]
        return torch.cat(flat).reshape(-1, 3).cpu().numpy().astype(np.float64)

    def bit_widths(self) -> Dict[str, Dict[str, float]]:
        """{layer: {"weight": bits, "activation": bits}} from the current scalars, un-rounded, as
        quant_model.get_bitwidth_dict gives them. The one call here that copies from the device to the host."""
        out: Dict[str, Dict[str, float]] = {}
        if not self._triples:
            return out
        vals = self._scalars_host()
        for (lname, side, _), (d, qm, t) in zip(self._triples, vals):
            b = math.log2(math.exp(t * math.log(abs(qm))) / abs(d) + 1) + 1
            out.setdefault(lname, {})["activation" if side else "weight"] = b
        return out

    def fixed_bits(self) -> Dict[str, Dict[str, int]]:
        """The integer bit widths the fix stage took ({} before its first step); copies from the device."""
        out: Dict[str, Dict[str, int]] = {}
        if not self.fixed:
            return out
        bits = self._bits.cpu().tolist()
        for (lname, side, _), b in zip(self._triples, bits):
            out.setdefault(lname, {})["activation" if side else "weight"] = int(b)
        return out

    # ---- the step -----------------------------------------------------------------------------------------------
    def _grad_ptr(self, name: str, p: torch.Tensor) -> int:
        g = p.grad
        if g is None:
            return 0
        if not g.is_cuda or g.device != p.device or g.dtype != torch.float32 or not g.is_contiguous() \
                or g.numel() != p.numel():
            raise QvitError(f"gradient of {name}: expected a contiguous float32 tensor on {p.device} of "
                            f"{p.numel()} elements (got {g.dtype} on {g.device}, strides {tuple(g.stride())})")
        return g.data_ptr()

    def _hyper(self, first_step: bool) -> _lib.Hyper:
        g = self.param_groups[0]
        adam = self.variant != "sgd"
        b1 = float(g["first_momentum"] or 0.0)
        b2 = float(g["second_momentum"] or 0.0) if adam else 0.0
        damp = float(g["dampening"] or 0.0)
        # the reference's Python doubles, rounded to fp32 where torch rounds them: at the call
        a1 = 1.0 - (b1 if adam else damp)
        a2 = 1.0 - b2
        bc1 = 1.0 - b1 ** self.num_steps if adam else 1.0
        bc2 = 1.0 - b2 ** self.num_steps if adam else 1.0
        wd = float(g["weight_decay"] or 0.0)
        lo, hi = self.grad_clip if self.grad_clip is not None else (-math.inf, math.inf)
        return _lib.Hyper(_VARIANTS[self.variant], int(first_step), float(g["lr"]), float(g["lr_quant"]), b1, b2, a1,
                          a2, wd, bc1, bc2, lo, hi)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.num_steps += 1
        n = self.num_steps
        stage = self.stage(n)
        # the bit-range schedule (geta.py:885-900)
        per = self.projection_period_duration
        self.max_bit_wt = bit_schedule_step(n, self.start_projection_step, self._schedule_end, per,
                                            self.bit_reduction, self.min_bit_wt, self.max_bit_wt)
        self.max_bit_act = bit_schedule_step(n, self.start_projection_step, self._schedule_end, per,
                                             self.bit_reduction, self.min_bit_act, self.max_bit_act)
        hyper = self._hyper(first_step=False)
        pr = self._prune

        if self._dense:
            ptrs = np.fromiter((self._grad_ptr(nm, p) for nm, p in self._dense), dtype=np.int64,
                               count=len(self._dense))
            live = ptrs != 0
            if pr is not None:
                pr.begin_step(n, ptrs, live & ~self._seen, hyper)   # the period boundary: scores and selection
            self._trow["grad"] = ptrs
            self._trow["flags"] = live & ~self._seen   # bit 0: the tensor's first step
            self._ttable.send(self._trow)
            _lib.qat_step(self._ttable.dev, len(self._dense), self._chunks, self._nchunks, hyper)
            self._seen |= live
        if self._triples:
            nq = len(self._triples)
            ptrs = np.fromiter((0 if p is None else self._grad_ptr(ln, p) for ln, _, ps in self._triples for p in ps),
                               dtype=np.int64, count=3 * nq).reshape(nq, 3)
            live = ptrs != 0
            fresh = live & ~self._qseen[:nq]
            self._qrow["g"][:nq] = ptrs
            self._qrow["flags"][:nq] = (fresh * np.array([1, 2, 4])).sum(axis=1)
            self._qtable.send(self._qrow if pr is None else pr.quant_rows(self._qrow))
            first_fix = stage == _lib.QAT_FIX and not self.fixed
            _lib.qat_quant_step(self._qtable.dev, nq, self._bits, stage, first_fix, hyper,
                                (self.min_bit_wt, self.max_bit_wt, self.min_bit_act, self.max_bit_act))
            self._qseen[:nq] |= live
        if pr is not None:
            pr.finish_step(n, hyper)
        if stage == _lib.QAT_FIX:
            self.fixed = True
        for inv in self._invalidate:
            inv()
        return loss

    # ---- state ---------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Step count, current max bits, moments, first-step marks and the fixed bit widths (cloned tensors), plus
        the param group's hyper-parameters: load_state_dict on an optimizer built over the same model continues
        bit for bit."""
        return {
            "num_steps": self.num_steps, "max_bit_wt": self.max_bit_wt, "max_bit_act": self.max_bit_act,
            "fixed": self.fixed, "variant": self.variant,
            "param_names": [n for n, _ in self._dense],
            "layer_sides": [(ln, side) for ln, side, _ in self._triples],
            "first_moments": [None if m is None else m.detach().clone() for m in self._m],
            "second_moments": [None if v is None else v.detach().clone() for v in self._v],
            "quant_moments": self._qmom.detach().clone(), "fixed_bits": self._bits.detach().clone(),
            "seen": self._seen.copy(), "quant_seen": self._qseen.copy(),
            "hyper": {k: v for k, v in self.param_groups[0].items() if k != "params"},
            **({} if self._prune is None else {"pruning": self._prune.state()}),
        }

    @torch.no_grad()
    def load_state_dict(self, state: dict) -> None:
        if state["variant"] != self.variant or state["param_names"] != [n for n, _ in self._dense] or \
                [tuple(x) for x in state["layer_sides"]] != [(ln, side) for ln, side, _ in self._triples]:
            raise ValueError("the state belongs to another variant or another model")
        for mine, theirs in ((self._m, state["first_moments"]), (self._v, state["second_moments"])):
            for a, b in zip(mine, theirs):
                if (a is None) != (b is None):
                    raise ValueError("the state keeps other moments than this optimizer")
                if a is not None:
                    a.copy_(b)
        self._qmom.copy_(state["quant_moments"])
        self._bits.copy_(state["fixed_bits"])
        self._seen[...] = state["seen"]
        self._qseen[...] = state["quant_seen"]
        self.num_steps = int(state["num_steps"])
        self.max_bit_wt, self.max_bit_act = int(state["max_bit_wt"]), int(state["max_bit_act"])
        self.fixed = bool(state["fixed"])
        self.param_groups[0].update(state["hyper"])
        if self._prune is not None:
            if "pruning" not in state:
                raise ValueError("the state carries no pruning state")
            self._prune.load(state["pruning"])

    # ---- pruning ------------------------------------------------------------------------------------------------
    def _need_prune(self) -> _PruneState:
        if self._prune is None:
            raise ValueError("the optimizer was built without prune_groups")
        return self._prune

    def pruned_rows(self) -> Dict[str, List[int]]:
        """{group name: sorted units committed as pruned}: rows of a one-row geometry, heads of a head group."""
        return {g.name: sorted(g.pruned) for g in self._need_prune().groups}

    def prune_metrics(self) -> Dict[str, float]:
        """The fields of the reference's compute_metrics (geta.py:1028-1071). Copies from the device."""
        return self._need_prune().metrics()
