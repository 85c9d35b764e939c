"""QuantAwareOptimizer: the reference's GETA optimizer on the device.

OTO/optimizer/geta.py (GETA.step, :873-943) with the pruning stages absent unless row groups are declared, over
OTO/optimizer/base_optimizer.py's grad_variant (:40-86): warm-up, bit-range projection with the reduction schedule,
and the final "fix" stage. A step is
two HIP launches (include/qvit_hip.h: qvit_qat_step for every dense tensor, qvit_qat_quant_step for every quantizer
scalar and its projection) and no device-to-host copy: the reference makes a few torch launches per parameter and
reads q_m and t_quant back with .item() per layer, side and step. The pruning stages (saliency scores, redundant
groups, the joint stage, geta.py:904-1026) run for row groups the user declares (PruneGroup; vit_mlp_prune_groups for
the MLP hidden units of a ViT, vit_head_prune_groups for its attention heads): the reference's optimizer takes ready-made parameter groups and only its graph tracer,
which is out of scope, produces them. See the second half of this module.

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
    that last read it has finished (its event), so an upload in flight never sees a half-written table."""

    def __init__(self, rows: int, cols: int, device: torch.device):
        self.dev = torch.zeros((max(rows, 1), cols), dtype=torch.int64, device=device)
        self.host = [torch.zeros((max(rows, 1), cols), dtype=torch.int64).pin_memory() for _ in range(2)]
        self.events: List[Optional[torch.cuda.Event]] = [None, None]
        self.turn = 0
        self.last: Optional[np.ndarray] = None

    def send(self, table: np.ndarray) -> None:
        if self.last is not None and np.array_equal(self.last, table):
            return
        i = self.turn
        self.turn ^= 1
        if self.events[i] is not None and not self.events[i].query():
            self.events[i].synchronize()   # two uploads behind: practically never taken
        self.host[i].numpy()[...] = table
        self.dev.copy_(self.host[i], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev.device))
        self.events[i] = ev
        self.last = table.copy()


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
                 grad_clip: Optional[Tuple[float, float]] = None, prune_groups: Optional[List["PruneGroup"]] = None,
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

        # constant columns of the two tables, and the chunk list (uploaded once)
        nd = len(self._dense)
        self._trow = np.zeros((max(nd, 1), _lib.QAT_TENSOR_BYTES // 8), dtype=np.int64)
        chunk_t, chunk_i = [], []
        for i, (_, p) in enumerate(self._dense):
            self._trow[i, 0] = p.data_ptr()
            self._trow[i, 2] = 0 if self._m[i] is None else self._m[i].data_ptr()
            self._trow[i, 3] = 0 if self._v[i] is None else self._v[i].data_ptr()
            self._trow[i, 4] = p.numel()
            n = -(-p.numel() // _lib.QAT_CHUNK)
            chunk_t.append(np.full(n, i, dtype=np.int32))
            chunk_i.append(np.arange(n, dtype=np.int32))
        chunks = np.stack([np.concatenate(chunk_t), np.concatenate(chunk_i)], axis=1) if nd else \
            np.zeros((0, 2), dtype=np.int32)
        self._nchunks = int(chunks.shape[0])
        self._chunks = torch.from_numpy(np.ascontiguousarray(chunks if self._nchunks else
                                                             np.zeros((1, 2), np.int32))).to(self.device)
        self._qrow = np.zeros((max(nq, 1), _lib.QAT_QUANT_BYTES // 8), dtype=np.int64)
        for i, (_, side, ps) in enumerate(self._triples):
            for s, p in enumerate(ps):
                self._qrow[i, s] = 0 if p is None else p.data_ptr()
            self._qrow[i, 6] = self._qmom.data_ptr() + 24 * i
            self._qrow[i, 7] = side
        self._ttable = _Upload(nd, self._trow.shape[1], self.device)
        self._qtable = _Upload(nq, self._qrow.shape[1], self.device)
        self._prune: Optional[_PruneState] = None
        if prune_groups is not None:
            self._prune = _PruneState(self, prune_groups, float(target_group_sparsity), int(start_pruning_step),
                                      int(pruning_steps), int(pruning_periods), int(group_divisible),
                                      importance_score_criteria)
            # the members leave the dense launch: qvit_prune_joint_apply steps them in every stage
            keep = ~np.isin(chunks[:, 0], list(self._prune.member_dense)) if self._nchunks else np.zeros(0, bool)
            chunks = chunks[keep]
            self._nchunks = int(chunks.shape[0])
            self._chunks = torch.from_numpy(np.ascontiguousarray(chunks if self._nchunks else
                                                                 np.zeros((1, 2), np.int32))).to(self.device)

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

    def _hyper(self, first_step: bool) -> tuple:
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
        return (_VARIANTS[self.variant], int(first_step), float(g["lr"]), float(g["lr_quant"]), b1, b2, a1, a2, wd,
                bc1, bc2, lo, hi)

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
            self._trow[:, 1] = ptrs
            self._trow[:, 5] = (live & ~self._seen).astype(np.int64) << 32   # flags bit 0, lr class 0
            self._ttable.send(self._trow)
            _lib.qat_step(self._ttable.dev, len(self._dense), self._chunks, self._nchunks, hyper)
            self._seen |= live
        if self._triples:
            nq = len(self._triples)
            ptrs = np.fromiter((0 if p is None else self._grad_ptr(ln, p) for ln, _, ps in self._triples for p in ps),
                               dtype=np.int64, count=3 * nq).reshape(nq, 3)
            live = ptrs != 0
            fresh = live & ~self._qseen[:nq]
            self._qrow[:nq, 3:6] = ptrs
            flags = (fresh * np.array([1, 2, 4])).sum(axis=1).astype(np.int64)
            self._qrow[:nq, 7] = (self._qrow[:nq, 7] & 0xffffffff) | (flags << 32)
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
    def _need_prune(self) -> "_PruneState":
        if self._prune is None:
            raise ValueError("the optimizer was built without prune_groups")
        return self._prune

    def pruned_rows(self) -> Dict[str, List[int]]:
        """{group name: sorted units committed as pruned}: rows of a one-row geometry, heads of a head group."""
        return {g.name: sorted(g.pruned) for g in self._need_prune().groups}

    def prune_metrics(self) -> Dict[str, float]:
        """The fields of the reference's compute_metrics (geta.py:1028-1071). Copies from the device."""
        return self._need_prune().metrics()


# ---- the pruning stages for declared row groups --------------------------------------------------------------------
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
    from .quant_layers import QuantizeLinear
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


def prune_tables(groups: List["_GroupState"], order: List[int], folded: bool, grow: np.ndarray) -> dict:
    """The item tables of the qvit_prune_* entry points from the groups' unit lists, as int64 pairs per 16-byte
    entry (group | row << 32, state | link << 32), and columns 4 and 5 of the group rows `grow` (rows and joint, the
    range of the redundant rows), written in place:
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
        state = np.zeros(g.num_groups, dtype=np.int64)
        state[g.active] = _lib.PRUNE_REDUNDANT
        state[g.pruned] = _lib.PRUNE_PRUNED
        rows = np.arange(g.rows, dtype=np.int64)
        unit = np.zeros(g.rows, dtype=np.int64) if g.basic else (rows // g.unit_rows) % g.num_groups
        items.append(np.stack([gi | (rows << 32), (state if g.basic else state[unit]) | (unit << 32)], axis=1))
        if folded and g.prunable:
            units.append(np.stack([gi | (np.arange(g.num_groups, dtype=np.int64) << 32), state | (nitems << 32)],
                                  axis=1))
        nitems += g.rows
        joint = g.prunable and len(g.active) > 0
        grow[gi, 4] = g.rows | (int(joint) << 32)
        grow[gi, 5] = 0
        if joint:
            act = unit_rows_of(g.active, g.num_groups, g.sections, g.unit_rows)
            link = np.zeros(len(act), np.int64) if g.basic else \
                np.repeat(np.asarray(g.active, dtype=np.int64), g.sections * g.unit_rows)
            grow[gi, 5] = nred | (len(act) << 32)
            red.append(np.stack([gi | (act << 32), _lib.PRUNE_REDUNDANT | (link << 32)], axis=1))
            nred += len(act)
            joint_groups.append(gi)
    empty = np.zeros((0, 2), np.int64)
    return {"items": np.concatenate(items) if items else empty, "red": np.concatenate(red) if red else empty,
            "units": np.concatenate(units) if units else empty, "joint": joint_groups}


class _PruneState:
    """The pruning half of QuantAwareOptimizer: the host bookkeeping of geta.py:904-919, :1024-1026 and the device
    tables of the qvit_prune_* entry points. The host's lists (important, active, pruned, the global ranking) count
    units; the device's items are physical rows, each with its unit's state. Per step: qvit_prune_joint_apply for the members of every group, and
    while any group has active redundant rows qvit_prune_joint_scalars, _reduce and _finish in front of it; at a
    period boundary qvit_prune_scores and its finish, followed by the step's one host synchronisation."""

    def __init__(self, opt: "QuantAwareOptimizer", groups: List[PruneGroup], sparsity: float, start: int, steps: int,
                 periods: int, divisible: int, criteria):
        self.opt = opt
        self.groups = groups = [_GroupState(g) for g in groups]
        self.start, self.steps = start, steps
        self.periods = int(max(1, periods))
        self.period = steps // self.periods
        self.divisible = divisible
        self.sparsity = sparsity
        weights = dict(zip(_CRITERIA, [0.2] * 5)) if criteria == "default" else dict(criteria)
        if set(weights) - set(_CRITERIA):
            raise ValueError(f"importance_score_criteria: unknown {sorted(set(weights) - set(_CRITERIA))}")
        self.weights = tuple(float(weights.get(c, 0.0)) for c in _CRITERIA)
        dense_index = {id(p): i for i, (_, p) in enumerate(opt._dense)}
        triple_index = {(id(ps[0]), side): i for i, (_, side, ps) in enumerate(opt._triples)}
        self.member_dense: List[int] = []       # index in opt._dense of every member, in table order
        self.member_group: List[int] = []
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

        dev = opt.device
        ng = len(groups)
        self._grow = np.zeros((ng, _lib.PRUNE_GROUP_BYTES // 8), dtype=np.int64)
        mrows = []
        for gi, g in enumerate(groups):
            ly = g.layer
            t = getattr(ly, "t_quant_wt", None)
            self._grow[gi, 0:3] = (ly.d_quant_wt.data_ptr(), ly.q_m_wt.data_ptr(), 0 if t is None else t.data_ptr())
            self._grow[gi, 3] = len(mrows) | (len(g.members) << 32)
            elems = 0
            for p in g.members:
                di = dense_index[id(p)]
                width = p.numel() // g.rows
                elems += width * g.sections * g.unit_rows
                mrows.append([p.data_ptr(), 0, 0 if opt._m[di] is None else opt._m[di].data_ptr(),
                              0 if opt._v[di] is None else opt._v[di].data_ptr(), width,
                              1 if p is ly.weight else 0])
                self.member_dense.append(di)
                self.member_group.append(gi)
            self._grow[gi, 6] = elems
            self._grow[gi, 7] = 0 if g.basic else (g.sections | (g.unit_rows << 32))
        self._mrow = np.array(mrows, dtype=np.int64)
        self.nmembers = len(mrows)
        self.nrows = sum(g.rows for g in groups)
        self.nprunable_rows = sum(g.rows for g in groups if g.prunable)
        # some unit is a set of rows: the scores go through qvit_prune_scores_fold and a table of the units
        self.folded = any(not g.basic for g in groups if g.prunable)
        self._gtable = _Upload(ng, self._grow.shape[1], dev)
        self._mtable = _Upload(self.nmembers, self._mrow.shape[1], dev)
        self._itable = _Upload(self.nrows, _lib.PRUNE_ITEM_BYTES // 8, dev)    # every row, prunable groups first
        self._rtable = _Upload(self.nrows, _lib.PRUNE_ITEM_BYTES // 8, dev)    # the active redundant rows
        self._jtable = _Upload(2 * ng, opt._qrow.shape[1], dev)
        self._sums = torch.zeros((max(self.nrows, 1), 3), dtype=torch.float64, device=dev)
        self._scores = torch.zeros(max(self.nrows, 1), dtype=torch.float32, device=dev)
        if self.folded:
            self._utable = _Upload(self.total_num_groups, _lib.PRUNE_ITEM_BYTES // 8, dev)   # the prunable units
            self._unit_sums = torch.zeros((max(self.total_num_groups, 1), 3), dtype=torch.float64, device=dev)
        self._partials = torch.zeros((max(self.nrows, 1), 6), dtype=torch.float64, device=dev)
        self.gamma = torch.zeros(ng, dtype=torch.float32, device=dev)
        self.info = torch.full((ng,), -1, dtype=torch.int32, device=dev)
        self._nred = 0
        self._jrow = np.zeros((2 * ng, opt._qrow.shape[1]), dtype=np.int64)
        self._qsend = np.zeros_like(opt._qrow)
        self._member_group = np.asarray(self.member_group)
        self._tables()

    # ---- tables ---------------------------------------------------------------------------------------------------
    def _tables(self) -> None:
        """The group, item and joint quantizer rows from the host lists (rebuilt when the lists change)."""
        t = prune_tables(self.groups, self.order, self.folded, self._grow)
        self._items, self._nred = t["items"], int(t["red"].shape[0])
        self._red = np.zeros((max(self.nrows, 1), 2), dtype=np.int64)
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
        self._qsend[self._joint_rows, 0] = 0
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

    def begin_step(self, n: int, grad_ptrs: np.ndarray, fresh: np.ndarray, hyper: tuple) -> None:
        self._mrow[:, 1] = grad_ptrs[self.member_dense]
        self._mrow[:, 5] = (self._mrow[:, 5] & 0xffffffff) | (fresh[self.member_dense].astype(np.int64) << 32)
        if self._boundary(n):
            self._select(hyper)
        # before any launch of this step: the joint stage reads every member's gradient (compute_gamma_d would raise)
        for gi, g in enumerate(self.groups):
            if g.prunable and g.active and (self._mrow[self._member_group == gi, 1] == 0).any():
                raise QvitError(f"group {g.name}: every member needs a gradient in the joint stage")

    def _select(self, hyper: tuple) -> None:
        # geta.py:905-919: commit, the scores (this step's grad_variant, the parameters before the update), selection
        self.commit()
        self._tables()
        self._send()
        ng = len(self.groups)
        if self.folded:
            _lib.prune_scores(self._gtable.dev, ng, self._mtable.dev, self.nmembers, self._itable.dev,
                              self.nprunable_rows, self._sums, self.weights, self._scores, hyper,
                              units=self._utable.dev, nunits=self.total_num_groups, unit_sums=self._unit_sums)
        else:
            _lib.prune_scores(self._gtable.dev, ng, self._mtable.dev, self.nmembers, self._itable.dev,
                              self.total_num_groups, self._sums, self.weights, self._scores, hyper)
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

    def finish_step(self, n: int, hyper: tuple) -> None:
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
            _lib.prune_joint_finish(self._gtable.dev, ng, self._partials, self._nred, opt.param_groups[0]["lr"],
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


def _resized_linear(src: nn.Linear, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> nn.Linear:
    """A layer of src's kind around the given weight and bias, src's quantizer scalars and clip values carried over."""
    from .quant_layers import QuantizeLinear
    out_f, in_f = weight.shape
    if isinstance(src, QuantizeLinear):
        new = QuantizeLinear(in_f, out_f, bias=bias is not None, quant_type=src.quant_type, quant_mode=src.quant_mode)
        new.weight_clip_val, new.act_clip_val = src.weight_clip_val, src.act_clip_val
    else:
        new = nn.Linear(in_f, out_f, bias=bias is not None)
    new = new.to(device=weight.device, dtype=weight.dtype)
    new.weight.data.copy_(weight)
    new.weight.requires_grad_(src.weight.requires_grad)
    if bias is not None:
        new.bias.data.copy_(bias)
        new.bias.requires_grad_(src.bias.requires_grad)
    for side in _SIDES:
        for sc in _SCALARS:
            a, b = getattr(src, f"{sc}_{side}", None), getattr(new, f"{sc}_{side}", None)
            if a is not None and b is not None:
                b.data.copy_(a.data)
                b.requires_grad_(a.requires_grad)
    new.train(src.training)
    if callable(getattr(new, "invalidate", None)):
        new.invalidate()
    return new


@torch.no_grad()
def compress_pruned_mlp(model: nn.Module) -> nn.Module:
    """Removes every all-zero fc1 row (weight row and bias entry both zero) of every blocks[i].mlp together with its
    fc2 column, in place, and returns the model: this project's counterpart of the reference's construct_subnet for
    this one structure. The quantizer scalars are carried over and the plans start afresh. An optimizer built over
    the model before the call no longer matches it."""
    for blk in model.blocks:
        fc1, fc2 = blk.mlp.fc1, blk.mlp.fc2
        dead = (fc1.weight == 0).all(dim=1)
        if fc1.bias is not None:
            dead &= fc1.bias == 0
        keep = (~dead).nonzero().flatten()
        if keep.numel() == fc1.out_features:
            continue
        if keep.numel() == 0:
            raise ValueError("compress_pruned_mlp: a block's MLP has no hidden unit left")
        blk.mlp.fc1 = _resized_linear(fc1, fc1.weight[keep], None if fc1.bias is None else fc1.bias[keep])
        blk.mlp.fc2 = _resized_linear(fc2, fc2.weight[:, keep], fc2.bias)
    return model


@torch.no_grad()
def compress_pruned_heads(model: nn.Module) -> nn.Module:
    """Removes every attention head whose q, k and v rows of attn.qkv.weight and entries of attn.qkv.bias are all
    zero, together with the matching columns of attn.proj.weight, in place, and returns the model; sets
    attn.num_heads and leaves head_dim and the softmax scale as they are. The quantizer scalars are carried over and
    the plans start afresh. A removed head's bias entries are zero, so the qkv layer's output bound, and with it the
    attention input scale, is the uncompressed layer's. Composes with compress_pruned_mlp in either order. An
    optimizer built over the model before the call no longer matches it."""
    for blk in model.blocks:
        a = blk.attn
        H, hd = int(a.num_heads), int(a.head_dim)
        if a.qkv.out_features != 3 * H * hd or a.proj.in_features != H * hd:
            raise ValueError(f"compress_pruned_heads: qkv has {a.qkv.out_features} outputs and proj {a.proj.in_features} "
                             f"inputs, not 3 x {H} x {hd} and {H} x {hd}")
        dead = (units_view(a.qkv.weight, H, 3, hd) == 0).all(dim=1)
        if a.qkv.bias is not None:
            dead &= (units_view(a.qkv.bias, H, 3, hd) == 0).all(dim=1)
        keep = (~dead).nonzero().flatten().tolist()
        if len(keep) == H:
            continue
        if not keep:
            raise ValueError("compress_pruned_heads: a block's attention has no head left")
        rows = torch.from_numpy(unit_rows_of(keep, H, 3, hd).reshape(len(keep), 3, hd).transpose(1, 0, 2).reshape(-1)
                                ).to(a.qkv.weight.device)   # section-major again: [3, kept heads, hd]
        cols = torch.from_numpy(unit_rows_of(keep, H, 1, hd)).to(a.qkv.weight.device)
        a.qkv = _resized_linear(a.qkv, a.qkv.weight[rows], None if a.qkv.bias is None else a.qkv.bias[rows])
        a.proj = _resized_linear(a.proj, a.proj.weight[:, cols], a.proj.bias)
        a.num_heads = len(keep)
    return model
