"""Times the group-lasso penalty of QuantAwareOptimizer (group_lasso_lambda; qvit_group_lasso) on the ViT-B/16 and
ViT-L/16 parameter sets with vit_head_prune_groups + vit_mlp_prune_groups:
  (a) the penalty alone, all its launches, device time between two events, against the fp32 torch transcription of
      the reference (tests/group_lasso_ref.py: penalty_torch, forward + autograd.grad into .grad) on the same device;
  (b) step() with the penalty against step() with group_lasso_lambda=None on the same parameters, the steps
      interleaved, beside the expectation from bytes: 12 B per member element (p read, grad read and written) on the
      step's 28 B, and 4 B more per element of the head units, whose p is read twice;
  (c) the one-row pass (the MLP groups alone) and the passes of the head groups alone with the bytes they move; the
      head groups' gradient pass is the difference between lambda > 0 and lambda = 0, which skips it.

Usage: python tools/group_lasso_bench.py [--out profiles/group_lasso_bench.txt] [--models base large] [--reps 20]
Same process, same device; medians of `reps` after `warmup` untimed; wall ms from an idle device to an idle device for
the steps, device ms for the penalty."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from group_lasso_ref import penalty_torch   # noqa: E402
from qat_step_bench import HBM_PEAK, MODELS, build_model, device_ms   # noqa: E402

from quantized_vit_amd import (QuantAwareOptimizer, _lib, build, vit_head_prune_groups,   # noqa: E402
                               vit_mlp_prune_groups)

ADAMW = dict(variant="adamw", first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2, lr=1e-5, lr_quant=1e-6)
SCHED = dict(start_projection_step=0, projection_steps=10 ** 6, projection_periods=1, start_pruning_step=10 ** 6,
             pruning_steps=10 ** 6, pruning_periods=1)   # no boundary in the timed steps
LAMBDA = 1e-6


def interleaved_wall_ms(fns, warmup, reps):
    """Medians of fn() for every fn, one call of each in turn, from an idle device to an idle device."""
    times = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                times[i].append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(t) for t in times]


def penalty_call(opt, lam):
    pr = opt._prune
    ptrs = np.array([opt._grad_ptr(n, p) for n, p in opt._dense], dtype=np.int64)
    fresh = np.zeros(len(ptrs), dtype=bool)
    return lambda: pr.penalty(lam, ptrs, fresh)


def unit_elems(opt):
    pr = opt._prune
    return sum(g.num_groups * int(pr._grow["elems"][i]) for i, g in enumerate(pr.groups) if g.prunable)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_lasso_bench.txt"))
    ap.add_argument("--models", nargs="+", default=["base", "large"], choices=list(MODELS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-reps", type=int, default=5)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    gbs = lambda n, per, ms: n * per / (ms * 1e-3) / 1e9   # noqa: E731
    lines = [f"# group_lasso_bench: {torch.cuda.get_device_name(0)}, library {_lib.build_id()}, torch "
             f"{torch.__version__}",
             f"# adamw, lambda {LAMBDA}; medians of {a.reps} ({a.ref_reps} for the transcription) after {a.warmup} "
             "untimed; head + MLP groups",
             "# model | (a) penalty device ms, GB/s at 12 B (+ 4 B head), of HBM peak | transcription device ms | "
             "transcription / penalty | (b) step with penalty ms | step without ms | measured ratio | expected from "
             "bytes | (c) one-row pass ms, GB/s at 12 B | head passes ms, GB/s at 16 B | head gradient pass ms, GB/s at "
             "12 B"]
    for mname in a.models:
        model = build_model(mname, dev)
        both = lambda: vit_head_prune_groups(model) + vit_mlp_prune_groups(model)   # noqa: E731
        make = lambda groups, lam: QuantAwareOptimizer(model, prune_groups=groups, group_lasso_lambda=lam,   # noqa
                                                       **ADAMW, **SCHED)
        opt, opt0 = make(both(), LAMBDA), make(both(), None)
        pr = opt._prune
        n_all = unit_elems(opt)
        dense_n = sum(p.numel() for _, p in opt._dense)

        t_pen = device_ms(penalty_call(opt, LAMBDA), a.warmup, a.reps)
        ref_groups = [(pr.groups[gi].members, pr.groups[gi].sections, pr.groups[gi].unit_rows) for gi in pr.order
                      if pr.groups[gi].prunable]
        t_ref = device_ms(lambda: penalty_torch(ref_groups, None, LAMBDA), 1, a.ref_reps)
        t_with, t_without = interleaved_wall_ms([opt.step, opt0.step], a.warmup, a.reps)
        del opt0

        mlp, head = make(vit_mlp_prune_groups(model), LAMBDA), make(vit_head_prune_groups(model), LAMBDA)
        n_mlp, n_head = unit_elems(mlp), unit_elems(head)
        t_mlp = device_ms(penalty_call(mlp, LAMBDA), a.warmup, a.reps)
        t_head = device_ms(penalty_call(head, LAMBDA), a.warmup, a.reps)
        t_head0 = device_ms(penalty_call(head, 0.0), a.warmup, a.reps)
        t_grad = t_head - t_head0
        bytes_pen = 12 * n_all + 4 * n_head
        expected = 1.0 + bytes_pen / (28.0 * dense_n)
        line = (f"{mname} (dense {dense_n / 1e6:.1f} M, members {n_all / 1e6:.1f} M, of them heads "
                f"{n_head / 1e6:.1f} M) | {t_pen:.3f}, {gbs(bytes_pen, 1, t_pen):.0f}, "
                f"{100 * gbs(bytes_pen, 1, t_pen) * 1e9 / HBM_PEAK:.0f} % | {t_ref:.2f} | {t_ref / t_pen:.0f}x | "
                f"{t_with:.3f} | {t_without:.3f} | {t_with / t_without:.3f} | {expected:.3f} | {t_mlp:.3f}, "
                f"{gbs(n_mlp, 12, t_mlp):.0f} | {t_head:.3f}, {gbs(n_head, 16, t_head):.0f} | {t_grad:.3f}, "
                f"{gbs(n_head, 12, t_grad):.0f}")
        print(line, flush=True)
        lines.append(line)
        del opt, mlp, head, model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
