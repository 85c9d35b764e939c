"""Times a joint-stage QuantAwareOptimizer.step() (adamw, the MLP groups of vit_mlp_prune_groups with half of every
group's rows active redundant) on ViT-B/16 and ViT-L/16 parameter sets against
  * the range-stage step() without prune_groups on the same parameters: the code path of before this feature, so
    the baseline is taken on the same box in the same job;
  * a literal torch transcription of the joint stage on the same device (tests/prune_step_ref.py: PruneTorch, the
    reference's gathers, torch.cat, norms and dots read back with .item(), and its host loop);
and puts the measured ratio beside the expectation from bytes: the joint stage reads the redundant rows of p, grad,
m and v once more for the reduce, so joint / range should be near 1 + 16 B x redundant elements / (28 B x elements).
The member update and the reduce are also timed alone, with the bytes they move, to say where a gap comes from.

Usage: python tools/prune_step_bench.py [--out profiles/prune_step_bench.txt] [--models base large] [--reps 20]
Same process, same device, candidates interleaved per model; medians of `reps` steps after `warmup` untimed ones;
wall time from an idle device to an idle device (host work included), device time between two events for the single
kernels. The redundant sets are installed by hand and the period is long, so that every timed step is a joint step."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from prune_step_ref import Group, PruneHyper, PruneTorch   # noqa: E402
from qat_step_bench import HBM_PEAK, MODELS, build_model, device_ms, wall_ms   # noqa: E402

from quantized_vit_amd import QuantAwareOptimizer, _lib, build, vit_mlp_prune_groups   # noqa: E402

ADAMW = dict(variant="adamw", first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2, lr=1e-5, lr_quant=1e-6)
RANGE = dict(start_projection_step=0, projection_steps=10 ** 6, projection_periods=1)
PRUNE = dict(start_pruning_step=1, pruning_steps=10 ** 6, pruning_periods=1, target_group_sparsity=0.5)


def install(groups, num_steps_owner, period_owner):
    """Every second row of every group active redundant; no boundary fires (the period counter is past the end)."""
    for g in groups:
        g.active = list(range(0, g.num_groups, 2))
        g.pruned = []
        g.important = [i for i in range(g.num_groups) if i % 2]
    num_steps_owner.num_steps = 1
    setattr(period_owner, "curr_period", 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_step_bench.txt"))
    ap.add_argument("--models", nargs="+", default=["base", "large"], choices=list(MODELS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-reps", type=int, default=3)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    lines = [f"# prune_step_bench: {torch.cuda.get_device_name(0)}, library {_lib.build_id()}, "
             f"torch {torch.__version__}",
             f"# adamw; medians of {a.reps} steps ({a.ref_reps} for the transcription) after {a.warmup} untimed; wall "
             "ms from an idle device to an idle device; half of every MLP group's rows active redundant",
             "# model | joint step ms | range step ms (no groups) | measured ratio | expected 1 + 16 B red / 28 B all "
             "| transcription ms | transcription / joint | apply kernel ms, GB/s, of HBM peak | reduce kernel ms, GB/s "
             "| dense kernel (no groups) ms, GB/s | dense kernel (members out) ms"]
    for mname in a.models:
        model = build_model(mname, dev)
        state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        nparam = sum(p.numel() for p in model.parameters())

        # the baseline: the range stage without groups
        opt0 = QuantAwareOptimizer(model, **ADAMW, **RANGE, fix_after_step=10 ** 9)
        t_range = wall_ms(opt0.step, a.warmup, a.reps)
        hyper0 = opt0._hyper(False)
        t_dense0 = device_ms(lambda: _lib.qat_step(opt0._ttable.dev, len(opt0._dense), opt0._chunks, opt0._nchunks,
                                                   hyper0), a.warmup, a.reps)
        dense_n = sum(p.numel() for _, p in opt0._dense)
        del opt0

        # the joint stage
        model.load_state_dict(state0)
        opt = QuantAwareOptimizer(model, prune_groups=vit_mlp_prune_groups(model), **ADAMW, **RANGE, **PRUNE)
        pr = opt._prune
        install(pr.groups, opt, pr)
        pr._tables()
        t_joint = wall_ms(opt.step, a.warmup, a.reps)
        assert pr._nred and pr.curr_period == 1, "the timed steps were not joint steps"
        ng, hyper = len(pr.groups), opt._hyper(False)
        member_n = sum(g.num_groups * int(pr._grow["elems"][i]) for i, g in enumerate(pr.groups))
        red_n = sum(len(g.active) * int(pr._grow["elems"][i]) for i, g in enumerate(pr.groups))
        t_apply = device_ms(lambda: _lib.prune_joint_apply(pr._gtable.dev, ng, pr._mtable.dev, pr.nmembers,
                                                           pr._itable.dev, pr.nrows, pr.gamma, hyper),
                            a.warmup, a.reps)
        t_reduce = device_ms(lambda: _lib.prune_joint_reduce(pr._gtable.dev, ng, pr._mtable.dev, pr.nmembers,
                                                             pr._rtable.dev, pr._nred, pr._partials, hyper),
                             a.warmup, a.reps)
        t_dense1 = device_ms(lambda: _lib.qat_step(opt._ttable.dev, len(opt._dense), opt._chunks, opt._nchunks, hyper),
                             a.warmup, a.reps)
        expected = 1.0 + 16.0 * red_n / (28.0 * dense_n)

        # the transcription of the joint stage, same parameters, gradients and redundant sets
        model.load_state_dict(state0)
        params = {n: p.detach() for n, p in model.named_parameters()}
        grads = {n: p.grad for n, p in model.named_parameters()}
        rgroups = [Group(g.name, f"{g.name}.fc1", [f"{g.name}.fc1.weight", f"{g.name}.fc1.bias"]) for g in pr.groups]
        ref = PruneTorch(params, PruneHyper(**ADAMW, **RANGE, **PRUNE), rgroups)
        install(ref.groups, ref, ref)
        t_ref = wall_ms(lambda: ref.step(grads), 1, a.ref_reps)
        assert ref.last and ref.curr_period == 1, "the transcription's steps were not joint steps"

        gb = lambda n, bytes_per, ms: n * bytes_per / (ms * 1e-3) / 1e9   # noqa: E731
        line = (f"{mname} ({nparam / 1e6:.1f} M, members {member_n / 1e6:.1f} M, redundant {red_n / 1e6:.1f} M) | "
                f"{t_joint:.3f} | {t_range:.3f} | {t_joint / t_range:.3f} | {expected:.3f} | {t_ref:.1f} | "
                f"{t_ref / t_joint:.0f}x | {t_apply:.3f}, {gb(member_n, 28, t_apply):.0f}, "
                f"{100 * gb(member_n, 28, t_apply) * 1e9 / HBM_PEAK:.0f} % | {t_reduce:.3f}, "
                f"{gb(red_n, 16, t_reduce):.0f} | {t_dense0:.3f}, {gb(dense_n, 28, t_dense0):.0f} | {t_dense1:.3f}")
        print(line, flush=True)
        lines.append(line)
        del opt, ref, model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
