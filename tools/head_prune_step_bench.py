"""Two measurements for the head groups of the QAT optimizer.

1. The joint-stage QuantAwareOptimizer.step() (adamw) on ViT-B/16 and ViT-L/16 parameter sets with head AND MLP groups,
   every second unit of every group active redundant, against (a) the range-stage step without groups and (b) the joint
   step with the MLP groups only, all in one job, beside the expectation from bytes, 1 + 16 B x redundant elements /
   (28 B x elements), and with the member update and the reduce timed alone.
2. What a compressed model buys: the ViT-B/16 batch-256 forward with 6 of 12 heads left in every block against the full
   model, with the per-kernel times of the fused qkv + attention kernel and of proj (vit_model.KERNEL_TIMING).

Usage: python tools/head_prune_step_bench.py [--out profiles/head_prune_step_bench.txt] [--models base large]
Same process, same device; medians of `reps` after `warmup` untimed ones; wall time from an idle device to an idle
device for the steps and the forwards, device time between two events for the single kernels."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from prune_step_bench import ADAMW, PRUNE, RANGE, install   # noqa: E402
from qat_step_bench import MODELS, build_model, device_ms, wall_ms   # noqa: E402

from quantized_vit_amd import (QuantAwareOptimizer, _lib, build, compress_pruned_heads, vit_head_prune_groups,   # noqa: E402
                               vit_mlp_prune_groups, vit_model)
from quantized_vit_amd.qat_prune import unit_rows_of   # noqa: E402


def joint(model, groups, a):
    """(wall ms of a joint step, apply kernel ms, reduce kernel ms, member elements, redundant elements)."""
    opt = QuantAwareOptimizer(model, prune_groups=groups, **ADAMW, **RANGE, **PRUNE)
    pr = opt._prune
    install(pr.groups, opt, pr)
    pr._tables()
    t = wall_ms(opt.step, a.warmup, a.reps)
    assert pr._nred and pr.curr_period == 1, "the timed steps were not joint steps"
    ng, hyper = len(pr.groups), opt._hyper(False)
    member_n = sum(g.num_groups * int(pr._grow["elems"][i]) for i, g in enumerate(pr.groups))
    red_n = sum(len(g.active) * int(pr._grow["elems"][i]) for i, g in enumerate(pr.groups))
    t_apply = device_ms(lambda: _lib.prune_joint_apply(pr._gtable.dev, ng, pr._mtable.dev, pr.nmembers, pr._itable.dev,
                                                       pr.nrows, pr.gamma, hyper), a.warmup, a.reps)
    t_reduce = device_ms(lambda: _lib.prune_joint_reduce(pr._gtable.dev, ng, pr._mtable.dev, pr.nmembers,
                                                         pr._rtable.dev, pr._nred, pr._partials, hyper),
                         a.warmup, a.reps)
    return t, t_apply, t_reduce, member_n, red_n


def forward_times(model, img, a):
    """(wall ms of a forward, median device ms per launch of the timed kernels)."""
    def run():
        with torch.no_grad():
            model(img)
    t = wall_ms(run, a.warmup, a.reps)
    names = ("qkv_attn", "proj")
    for n in names:
        vit_model.KERNEL_TIMING[n] = []
    for _ in range(a.reps):
        run()
    torch.cuda.synchronize()
    per = {n: statistics.median(s.elapsed_time(e) for s, e in vit_model.KERNEL_TIMING.pop(n)) for n in names}
    return t, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_prune_step_bench.txt"))
    ap.add_argument("--models", nargs="+", default=["base", "large"], choices=list(MODELS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    lines = [f"# head_prune_step_bench: {torch.cuda.get_device_name(0)}, library {_lib.build_id()}, "
             f"torch {torch.__version__}",
             f"# adamw; medians of {a.reps} steps after {a.warmup} untimed; wall ms from an idle device to an idle "
             "device; every second unit of every group active redundant",
             "# model | groups | joint step ms | range step ms (no groups) | ratio to range | expected 1 + 16 B red / "
             "28 B all | ratio to the MLP-only joint step | apply kernel ms, GB/s | reduce kernel ms, GB/s"]
    gb = lambda n, bytes_per, ms: n * bytes_per / (ms * 1e-3) / 1e9   # noqa: E731
    for mname in a.models:
        model = build_model(mname, dev)
        state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        opt0 = QuantAwareOptimizer(model, **ADAMW, **RANGE, fix_after_step=10 ** 9)
        t_range = wall_ms(opt0.step, a.warmup, a.reps)
        dense_n = sum(p.numel() for _, p in opt0._dense)
        del opt0
        t_mlp = None
        for label, make in (("mlp", lambda m: vit_mlp_prune_groups(m)),
                            ("heads+mlp", lambda m: vit_head_prune_groups(m) + vit_mlp_prune_groups(m))):
            model.load_state_dict(state0)
            t, t_apply, t_reduce, member_n, red_n = joint(model, make(model), a)
            t_mlp = t if t_mlp is None else t_mlp
            line = (f"{mname} ({dense_n / 1e6:.1f} M) | {label} (members {member_n / 1e6:.1f} M, redundant "
                    f"{red_n / 1e6:.1f} M) | {t:.3f} | {t_range:.3f} | {t / t_range:.3f} | "
                    f"{1.0 + 16.0 * red_n / (28.0 * dense_n):.3f} | {t / t_mlp:.3f} | {t_apply:.3f}, "
                    f"{gb(member_n, 28, t_apply):.0f} | {t_reduce:.3f}, {gb(red_n, 16, t_reduce):.0f}")
            print(line, flush=True)
            lines.append(line)
        del model
        torch.cuda.empty_cache()

    # the compressed model
    from quantized_vit_amd.calibrate import build_quantized_vit, synthetic_images
    lines.append(f"# ViT-B/16 W4A8 forward, batch {a.batch}: heads per block | forward ms | fused qkv + attention ms per "
                 "block | proj ms per block")
    img = synthetic_images(a.batch, 224, seed=7).to(dev)
    model = build_quantized_vit("vit_base_patch16_224", seed=0).to(dev).eval()
    res = {}
    for heads in (12, 6):
        if heads == 6:
            with torch.no_grad():
                for blk in model.blocks:
                    rows = torch.from_numpy(unit_rows_of(range(6, 12), 12, 3, 64)).to(dev)
                    blk.attn.qkv.weight[rows] = 0
                    blk.attn.qkv.bias[rows] = 0
            compress_pruned_heads(model)
            assert all(b.attn.num_heads == 6 for b in model.blocks)
        res[heads] = forward_times(model, img, a)
        t, per = res[heads]
        line = f"{heads} | {t:.3f} | {per['qkv_attn']:.4f} | {per['proj']:.4f}"
        print(line, flush=True)
        lines.append(line)
    (t12, p12), (t6, p6) = res[12], res[6]
    lines.append(f"# 6 / 12 heads: forward {t6 / t12:.3f}, fused qkv + attention {p6['qkv_attn'] / p12['qkv_attn']:.3f}, "
                 f"proj {p6['proj'] / p12['proj']:.3f}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
