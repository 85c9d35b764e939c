"""Times QuantAwareOptimizer.step() on ViT-B/16 and ViT-L/16 parameter sets in every stage and variant, against
  * a literal torch transcription of the reference's step on the same device (tests/qat_step_ref.py: StepTorch, a
    per-parameter loop that reads q_m and t_quant back with .item());
  * torch.optim.AdamW(fused=True) over the dense tensors, as an outside mark;
and reports the dense kernel's achieved bytes per second against the HBM peak.

Usage: python tools/qat_step_bench.py [--out profiles/qat_step_bench.txt] [--models base large] [--reps 20]
Same process, same device, the candidates interleaved per configuration; medians of `reps` timed steps after
`warmup` untimed ones, device time between two events around the step (host launch work included: the queue is
drained before the first event, so a host-bound step shows as such)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from qat_step_ref import Hyper, StepTorch   # noqa: E402

from quantized_vit_amd import QuantAwareOptimizer, _lib, build, model_to_quantize_model   # noqa: E402
from quantized_vit_amd import vit_model   # noqa: E402

HBM_PEAK = 8.0e12   # bytes / s, the MI355X specification
VARIANTS = {
    "sgd": dict(variant="sgd", first_momentum=0.9, dampening=0.1, weight_decay=1e-2),
    "adam": dict(variant="adam", first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2),
    "adamw": dict(variant="adamw", first_momentum=0.9, second_momentum=0.999, weight_decay=1e-2),
}
STAGES = {
    "warmup": dict(start_projection_step=10 ** 9, fix_after_step=2 * 10 ** 9),
    "range": dict(start_projection_step=0, projection_steps=10 ** 6, projection_periods=1, fix_after_step=10 ** 9),
    "fix": dict(start_projection_step=0, fix_after_step=0),
}
BYTES_PER_ELEMENT = {"sgd": 20, "adam": 28, "adamw": 28}
MODELS = {"base": "vit_base_patch16_224", "large": "vit_large_patch16_224"}


def wall_ms(fn, warmup, reps):
    """Median wall time of fn() from an idle device to an idle device."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def device_ms(fn, warmup, reps):
    """Median device time of fn() between two events."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def build_model(name, dev):
    torch.manual_seed(0)
    model = getattr(vit_model, MODELS[name])().to(dev)
    model = model_to_quantize_model(model, num_bits=8, quant_mode="weight_and_activation")
    for p in model.parameters():
        p.grad = torch.randn_like(p) * (0.01 if p.numel() == 1 else 1.0)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qat_step_bench.txt"))
    ap.add_argument("--models", nargs="+", default=["base", "large"], choices=list(MODELS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-reps", type=int, default=5)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    lines = [f"# qat_step_bench: {torch.cuda.get_device_name(0)}, library {_lib.build_id()}, torch {torch.__version__}",
             f"# medians of {a.reps} steps ({a.ref_reps} for the transcription) after {a.warmup} untimed; wall ms from "
             "an idle device to an idle device",
             "# model variant stage | step ms | transcription ms | ratio | fused AdamW (dense only) ms | "
             "dense kernel ms | dense GB/s | of HBM peak"]
    for mname in a.models:
        model = build_model(mname, dev)
        state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        nparam = sum(p.numel() for p in model.parameters())
        for vname, vkw in VARIANTS.items():
            for sname, skw in STAGES.items():
                model.load_state_dict(state0)
                opt = QuantAwareOptimizer(model, lr=1e-5, lr_quant=1e-6, **vkw, **skw)
                t_step = wall_ms(opt.step, a.warmup, a.reps)
                dense_n = sum(p.numel() for _, p in opt._dense)
                hyper = opt._hyper(False)
                t_dense = device_ms(lambda: _lib.qat_step(opt._ttable.dev, len(opt._dense), opt._chunks,
                                                          opt._nchunks, hyper), a.warmup, a.reps)
                gbs = dense_n * BYTES_PER_ELEMENT[vname] / (t_dense * 1e-3)
                # the transcription, on the same parameters and gradients (it clones the gradients as the
                # reference does)
                model.load_state_dict(state0)
                params = {n: p.detach() for n, p in model.named_parameters()}
                grads = {n: p.grad for n, p in model.named_parameters()}
                ref = StepTorch(params, Hyper(lr=1e-5, lr_quant=1e-6, **vkw, **skw))
                t_ref = wall_ms(lambda: ref.step(grads), 2, a.ref_reps)
                t_fused = float("nan")
                if vname == "adamw":
                    model.load_state_dict(state0)
                    fused = torch.optim.AdamW([p for _, p in opt._dense], lr=1e-5, weight_decay=1e-2, fused=True)
                    t_fused = wall_ms(fused.step, a.warmup, a.reps)
                    del fused
                line = (f"{mname} ({nparam / 1e6:.1f} M) {vname} {sname} | {t_step:.3f} | {t_ref:.3f} | "
                        f"{t_ref / t_step:.1f}x | {t_fused:.3f} | {t_dense:.3f} | {gbs / 1e9:.0f} | "
                        f"{100 * gbs / HBM_PEAK:.0f} %")
                print(line, flush=True)
                lines.append(line)
                del opt, ref
        del model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
