"""Times forward plus backward of the full training objective (label smoothing, mixup, distillation) through
TrainLoss (qvit_train_loss, two launches) against a literal torch transcription of the reference's loss lines
(tests/train_loss_ref.py: utils.py:120-154, :264-280, with the accuracy count of :261-262) on the same device, and
reports the row kernel's time against its byte floor.

Usage: python tools/train_loss_bench.py [--out profiles/train_loss_bench.txt] [--reps 50] [--warmup 10]
Same process, same device, the two versions alternating rep by rep; medians of device time between two events around
forward + backward (host launch work included: the queue is drained before the first event, so a launch-bound
version shows as such). Launch counts and the kernel's own time come from one torch.profiler pass per version, apart
from the timed ones."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_loss_ref as R   # noqa: E402

from quantized_vit_amd import TrainLoss, _lib, build   # noqa: E402

HBM_PEAK = 8.0e12    # bytes / s, the MI355X specification
FP32_PEAK = 157e12   # vector fp32 operations / s
RESIDENT = 4096      # train_loss.hip kResident: longer rows are read twice
SHAPES = [(256, 1000), (128, 1000), (256, 21843)]
EPS, GAMMA, ALPHA, TEMP = 0.1, 0.3, 0.5, 5.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def device_ops(fn):
    """{kernel name: (count, device microseconds)} of one call of fn."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ops = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            n, us = ops.get(e.name, (0, 0.0))
            ops[e.name] = (n + 1, us + (e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total))
    return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_loss_bench.txt"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    lines = [f"# train_loss_bench: {torch.cuda.get_device_name(0)}, library {_lib.build_id()}, torch {torch.__version__}",
             f"# full objective: smoothing {EPS}, mixup gamma {GAMMA}, KD alpha {ALPHA} at T {TEMP}; forward + backward, "
             f"medians of {a.reps} alternating reps after {a.warmup} untimed, device ms between two events",
             "# B x C | TrainLoss ms | torch transcription ms | ratio | launches (HIP / torch) | row kernel us | "
             "byte floor us | kernel / floor | fp32 floor us | bound by"]
    crit = TrainLoss(label_smoothing=EPS, kd_alpha=ALPHA, kd_temperature=TEMP)
    for B, C in SHAPES:
        g = torch.Generator().manual_seed(B + C)
        s = (torch.randn(B, C, generator=g) * 3).to(dev).requires_grad_(True)
        t = (torch.randn(B, C, generator=g) * 3).to(dev)
        labels = torch.randint(0, C, (B,), generator=g).to(dev)
        perm = torch.randperm(B, generator=g).to(dev)
        labels_b = labels[perm]

        def ours():
            s.grad = None
            res = crit(s, labels, teacher_logits=t, mix=(labels_b, GAMMA))
            res.loss.backward()
            return res.loss, res.correct

        def transcription():
            s.grad = None
            loss, _, _, correct = R.objective(s, labels, EPS, perm, GAMMA, t, ALPHA, TEMP, torch.float32)
            loss.backward()
            return loss, correct

        for _ in range(a.warmup):
            ours()
            transcription()
        t_ours, t_ref = [], []
        for _ in range(a.reps):
            t_ours.append(timed(ours))
            t_ref.append(timed(transcription))
        t_ours, t_ref = statistics.median(t_ours), statistics.median(t_ref)
        check = abs(ours()[0].item() - transcription()[0].item())
        assert check < 1e-4, check   # (both compute the same objective)
        ops_ours, ops_ref = device_ops(ours), device_ops(transcription)
        n_ours, n_ref = (sum(n for n, _ in o.values()) for o in (ops_ours, ops_ref))
        k_us = sum(us / n for name, (n, us) in ops_ours.items() if "train_loss_row_kernel" in name)
        reads = 1 if C <= RESIDENT else 2
        floor_us = B * C * 4 * (2 * reads + 1) / HBM_PEAK * 1e6        # student + teacher read, gradient written
        flops_us = B * C * (3 + 3 * reads) * 20 / FP32_PEAK * 1e6      # about 20 operations per exp
        bound = "bytes" if floor_us >= flops_us else "fp32"
        slower = "" if t_ours < t_ref else "  (NOT faster than the transcription here)"
        line = (f"{B} x {C} | {t_ours:.3f} | {t_ref:.3f} | {t_ref / t_ours:.1f}x | {n_ours} / {n_ref} | {k_us:.1f} | "
                f"{floor_us:.1f} | {k_us / floor_us:.1f}x | {flops_us:.1f} | {bound}{slower}")
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
