"""ViTAttention.core forward + backward: the HIP path (qvit_attention + qvit_attention_backward behind
_AttentionCore) against the torch branch (the reference's four ops under autograd), alternated in one process.
HIP events, median of 20 after 3 warm-up rounds; peak memory from torch.cuda.max_memory_allocated over one
forward + backward. Usage: python tools/attn_bwd_bench.py [--out profiles/attention_backward_bench.txt]
--hd 80 times the ViT-Huge/14 shape (B=64, N=257, H=16, head dim 80) instead of the two 64-wide shapes."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quantized_vit_amd import build  # noqa: E402
from quantized_vit_amd.vit_model import ViTAttention  # noqa: E402

SHAPES = {64: [("ViT-B/16 b256", 256, 197, 12), ("ViT-L/16 @384 b128", 128, 577, 16)],
          80: [("ViT-H/14 b64", 64, 257, 16)]}
REPS, WARM = 20, 3


def one(attn, qkv, dO, B, N):
    x = qkv.detach().requires_grad_(True)
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record()
    y = attn.core(x, B, N)
    e1.record()
    y.backward(dO)
    e2.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), e1.elapsed_time(e2)


def peak(attn, qkv, dO, B, N):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    one(attn, qkv, dO, B, N)
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--hd", type=int, default=64, choices=(64, 80), help="head dim (selects the shapes)")
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    lines = [f"device: {torch.cuda.get_device_name(0)}; median of {REPS}, HIP events, paths alternated"]
    hd = a.hd
    for name, B, N, H in SHAPES[hd]:
        torch.manual_seed(0)
        hip = ViTAttention(H * hd, num_heads=H).to(dev).eval()
        ref = ViTAttention(H * hd, num_heads=H).to(dev).eval()
        ref.hip_ok = lambda qkv: False          # the parent's route under autograd: torch ops
        qkv = torch.randn(B, N, 3 * H * hd, device=dev)
        dO = torch.randn(B, N, H * hd, device=dev)
        t = {"hip": ([], []), "torch": ([], [])}
        for r in range(WARM + REPS):
            for key, m in (("hip", hip), ("torch", ref)):
                f, b = one(m, qkv, dO, B, N)
                if r >= WARM:
                    t[key][0].append(f)
                    t[key][1].append(b)
        mem = {"hip": peak(hip, qkv, dO, B, N), "torch": peak(ref, qkv, dO, B, N)}
        lines.append(f"{name}: B={B} N={N} H={H} hd={hd}   B*H*N*N*4 = {B * H * N * N * 4 / 2**20:.0f} MiB")
        for key in ("hip", "torch"):
            f, b = statistics.median(t[key][0]), statistics.median(t[key][1])
            lines.append(f"  {key:5s} forward {f:8.3f} ms  backward {b:8.3f} ms  total {f + b:8.3f} ms  "
                         f"peak memory above inputs {mem[key] / 2**20:9.1f} MiB")
        fh = statistics.median(t["hip"][0]) + statistics.median(t["hip"][1])
        ft = statistics.median(t["torch"][0]) + statistics.median(t["torch"][1])
        lines.append(f"  torch / hip total = {ft / fh:.2f}x   memory saved = {(mem['torch'] - mem['hip']) / 2**20:.0f} MiB")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
