"""qvit_gemm_f32w (frozen, pre-split weights) against the library's fp32 GEMM and qvit_gemm_f32_nt on the qkv / proj /
fc1 / fc2 forward shapes of ViT-B/16 b256 and ViT-L/16 @384 b128, at both precisions (six and three bf16 products),
and one end-to-end line: the ViT-B/16 b256 teacher forward with and without prepare_teacher.

    python tools/gemm_f32w_bench.py [--rounds 15] [--models vit_b,vit_l] [--no-e2e] [--out profiles/gemm_f32w_bench.txt]

Each sample is one call between two HIP events on the launch stream; the routes of a shape alternate sample by sample
inside one process after every one of them was warmed up; a row reports the median TFLOP/s (2 M N K / t) of each
route, its quartiles in microseconds, the relative error against the float64 product on a sample of 64 rows (max |err|
/ max |ref|), and `win` / `loss` against the library and against gemm_f32 where the quartile ranges do not overlap
(a difference larger than the run-to-run spread of this file), `-` where they do.
"""
import argparse
import copy
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantized_vit_amd import _lib, prepare_teacher  # noqa: E402
from quantized_vit_amd.vit_model import vit_base_patch16_224  # noqa: E402

MODELS = {"vit_b": ("ViT-B/16 b256", 50432, 768), "vit_l": ("ViT-L/16 @384 b128", 73856, 1024)}


def samples(fns, rounds):
    """Per-call microseconds of each fn, `rounds` sorted samples each, alternating the fns sample by sample."""
    for f in fns:          # warm-up: code objects, the library's algorithm choice, the allocator
        for _ in range(3):
            f()
    ev = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            ev[i].append((s, e))
    torch.cuda.synchronize()
    return [sorted(s.elapsed_time(e) * 1e3 for s, e in row) for row in ev]


def quartiles(v):
    return v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]


def verdict(t, other):
    """`t` against `other` by the quartile rule."""
    (q1, _, q3), (o1, _, o3) = quartiles(t), quartiles(other)
    return "win" if q3 < o1 else ("loss" if q1 > o3 else "-")


def bench_shape(dev, tag, layer, M, K, N, rounds, out):
    gen = torch.Generator(device=dev).manual_seed(M + K + N)
    x = torch.randn(M, K, device=dev, generator=gen)
    W = torch.randn(N, K, device=dev, generator=gen) * 0.02
    b = torch.randn(N, device=dev, generator=gen) * 0.01
    img3, img2 = _lib.pack_weight_b3(W, 3), _lib.pack_weight_b3(W, 2)
    y = torch.empty(M, N, device=dev)
    rows = torch.arange(0, M, M // 64, device=dev)[:64]
    ref = x[rows].double() @ W.double().t() + b.double()
    routes = [("library", lambda: F.linear(x, W, b)),
              ("gemm_f32", lambda: _lib.gemm_f32_nt(x, W, b, out=y)),
              ("f32w fp32", lambda: _lib.gemm_f32w(x, img3, N, 6, b, out=y)),
              ("f32w bf16x2", lambda: _lib.gemm_f32w(x, img2, N, 3, b, out=y))]
    times = samples([f for _, f in routes], rounds)
    flops = 2.0 * M * N * K
    for (name, f), t in zip(routes, times):
        q1, med, q3 = quartiles(t)
        err = float((f()[rows].double() - ref).abs().max() / ref.abs().max())
        vs = "" if name == "library" else f"vs library {verdict(t, times[0])}"
        if name.startswith("f32w"):
            vs += f", vs gemm_f32 {verdict(t, times[1])}"
        out(f"{tag:18s} {layer:4s} M={M:5d} N={N:4d} K={K:4d} {name:11s} {flops / med / 1e6:7.1f} TFLOP/s  "
            f"q1 {q1:8.1f} med {med:8.1f} q3 {q3:8.1f} us  rel err {err:.2e}  {vs}")


def bench_teacher(dev, rounds, out):
    """The ViT-B/16 b256 teacher forward (utils.py:268-274: once per step under no_grad)."""
    torch.manual_seed(0)
    plain = vit_base_patch16_224().to(dev).eval().requires_grad_(False)
    models = [("torch", plain), ("prepare_teacher fp32", prepare_teacher(copy.deepcopy(plain), "fp32")),
              ("prepare_teacher bf16x2", prepare_teacher(copy.deepcopy(plain), "bf16x2"))]
    img = torch.randn(256, 3, 224, 224, device=dev)
    with torch.no_grad():
        want = plain(img).double()
        times = samples([lambda m=m: m(img) for _, m in models], rounds)
        for (name, m), t in zip(models, times):
            q1, med, q3 = quartiles(t)
            diff = float((m(img).double() - want).abs().max() / want.abs().max())
            vs = "" if name == "torch" else f"vs torch {verdict(t, times[0])}"
            out(f"ViT-B/16 b256 teacher forward {name:22s} q1 {q1 / 1e3:7.2f} med {med / 1e3:7.2f} q3 {q3 / 1e3:7.2f} ms  "
                f"max |logit diff| / max |logit| vs torch {diff:.2e}  {vs}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--models", default="vit_b,vit_l")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_f32w_bench needs a GPU: nothing is timed without one")
    dev = torch.device("cuda:0")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # kept up to date line by line
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    out(f"gemm_f32w bench: {a.rounds} alternated samples per route, HIP events, {torch.cuda.get_device_name(0)}")
    for m in [m for m in a.models.split(",") if m]:
        tag, M, D = MODELS[m]
        for layer, N, K in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", 4 * D, D), ("fc2", D, 4 * D)):
            bench_shape(dev, tag, layer, M, K, N, a.rounds, out)
            torch.cuda.empty_cache()
    if not a.no_e2e:
        bench_teacher(dev, max(5, a.rounds // 2), out)


if __name__ == "__main__":
    main()
