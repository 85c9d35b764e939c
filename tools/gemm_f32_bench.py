"""qvit_gemm_f32_nt / qvit_gemm_f32_tn against the library's fp32 GEMMs on the qkv / proj / fc1 / fc2 shapes of
ViT-B/16 b256 and ViT-L/16 @384 b128: forward (x @ W^T + b), dgrad (G @ W) and wgrad (G^T @ x); for the forward also
qvit_gemm_wonly on W16 and W24 images of the same shape (what a plan of at most 24 bits runs today).

    python tools/gemm_f32_bench.py [--rounds 15] [--models vit_b,vit_l] [--out profiles/gemm_f32_bench.txt]

Each sample is one call between two HIP events on the launch stream (a call here takes 0.5 to 10 ms); the routes of a
shape alternate sample by sample inside one process after every one of them was warmed up; a row reports the median
TFLOP/s (2 M N K / t) of each route, its quartiles in microseconds, the relative error of each route's result against
the float64 product on a sample of 64 rows (max |err| / max |ref|), and `win` where the kernel's upper quartile lies
below the library's lower quartile (a difference larger than the run-to-run spread of this file).
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantized_vit_amd import _lib  # noqa: E402

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


def rel_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def bench_shape(dev, tag, layer, M, K, N, rounds, out):
    gen = torch.Generator(device=dev).manual_seed(M + K + N)
    x = torch.randn(M, K, device=dev, generator=gen)
    G = torch.randn(M, N, device=dev, generator=gen)
    W = torch.randn(N, K, device=dev, generator=gen) * 0.02
    b = torch.randn(N, device=dev, generator=gen) * 0.01
    Wt = W.t().contiguous()
    flops = 2.0 * M * N * K
    rows = torch.arange(0, M, M // 64, device=dev)[:64]
    y, gx, gw = (torch.empty(M, N, device=dev), torch.empty(M, K, device=dev), torch.empty(N, K, device=dev))
    ws = torch.empty(_lib.gemm_f32_tn_splits(M, N, K) * _lib.round_up(N, 128) * _lib.round_up(K, 128), device=dev)
    # the weight-only opponents: W16 / W24 code images of the same shape (random codes over the whole range of
    # two and three balanced base-256 digits)
    npad, kpad = _lib.round_up(N, _lib.TILE_N), _lib.round_up(K, _lib.TILE_K)
    wide = []
    for name, top in (("wonly W16", 32639), ("wonly W24", 127 * 65793)):
        codes = torch.randint(-top, top + 1, (N, K), device=dev, generator=gen).float()
        packed, wfmt = _lib.pack_weight_wide(codes, npad, kpad)
        d_wt = torch.tensor([0.02 / top], device=dev)
        wide.append((name, codes, packed, wfmt, d_wt, _lib.pad_bias(b, N, npad, dev)))
    ops = [
        ("fwd", [("library", lambda: F.linear(x, W, b)), ("gemm_f32", lambda: _lib.gemm_f32_nt(x, W, b, out=y))] +
         [(nm, (lambda pk=pk, wf=wf, dw=dw, bp=bp: _lib.gemm_wonly_rows(x, K, kpad, pk, wf, N, npad, dw, bp)))
          for nm, _, pk, wf, dw, bp in wide],
         lambda r: x[r].double() @ W.double().t() + b.double()),
        ("dgrad", [("library", lambda: torch.mm(G, W)), ("gemm_f32", lambda: _lib.gemm_f32_nt(G, Wt, out=gx))],
         lambda r: G[r].double() @ W.double()),
        ("wgrad", [("library", lambda: torch.mm(G.t(), x)),
                   ("gemm_f32", lambda: _lib.gemm_f32_tn(G, x, out=gw, workspace=ws))],
         lambda r: G[:, r].double().t() @ x.double()),
    ]
    for op, routes, ref_fn in ops:
        r = rows if op != "wgrad" else torch.arange(0, N, max(1, N // 64), device=dev)[:64]
        ref = ref_fn(r)
        times = samples([f for _, f in routes], rounds)
        lib_q1 = quartiles(times[0])[0]
        for (name, f), t in zip(routes, times):
            q1, med, q3 = quartiles(t)
            got = f()[r]
            if name.startswith("wonly"):   # its own weight: d_wt * codes
                _, codes, _, _, d_wt, _ = next(w for w in wide if w[0] == name)
                err = rel_err(got, x[r].double() @ (d_wt.double() * codes.double()).t() + b.double())
            else:
                err = rel_err(got, ref)
            verdict = "" if name == "library" else ("win" if q3 < lib_q1 else "-")
            out(f"{tag:18s} {layer:4s} {op:5s} M={M:5d} N={N:4d} K={K:4d} {name:9s} {flops / med / 1e6:7.1f} TFLOP/s  "
                f"q1 {q1:8.1f} med {med:8.1f} q3 {q3:8.1f} us  rel err {err:.2e}  {verdict}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--models", default="vit_b,vit_l")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_f32_bench needs a GPU: nothing is timed without one")
    dev = torch.device("cuda:0")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # kept up to date line by line
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    out(f"gemm_f32 bench: {a.rounds} alternated samples per route, HIP events, {torch.cuda.get_device_name(0)}")
    for m in a.models.split(","):
        tag, M, D = MODELS[m]
        for layer, N, K in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", 4 * D, D), ("fc2", D, 4 * D)):
            bench_shape(dev, tag, layer, M, K, N, max(15, a.rounds), out)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
