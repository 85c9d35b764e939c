"""QuantizeLinear's forward in W+A mode with 12- and 16-bit activations: quant_layers.A16_GEMM on
(qvit_quantize_act_i16 + qvit_gemm_a16) against off (qvit_fake_quant_f32 + qvit_gemm_wonly), on the qkv / proj / fc1 /
fc2 shapes of ViT-B/16 (M = 50432) and ViT-L/16 @384 (M = 73856) and at M = 197, for (weight / activation) bits
8 / 12, 12 / 12 and 16 / 16.

    python tools/gemm_a16_bench.py [--rounds 11] [--models vit_b,vit_l] [--out profiles/gemm_a16_bench.txt]

Each sample is one layer call under no_grad between two HIP events on the launch stream; the two routes alternate
sample by sample inside one process after both were warmed up. A row reports each route's median and quartiles in
microseconds, off / on of the medians, `win` where the new route's upper quartile lies below the old route's lower
quartile, `lose` for the reverse, `level` otherwise, and the largest difference of the two outputs over the largest
output (the old route is an fp32 GEMM of the same codes, the new one exact).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantized_vit_amd import quant_layers as ql  # noqa: E402

MODELS = {"vit_b": ("ViT-B/16", 50432, 768), "vit_l": ("ViT-L/16@384", 73856, 1024)}
BITS = [(8, 12), (12, 12), (16, 16)]
WA = ql.QuantizationMode.WEIGHT_AND_ACTIVATION


def samples(fns, rounds):
    """Per-call microseconds of each fn, `rounds` sorted samples each, alternating the fns sample by sample."""
    for f in fns:
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


def bench_layer(dev, tag, name, K, N, wbits, abits, Ms, rounds, out):
    torch.manual_seed(K + N + wbits)
    layer = ql.QuantizeLinear(K, N, quant_mode=WA).to(dev)
    ql.initialize_quant_layer(layer, num_bits=wbits, quant_mode=WA)
    with torch.no_grad():
        layer.d_quant_act.copy_(layer.q_m_act / (2 ** (abits - 1) - 1))
    layer.invalidate()
    layer.eval()
    qm = float(layer.q_m_act.detach())
    wfmt = layer.quant_plan().wfmt
    for M in Ms:
        x = 0.4 * qm * torch.randn(M, K, device=dev)   # a few saturate

        def run(on):
            ql.A16_GEMM = on
            with torch.no_grad():
                return layer(x)
        y_off, y_on = run(False), run(True)
        diff = float((y_on - y_off).abs().max() / y_off.abs().max())
        del y_off, y_on
        t_off, t_on = samples([lambda: run(False), lambda: run(True)], rounds)
        (a1, am, a3), (b1, bm, b3) = quartiles(t_off), quartiles(t_on)
        verdict = "win" if b3 < a1 else ("lose" if b1 > a3 else "level")
        out(f"{tag:13s} {name:4s} W{wbits:<2d}A{abits:<2d} wfmt {wfmt:2d} M={M:5d} N={N:4d} K={K:4d}  "
            f"off q1 {a1:8.1f} med {am:8.1f} q3 {a3:8.1f} us  on q1 {b1:8.1f} med {bm:8.1f} q3 {b3:8.1f} us  "
            f"off/on {am / bm:5.2f}  {verdict:5s}  max diff {diff:.1e}")
        del x
    ql.A16_GEMM = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--models", default="vit_b,vit_l")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_a16_bench needs a GPU: nothing is timed without one")
    dev = torch.device("cuda:0")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # kept up to date line by line
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    out(f"gemm_a16 bench: layer forward, {a.rounds} alternated samples per route, HIP events, "
        f"{torch.cuda.get_device_name(0)}; off = qvit_fake_quant_f32 + qvit_gemm_wonly, on = qvit_quantize_act_i16 + "
        f"qvit_gemm_a16")
    for m in a.models.split(","):
        tag, M, D = MODELS[m]
        for name, N, K in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", 4 * D, D), ("fc2", D, 4 * D)):
            for wbits, abits in BITS:
                bench_layer(dev, tag, name, K, N, wbits, abits, (M, 197), a.rounds, out)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
