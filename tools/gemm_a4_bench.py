"""A 4-bit W+A QuantizeLinear's forward with quant_layers.A4_GEMM on (qvit_quantize_act_i4 + qvit_gemm_a4: packed
nibble activation codes) against off (qvit_quantize_act_i8 + qvit_gemm), on the qkv / proj / fc1 / fc2 shapes of
ViT-B/16 and ViT-L/16 at M = 50432, 73856 and 197.

    python tools/gemm_a4_bench.py [--rounds 11] [--models vit_b,vit_l] [--out profiles/gemm_a4_bench.txt]

Two tables, because the quantizer reads the fp32 input on either route and would hide the GEMM's change:
  layer  one layer call under no_grad (quantizer + GEMM), switch off against on;
  gemm   the GEMM alone on codes made once, qvit_gemm (int8 codes) against qvit_gemm_a4 (the same codes packed), into a
         preallocated output.
Each sample lies between two HIP events on the launch stream; the two routes alternate sample by sample inside one
process after both were warmed up. A row reports each route's median and quartiles in microseconds, off / on of the
medians, `win` where the new route's upper quartile lies below the old route's lower quartile, `lose` for the reverse,
`level` otherwise, and whether the two outputs are the same bytes.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantized_vit_amd import _lib, quant_layers as ql  # noqa: E402

MODELS = {"vit_b": ("ViT-B/16", 768), "vit_l": ("ViT-L/16", 1024)}
ROWS = (50432, 73856, 197)
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


def row(out, what, tag, name, M, N, K, t_off, t_on, same):
    (a1, am, a3), (b1, bm, b3) = quartiles(t_off), quartiles(t_on)
    verdict = "win" if b3 < a1 else ("lose" if b1 > a3 else "level")
    out(f"{what:5s} {tag:9s} {name:4s} M={M:5d} N={N:4d} K={K:4d}  off q1 {a1:8.1f} med {am:8.1f} q3 {a3:8.1f} us  "
        f"on q1 {b1:8.1f} med {bm:8.1f} q3 {b3:8.1f} us  off/on {am / bm:5.2f}  {verdict:5s}  "
        f"{'same bytes' if same else 'DIFFERENT'}")


def bench_layer(dev, tag, name, K, N, rounds, out):
    torch.manual_seed(K + N)
    layer = ql.QuantizeLinear(K, N, quant_mode=WA).to(dev)
    ql.initialize_quant_layer(layer, num_bits=4, quant_mode=WA)
    layer.eval()
    plan = layer.quant_plan()
    qm = float(layer.q_m_act.detach())
    for M in ROWS:
        x = 0.4 * qm * torch.randn(M, K, device=dev)   # a few saturate

        def run(on):
            ql.A4_GEMM = on
            with torch.no_grad():
                return layer(x)
        same = torch.equal(run(False), run(True))
        t_off, t_on = samples([lambda: run(False), lambda: run(True)], rounds)
        ql.A4_GEMM = False
        row(out, "layer", tag, name, M, N, K, t_off, t_on, same)

        codes = layer._act_codes(x, plan)
        packed = _lib.quantize_act_i4(x, *plan.act_q, 0, torch.empty((M, plan.kpad // 2), dtype=torch.uint8,
                                                                   device=dev), plan.kpad)
        del x
        wimg, wfmt = plan.gemm_weights()
        tail = (M, plan.kpad, wimg, wfmt, plan.n, plan.npad, plan.d_act, plan.d_wt, plan.bias_pad, _lib.EPI_F32)
        y8, y4 = (torch.empty((M, _lib.round_up(N, 4)), dtype=torch.float32, device=dev) for _ in range(2))
        g8, g4 = (lambda: _lib.gemm(codes, *tail, y8)), (lambda: _lib.gemm_a4(packed, *tail, y4))
        same = torch.equal(g8(), g4())
        t_off, t_on = samples([g8, g4], rounds)
        row(out, "gemm", tag, name, M, N, K, t_off, t_on, same)
        del codes, packed, y8, y4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--models", default="vit_b,vit_l")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_a4_bench needs a GPU: nothing is timed without one")
    dev = torch.device("cuda:0")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # kept up to date line by line
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    out(f"gemm_a4 bench: {a.rounds} alternated samples per route, HIP events, {torch.cuda.get_device_name(0)}; "
        f"layer: off = qvit_quantize_act_i8 + qvit_gemm, on = qvit_quantize_act_i4 + qvit_gemm_a4; "
        f"gemm: off = qvit_gemm, on = qvit_gemm_a4, 4-bit weights (QVIT_W4R)")
    for m in a.models.split(","):
        tag, D = MODELS[m]
        for name, N, K in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", 4 * D, D), ("fc2", D, 4 * D)):
            bench_layer(dev, tag, name, K, N, a.rounds, out)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
