"""A 4-bit W+A QuantizeLinear's forward with quant_layers.F6_GEMM on (qvit_quantize_act_f6 + qvit_gemm_f6: both
operands as FP6 E2M3 fields on v_mfma_f32_16x16x128_f8f6f4) against off (qvit_quantize_act_i8 + qvit_gemm), on the
qkv / proj / fc1 / fc2 shapes of ViT-B/16 and ViT-L/16 at M = 50432, 73856 and 197.

    python tools/gemm_f6_bench.py [--rounds 11] [--models vit_b,vit_l] [--out profiles/gemm_f6_bench.txt]

The method and the two tables are tools/gemm_a4_bench.py's (its samples / quartiles / row): `layer` is one layer call
under no_grad with the switch off against on, `gemm` the GEMM alone on codes made once, qvit_gemm (int8 codes, the
register image) against qvit_gemm_f6 (the same codes as FP6), into a preallocated output.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gemm_a4_bench import MODELS, ROWS, WA, row, samples  # noqa: E402
from quantized_vit_amd import _lib, quant_layers as ql  # noqa: E402


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
            ql.F6_GEMM = on
            with torch.no_grad():
                return layer(x)
        same = torch.equal(run(False), run(True))
        t_off, t_on = samples([lambda: run(False), lambda: run(True)], rounds)
        ql.F6_GEMM = False
        row(out, "layer", tag, name, M, N, K, t_off, t_on, same)

        codes = layer._act_codes(x, plan)
        f6 = _lib.quantize_act_f6(x, *plan.act_q, 0, torch.empty((M, plan.kpad // 4 * 3), dtype=torch.uint8,
                                                                  device=dev), plan.kpad)
        del x
        wimg, wfmt = plan.gemm_weights()
        tail = (plan.n, plan.npad, plan.d_act, plan.d_wt, plan.bias_pad, _lib.EPI_F32)
        y8, y6 = (torch.empty((M, _lib.round_up(N, 4)), dtype=torch.float32, device=dev) for _ in range(2))
        g8 = lambda: _lib.gemm(codes, M, plan.kpad, wimg, wfmt, *tail, y8)
        g6 = lambda: _lib.gemm_f6(f6, M, plan.kpad, plan.extra["w6f"], *tail, y6)
        same = torch.equal(g8(), g6())
        t_off, t_on = samples([g8, g6], rounds)
        row(out, "gemm", tag, name, M, N, K, t_off, t_on, same)
        del codes, f6, y8, y6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--models", default="vit_b,vit_l")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_f6_bench needs a GPU: nothing is timed without one")
    dev = torch.device("cuda:0")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:   # kept up to date line by line
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    out(f"gemm_f6 bench: {a.rounds} alternated samples per route, HIP events, {torch.cuda.get_device_name(0)}; "
        f"layer: off = qvit_quantize_act_i8 + qvit_gemm, on = qvit_quantize_act_f6 + qvit_gemm_f6; "
        f"gemm: off = qvit_gemm (QVIT_W4R), on = qvit_gemm_f6 (QVIT_W6F)")
    for m in a.models.split(","):
        tag, D = MODELS[m]
        for name, N, K in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", 4 * D, D), ("fc2", D, 4 * D)):
            bench_layer(dev, tag, name, K, N, a.rounds, out)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
