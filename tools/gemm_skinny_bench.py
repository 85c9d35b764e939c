"""qvit_gemm against qvit_gemm_skinny on the proj / fc1 / fc2 shapes of ViT-B and ViT-L at small row counts, and the
whole ViT-B forward at b1 and b8 with quant_layers.GEMM_SKINNY off and on.

    python tools/gemm_skinny_bench.py [--rounds 15] [--batch 20] [--out profiles/gemm_skinny_bench.txt] [--no-model]

Each sample is `--batch` back-to-back launches between two HIP events on the launch stream (a single launch of
10 us is below what an event pair resolves), divided by the batch; the two paths alternate sample by sample inside
one process, and each row reports both medians, the spread of each (the interquartile range over the rounds, as a
share of the median), the S the automatic split chose, and `win` where the skinny path's upper quartile lies below
qvit_gemm's lower quartile (a difference larger than the run-to-run spread of this file). The last line names the
largest M at which every layer shape wins. Random full-range codes; the int4 layers on the QVIT_W4R image.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantized_vit_amd import _lib, quant_layers  # noqa: E402

MS = (197, 256, 788, 1576, 3152)


def p(v, dev):
    return torch.tensor([float(v)], device=dev)


def samples(fns, rounds, batch):
    """Per-call microseconds of each fn, `rounds` samples each, alternating the fns sample by sample."""
    for f in fns:          # warm-up: code objects, the workspace
        for _ in range(3):
            f()
    ev = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(batch):
                f()
            e.record()
            ev[i].append((s, e))
    torch.cuda.synchronize()
    return [sorted(s.elapsed_time(e) * 1e3 / batch for s, e in row) for row in ev]


def quartiles(v):
    """(lower quartile, median, upper quartile) of sorted samples."""
    return v[len(v) // 4], v[len(v) // 2], v[(3 * len(v)) // 4]


def layer_rows(dev, rounds, batch, out):
    qt = _lib.QT_NONLINEAR
    kw = dict(out_qtype=qt, out_d=p(4.0 / 127, dev), out_qm=p(4.0, dev), out_t=p(1.0, dev))
    geo = quant_layers.epilogue_table_geometry(qt, 4.0 / 127, 4.0, 1.0,
                                               quant_layers.saturation_level(qt, 4.0 / 127, 4.0, 1.0), True)
    table = _lib.epi_table_build(_lib.EPI_I8_GELU, qt, kw["out_d"], kw["out_qm"], kw["out_t"], 0, *geo, dev)
    d_a, d_w = p(1 / 127, dev), p(0.05 / 7, dev)
    out(f"{'model':6s} {'layer':5s} {'M':>5s} {'N':>5s} {'K':>5s} {'S':>3s} {'gemm us':>9s} {'iqr%':>5s} "
        f"{'skinny us':>9s} {'iqr%':>5s} {'skinny/gemm':>11s} win")
    wins = {M: True for M in MS}
    for model, D in (("vit_b", 768), ("vit_l", 1024)):
        for layer, N, K, epi in (("proj", D, D, _lib.EPI_F32_RESID), ("fc1", 4 * D, D, _lib.EPI_I8_GELU),
                                 ("fc2", D, 4 * D, _lib.EPI_F32_RESID)):
            packed = torch.randint(0, 256, (N * K // 2,), dtype=torch.uint8, device=dev)   # npad == N
            bias = torch.randn(N, device=dev) * 0.01
            for M in MS:
                A = torch.randint(-127, 128, (M, K), dtype=torch.int8, device=dev)
                i8 = epi == _lib.EPI_I8_GELU
                C = torch.zeros((M, N), dtype=torch.int8 if i8 else torch.float32, device=dev)
                args = (A, M, K, packed, _lib.W4R, N, N, d_a, d_w, bias, epi, C)
                ekw = dict(kw, epi_table=table) if i8 else {}
                nbytes = _lib.gemm_skinny_workspace_bytes(M, K, N)
                S = 1 if nbytes == 0 else (nbytes - 65536) // (((M + 63) // 64) * (N // 64) * 16384)
                g, s = samples([lambda: _lib.gemm(*args, **ekw), lambda: _lib.gemm_skinny(*args, **ekw)], rounds, batch)
                (g1, mg, g3), (s1, ms, s3) = quartiles(g), quartiles(s)
                wins[M] &= s3 < g1
                out(f"{model:6s} {layer:5s} {M:5d} {N:5d} {K:5d} {S:3d} {mg:9.2f} {100 * (g3 - g1) / mg:5.1f} "
                    f"{ms:9.2f} {100 * (s3 - s1) / ms:5.1f} {ms / mg:11.3f} {'win' if s3 < g1 else '-'}")
    allwin = [M for M in MS if wins[M]]
    out(f"largest M at which every layer shape wins: {max(allwin) if allwin else 'none'}"
        f" (all of {', '.join(map(str, allwin)) or 'none'})")


def model_rows(dev, rounds, out):
    from quantized_vit_amd.calibrate import build_quantized_vit, synthetic_images
    model = build_quantized_vit("vit_base_patch16_224", seed=0).to(dev).eval()
    saved = quant_layers.GEMM_SKINNY, quant_layers.GEMM_SKINNY_MAX_M
    out(f"\nvit_base_patch16_224 forward, GEMM_SKINNY off / on (GEMM_SKINNY_MAX_M = {saved[1]}, then 4096)")
    try:
        for B in (1, 8):
            img = synthetic_images(B, 224, seed=1).to(dev)

            def fwd(on, max_m):
                def f():
                    quant_layers.GEMM_SKINNY, quant_layers.GEMM_SKINNY_MAX_M = on, max_m
                    with torch.no_grad():
                        model(img)
                return f
            off, on, on_all = samples([fwd(False, saved[1]), fwd(True, saved[1]), fwd(True, 4096)], rounds, 3)
            (a1, ma, a3), (b1, mb, b3), (c1, mc, c3) = quartiles(off), quartiles(on), quartiles(on_all)
            out(f"b{B}: off {ma:9.1f} us (iqr {100 * (a3 - a1) / ma:.1f} %)   on {mb:9.1f} us (iqr "
                f"{100 * (b3 - b1) / mb:.1f} %)   on, every M {mc:9.1f} us (iqr {100 * (c3 - c1) / mc:.1f} %)")
    finally:
        quant_layers.GEMM_SKINNY, quant_layers.GEMM_SKINNY_MAX_M = saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_skinny_bench needs a GPU: nothing is timed without one")
    dev = torch.device("cuda:0")
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    layer_rows(dev, a.rounds, a.batch, out)
    if not a.no_model:
        model_rows(dev, a.rounds, out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
