"""Times qvit_quant_backward with HIP events at fc1's activation shape (50432 x 768, ViT-B/16 at batch 256) and
at a weight shape (3072 x 768), linear and nonlinear, against torch.mul(x, g, out=gx) on the same tensors (the
same three streams of HBM traffic: two reads, one write). Warm-up, then the median of 20 runs.

Usage: python tools/quant_bwd_bench.py [--out profiles/quant_backward_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from quantized_vit_amd import _lib  # noqa: E402

SHAPES = [("fc1 activation", 50432, 768), ("weight", 3072, 768)]
RUNS, WARMUP = 20, 5


def median_ms(fn) -> float:
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_backward_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    d = torch.tensor([0.02], device=dev)
    qm = torch.tensor([2.545], device=dev)
    t = torch.tensor([0.9], device=dev)
    lines = [f"qvit_quant_backward vs torch.mul(x, g, out=gx); median of {RUNS} runs after {WARMUP} warm-ups; "
             f"{torch.cuda.get_device_name(dev)}; library {_lib.build_id()}",
             f"{'shape':<28}{'kernel':<12}{'ms':>9}{'GB/s':>9}{'vs mul':>9}"]
    for name, rows, cols in SHAPES:
        n = rows * cols
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(n, device=dev, generator=gen)
        g = torch.randn(n, device=dev, generator=gen)
        gx = torch.empty_like(x)
        scal = torch.empty(3, device=dev)
        nbytes = lib.qvit_quant_backward_workspace_bytes(n)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        traffic = 3 * 4 * n   # read x, read g, write gx

        def backward(qtype, tq):
            _lib._check(lib.qvit_quant_backward(x.data_ptr(), g.data_ptr(), n, qtype, d.data_ptr(), qm.data_ptr(),
                                                None if tq is None else tq.data_ptr(), -2.0, 2.0, 0.0,
                                                gx.data_ptr(), scal.data_ptr(), ws.data_ptr(), nbytes, stream),
                        "qvit_quant_backward")

        mul = median_ms(lambda: torch.mul(x, g, out=gx))
        rowsout = [("torch.mul", mul)]
        rowsout.append(("linear", median_ms(lambda: backward(_lib.QT_LINEAR, None))))
        rowsout.append(("nonlinear", median_ms(lambda: backward(_lib.QT_NONLINEAR, t))))
        for kern, ms in rowsout:
            lines.append(f"{name + f' {rows}x{cols}':<28}{kern:<12}{ms:>9.4f}{traffic / ms / 1e6:>9.0f}"
                         f"{ms / mul:>9.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
