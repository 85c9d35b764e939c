"""One transformer Block forward + backward under autograd (W4 A8, the integer path), the modules route against the
TRAIN_FUSE route (quant_layers.layernorm_linear / gelu_linear: LayerNorm and GELU fused with the next layer's
quantizer, forward and backward), and the three new backward kernels alone against their algorithmic HBM bytes.
Routes alternated in one process, HIP events, median of 20 after 3 warm-up rounds; peak memory from
torch.cuda.max_memory_allocated above the block's parameters and input. The kernels' inputs are larger than the
256 MB last-level cache, so a timed call reads them from HBM.
Usage: python tools/block_train_bench.py [--out profiles/block_train_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quantized_vit_amd import _lib, build  # noqa: E402
from quantized_vit_amd import vit_model as vm  # noqa: E402
from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType  # noqa: E402
from quantized_vit_amd.quant_model import model_to_quantize_model  # noqa: E402

# (model, batch, tokens, embed dim, heads)
SHAPES = [("ViT-B/16 b256", 256, 197, 768, 12), ("ViT-L/16 @384 b128", 128, 577, 1024, 16)]
REPS, WARM = 20, 3


def make_block(dev, C, heads):
    torch.manual_seed(0)
    blk = vm.Block(C, heads, qkv_bias=True).to(dev)
    blk = model_to_quantize_model(blk, num_bits=4, quant_type=QuantizationType.SYMMETRIC_LINEAR,
                                  quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION).eval()
    with torch.no_grad():   # int8 activation codes over the range the block's activations take
        for l in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
            l.q_m_act.fill_(3.0)
            l.d_quant_act.fill_(3.0 / 127.3)
            l.invalidate()
            assert l.quant_plan().int_path
    return blk


def step(blk, x, G, fuse):
    vm.TRAIN_FUSE = fuse
    for p in blk.parameters():
        p.grad = None
    xin = x.detach().requires_grad_(True)
    y = blk(xin)
    y.backward(G)
    return xin.grad


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench_block(dev, name, B, N, C, heads, lines):
    blk = make_block(dev, C, heads)
    x = torch.randn(B, N, C, device=dev)
    G = torch.randn(B, N, C, device=dev)
    routes = (("modules", False), ("fused", True))
    times = {r: [] for r, _ in routes}
    for i in range(WARM + REPS):
        for r, fuse in routes:
            t = timed(lambda: step(blk, x, G, fuse))
            if i >= WARM:
                times[r].append(t)
    med = {r: statistics.median(v) for r, v in times.items()}
    mem = {r: peak(lambda: step(blk, x, G, fuse)) for r, fuse in routes}
    vm.TRAIN_FUSE = False
    for r, _ in routes:
        lines.append(f"{name} block fwd+bwd M={B * N} C={C} {r:8s}: median {med[r]:8.3f} ms "
                     f"(min {min(times[r]):.3f}, max {max(times[r]):.3f}), peak {mem[r]:9.1f} MiB")
    lines.append(f"{name} fused / modules: time {med['fused'] / med['modules']:.4f}, "
                 f"peak memory {mem['fused'] / mem['modules']:.4f}")
    del blk, x, G
    torch.cuda.empty_cache()


def bench_kernels(dev, name, M, C, lines):
    d = torch.tensor([3.0 / 127.3], device=dev)
    qm = torch.tensor([3.0], device=dev)
    H = 4 * C
    x, g = torch.randn(M, C, device=dev), torch.randn(M, C, device=dev)
    gam, bet = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    h, gh = torch.randn(M, H, device=dev), torch.randn(M, H, device=dev)
    out_c, out_h = torch.empty_like(g), torch.empty_like(gh)
    grid = min(1024, (M + 3) // 4)
    cases = [("layernorm_quant_backward", 3 * M * C * 4 + 2 * (grid * 2 * C * 4),
              lambda: _lib.layernorm_quant_backward(x, gam, bet, 1e-6, _lib.QT_LINEAR, d, qm, None, -2.0, 2.0, g,
                                                    grad_x=out_c)),
             ("quant_backward + torch LN bwd (modules)", None, None),
             ("gelu_quant_backward", 3 * M * H * 4,
              lambda: _lib.gelu_quant_backward(h, gh, _lib.QT_LINEAR, d, qm, None, -2.0, 2.0, grad_h=out_h)),
             ("quant_backward [M, 4C] (for scale)", 3 * M * H * 4,
              lambda: _lib.quant_backward(h, gh, _lib.QT_LINEAR, d, qm, None, -2.0, 2.0, grad_x=out_h))]
    for label, nbytes, fn in cases:
        if fn is None:
            continue
        ts = [timed(fn) for _ in range(WARM + REPS)][WARM:]
        t = statistics.median(ts)
        lines.append(f"{name} {label:36s} M={M}: median {t * 1e3:9.1f} us, {nbytes / 2 ** 20:8.1f} MiB algorithmic, "
                     f"{nbytes / t / 1e6:7.1f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    lines = [f"block_train_bench: {torch.cuda.get_device_name(0)}, lib {_lib.build_id()}, torch {torch.__version__}; "
             f"median of {REPS} after {WARM} warm-up rounds, routes alternated, HIP events"]
    for name, B, N, C, heads in SHAPES:
        bench_block(dev, name, B, N, C, heads, lines)
    for name, B, N, C, heads in SHAPES:
        bench_kernels(dev, name, B * N, C, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
