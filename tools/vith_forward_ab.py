"""Times the W4A8 forward of vit_huge_patch14_224_in21k (embed 1280, 16 heads of 80, 257 tokens) under no_grad on its
two block routes, alternated in one process: the split route (qvit_gemm_qkv_split_hd -> qvit_attention_split with the
int8 epilogue) and the previous route (ViTAttention.split_ok forced off: fp32 qkv GEMM -> qvit_attention ->
proj's quantizer as a launch of its own). HIP events around a whole forward, the median of --iters after warm-up per
round, three rounds per route. --depth shortens the model (the blocks are alike)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quantized_vit_amd import _lib, calibrate, vit_model  # noqa: E402
from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType  # noqa: E402
from quantized_vit_amd.quant_model import model_to_quantize_model  # noqa: E402


@torch.no_grad()
def build(dev, depth):
    """calibrate.build_quantized_vit's recipe on the ViT-Huge/14 factory (W4 nonlinear t = 1, A8 calibrated)."""
    torch.manual_seed(0)
    model = vit_model.vit_huge_patch14_224_in21k(num_classes=1000, has_logits=False)
    if depth:
        del model.blocks[depth:]
    calibrate.redraw_init_artifacts(model)
    model = model.to(dev).eval()
    img = calibrate.synthetic_images(2, 224, seed=1, device=dev)
    absmax = calibrate.collect_input_absmax(model, img)
    model = model_to_quantize_model(model, num_bits=4, quant_type=QuantizationType.SYMMETRIC_NONLINEAR,
                                    quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    calibrate.set_activation_quant(model, absmax, bits=8, t=1.0)
    return model.eval()


def timeit(fn, iters):
    ts = []
    for _ in range(iters + 2):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        ts.append((s, e))
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ts[2:])
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--depth", type=int, default=0, help="keep only the first DEPTH blocks (0: all 32)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--lib", default="", help="load this library build instead (diagnostic variants)")
    a = ap.parse_args()
    if a.lib:
        _lib.load(a.lib)
    dev = torch.device("cuda:0")
    model = build(dev, a.depth)
    x = calibrate.synthetic_images(a.batch, 224, seed=1000, device=dev)
    real = vit_model.ViTAttention.split_ok
    calls = []
    real_split = _lib.attention_split

    def counted(*args, **kw):
        calls.append(args[5])
        return real_split(*args, **kw)

    def route(split):
        vit_model.ViTAttention.split_ok = real if split else (lambda self, p: False)

    def fwd():
        with torch.no_grad():
            return model(x)

    logits = {}
    for name, split in (("split route", True), ("previous route", False)):   # warm both, and check the routing
        route(split)
        _lib.attention_split = counted
        calls.clear()
        logits[name] = fwd().double()
        _lib.attention_split = real_split
        assert calls == ([80] * len(model.blocks) if split else []), (name, calls)
        timeit(fwd, 3)
    d = float((logits["split route"] - logits["previous route"]).abs().max()) / float(logits["previous route"].abs().max())
    times = {"split route": [], "previous route": []}
    for _ in range(3):
        for name, split in (("split route", True), ("previous route", False)):
            route(split)
            times[name].append(timeit(fwd, a.iters))
    route(True)
    med = {k: sorted(v)[1] for k, v in times.items()}
    for k, v in times.items():
        print(f"vit_huge_patch14_224_in21k W4A8 b{a.batch} depth {len(model.blocks)} {k:15s} {med[k]:9.3f} ms  "
              f"{a.batch / med[k] * 1e3:8.1f} img/s  rounds {' '.join(f'{t:.3f}' for t in v)}", flush=True)
    print(f"previous / split = {med['previous route'] / med['split route']:.4f}; logits distance between the routes "
          f"{d:.3e} (max |diff| / max |previous|)", flush=True)


if __name__ == "__main__":
    main()
