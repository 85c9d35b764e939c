"""The backward GEMMs of one QuantizeLinear on the integer path (W4 A8): dgrad (grad_out @ quantize_weight(W)) and
wgrad (grad_out^T @ quantize_act(x)), the HIP route (qvit_gemm_wonly on the transposed codes; the activation
quantizer to int8 codes + qvit_gemm_wgrad) against the torch route (torch.mm on the cached fake-quant weight; the
fp32 fake quantizer + torch.mm), each with the operand preparation its route runs per backward. Routes alternated
in one process, HIP events, median of 20 after 3 warm-up rounds; TFLOP/s are fp32-equivalent (2 M N K / time);
peak memory from torch.cuda.max_memory_allocated above the operands.
Usage: python tools/layer_bwd_bench.py [--out profiles/layer_backward_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quantized_vit_amd import _lib, build  # noqa: E402
from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeLinear  # noqa: E402

# (model, layer, M, K = in-features, N = out-features)
SHAPES = [("ViT-B/16 b256", "qkv", 256 * 197, 768, 2304), ("ViT-B/16 b256", "proj", 256 * 197, 768, 768),
          ("ViT-B/16 b256", "fc1", 256 * 197, 768, 3072), ("ViT-B/16 b256", "fc2", 256 * 197, 3072, 768),
          ("ViT-L/16 @384 b128", "qkv", 128 * 577, 1024, 3072), ("ViT-L/16 @384 b128", "proj", 128 * 577, 1024, 1024),
          ("ViT-L/16 @384 b128", "fc1", 128 * 577, 1024, 4096), ("ViT-L/16 @384 b128", "fc2", 128 * 577, 4096, 1024)]
REPS, WARM = 20, 3


def make_layer(dev, K, N):
    layer = QuantizeLinear(K, N, bias=True, quant_type=QuantizationType.SYMMETRIC_LINEAR,
                           quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION).to(dev).eval()
    with torch.no_grad():
        layer.weight.normal_(0.0, 0.02)
        wmax = float(layer.weight.abs().max())
        layer.q_m_wt.fill_(wmax)
        layer.d_quant_wt.fill_(wmax / 7.3)         # levels 7: int4 weight codes
        layer.q_m_act.fill_(3.0)
        layer.d_quant_act.fill_(3.0 / 127.3)       # levels 127: int8 activation codes
    layer.invalidate()
    plan = layer.quant_plan()
    assert plan.int_path and plan.wfmt == _lib.W4
    return layer, plan


def ops(layer, plan, x, G):
    shape = tuple(x.shape)
    w_q = layer.w_fakequant(plan)                  # cached on the plan by both the parent's route and this one

    def torch_dgrad():
        return layer._gemm_grads(plan, shape, None, w_q, G)[0]

    def torch_wgrad():
        x_q = _lib.fake_quant_f32(x, plan.qtype, plan.d_act, plan.qm_act, plan.t_act)
        return layer._gemm_grads(plan, shape, x_q, None, G)[1]

    def hip_dgrad():
        return layer._gemm_grads_hip(plan, x, None, None, G, True, False)[0]

    def hip_wgrad():
        return layer._gemm_grads_hip(plan, x, None, None, G, False, True)[1]

    return {"dgrad": (("hip", hip_dgrad), ("torch", torch_dgrad)), "wgrad": (("hip", hip_wgrad), ("torch", torch_wgrad))}


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
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    lines = [f"device: {torch.cuda.get_device_name(0)}; median of {REPS} (min in brackets), HIP events, routes "
             f"alternated in one process; TFLOP/s fp32-equivalent = 2 M N K / time"]
    for model, name, M, K, N in SHAPES:
        torch.manual_seed(0)
        layer, plan = make_layer(dev, K, N)
        x = torch.randn(M, K, device=dev)
        G = torch.randn(M, N, device=dev)
        plan.packed_t()                            # packed once per parameter version, outside the timed region
        lines.append(f"{model} {name}: M={M} K={K} N={N}   wgrad splits {_lib.gemm_wgrad_splits(M, N, K)}")
        for op, routes in ops(layer, plan, x, G).items():
            t = {key: [] for key, _ in routes}
            for r in range(WARM + REPS):
                for key, fn in routes:
                    ms = timed(fn)
                    if r >= WARM:
                        t[key].append(ms)
            med = {}
            for key, fn in routes:
                med[key] = statistics.median(t[key])
                lines.append(f"  {op} {key:5s} {med[key]:8.3f} ms [{min(t[key]):8.3f}]  "
                             f"{2.0 * M * N * K / med[key] / 1e9:7.1f} TFLOP/s  "
                             f"peak memory above operands {peak(fn) / 2**20:8.1f} MiB")
            lines.append(f"  {op} torch / hip = {med['torch'] / med['hip']:.2f}x")
        del layer, plan, x, G
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
