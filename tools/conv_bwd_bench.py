"""The backward GEMMs of one QuantizeConv2d on the integer path (W4 A8), per op and per route, each with the operand
preparation its route runs per backward:
  dgrad  hip  : qvit_gemm_wonly on the transposed weight codes (P = G2 @ d_wt k_w), then qvit_col2im_quant_backward
                (col2im + the activation quantizer's backward)
         torch: torch.nn.grad.conv2d_input on the cached fake-quant weight, then qvit_quant_backward over the image
  wgrad  hip  : qvit_im2col_quant_i8 (the forward's codes again) + qvit_gemm_wgrad
         torch: the fp32 fake quantizer over the image + torch.nn.grad.conv2d_weight
The output gradient is handed to each route in the layout it reads: the [B, OH OW, N] rows that arrive behind
PatchEmbed for the kernels, the NCHW copy torch's route makes of them for the library (that copy, made once per
backward and shared by both library ops, is timed on its own line). The fold kernel is also timed alone, against its
algorithmic traffic (P read once, x read once, grad_x written once). Routes alternated in one process, HIP events,
median of 20 after 3 warm-up rounds; peak memory from torch.cuda.max_memory_allocated above the operands.
Usage: python tools/conv_bwd_bench.py [--out profiles/conv_backward_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quantized_vit_amd import _lib, build  # noqa: E402
from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeConv2d  # noqa: E402

# (name, input shape, out channels, kernel, stride, padding)
LAYERS = [("ViT-B/16 b256 patch embed", (256, 3, 224, 224), 768, 16, 16, 0),
          ("ViT-L/16 @384 b128 patch embed", (128, 3, 384, 384), 1024, 16, 16, 0),
          ("ViT-H/14 b64 patch embed", (64, 3, 224, 224), 1280, 14, 14, 0),
          ("3x3 stride 1 64 -> 64 on 56 x 56 b32", (32, 64, 56, 56), 64, 3, 1, 1)]
REPS, WARM = 20, 3


def make_layer(dev, cin, cout, k, s, p):
    layer = QuantizeConv2d(cin, cout, k, stride=s, padding=p, bias=True, quant_type=QuantizationType.SYMMETRIC_LINEAR,
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
    assert plan.int_path and plan.wfmt == _lib.W4 and plan.has_codes
    return layer, plan


def ops(layer, plan, x, G_rows, G_nchw):
    shape = tuple(x.shape)
    w_q = layer.w_fakequant(plan).view_as(layer.weight)   # cached on the plan
    clip = layer.act_clip_val
    G_cl = G_rows.transpose(1, 2).reshape(G_nchw.shape[0], plan.n, *G_nchw.shape[2:])   # channels-last view
    assert G_cl.data_ptr() == G_rows.data_ptr()

    def torch_dgrad():
        g = layer._gemm_grads(plan, shape, None, w_q, G_nchw)[0]
        return _lib.quant_backward(x, g, plan.qtype, plan.d_act, plan.qm_act, plan.t_act, clip[0], clip[1], grad_x=g)

    def torch_wgrad():
        x_q = _lib.fake_quant_f32(x, plan.qtype, plan.d_act, plan.qm_act, plan.t_act)
        return layer._gemm_grads(plan, shape, x_q, None, G_nchw)[1]

    def hip_dgrad():
        return layer._gemm_grads_hip(plan, x, None, None, G_cl, True, False)

    def hip_wgrad():
        return layer._gemm_grads_hip(plan, x, None, None, G_cl, False, True)[1]

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


def median_ms(fn):
    t = [timed(fn) for _ in range(WARM + REPS)][WARM:]
    return statistics.median(t), min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    lines = [f"device: {torch.cuda.get_device_name(0)}; median of {REPS} (min in brackets), HIP events, routes "
             f"alternated in one process"]
    for name, xshape, cout, k, s, p in LAYERS:
        torch.manual_seed(0)
        layer, plan = make_layer(dev, xshape[1], cout, k, s, p)
        geometry = (layer.kernel_size, layer.stride, layer.padding, layer.dilation)
        x = torch.randn(xshape, device=dev)
        OH, OW = _lib.conv_out_hw(xshape[2], xshape[3], *geometry)
        M = xshape[0] * OH * OW
        G_rows = torch.randn(xshape[0], OH * OW, cout, device=dev)
        G_nchw = G_rows.transpose(1, 2).reshape(xshape[0], cout, OH, OW).contiguous()
        plan.packed_t()                            # packed once per parameter version, outside the timed region
        lines.append(f"{name}: x {xshape} k={k} s={s} p={p}   M={M} K={plan.k} N={cout}   "
                     f"P / image = {M * plan.k / x.numel():.2f}")
        for op, routes in ops(layer, plan, x, G_rows, G_nchw).items():
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
                             f"peak memory above operands {peak(fn) / 2**20:8.1f} MiB")
            lines.append(f"  {op} torch / hip = {med['torch'] / med['hip']:.2f}x")
        G_cl = G_rows.transpose(1, 2).reshape(G_nchw.shape)
        med, mn = median_ms(lambda: G_cl.contiguous())
        lines.append(f"  torch route only: NCHW copy of the output gradient {med:8.3f} ms [{mn:8.3f}] (once per backward)")
        # the fold kernel alone, buffers allocated outside
        P = torch.randn(M, plan.k, device=dev)
        out = torch.empty_like(x)
        nbytes = int(_lib.load().qvit_col2im_quant_backward_workspace_bytes(*xshape, *geometry[0], *geometry[1],
                                                                            *geometry[2], *geometry[3]))
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        traffic = 4 * (P.numel() + 2 * x.numel())
        for label, xin in (("fused", x), ("fold only", None)):
            qargs = (plan.qtype, plan.d_act, plan.qm_act, plan.t_act, *layer.act_clip_val) if xin is not None else ()
            med, mn = median_ms(lambda: _lib.col2im_quant_backward(P, xin, xshape, *geometry, *qargs, grad_x=out,
                                                                   workspace=ws if xin is not None else None))
            tr = traffic if xin is not None else traffic - 4 * x.numel()
            lines.append(f"  qvit_col2im_quant_backward {label:9s} {med:8.3f} ms [{mn:8.3f}]  algorithmic traffic "
                         f"{tr / 2**20:7.1f} MiB -> {tr / med / 1e9:6.2f} TB/s")
        del layer, plan, x, G_rows, G_nchw, G_cl, P, out, ws
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
