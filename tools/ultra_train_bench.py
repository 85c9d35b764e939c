"""UltraNet training step and its backward contractions: HIP route against the library route (QVIT_ULTRA_BWD=torch).

  python tools/ultra_train_bench.py [--batch 64] [--size 416] [--reps 20] [--out profiles/ultra_train_bench.txt]

Times (HIP events, median of --reps, the routes alternated in one process): forward + backward of
UltraNetQua.forward_modules in training mode on three routes (both contractions forced onto the HIP kernels at every
layer, i.e. the module's defaults ULTRA_BWD_DEFAULT_TORCH / DGRAD_HIP_MAX_PIXELS cleared; the default mix
QVIT_ULTRA_BWD=hip; the library, QVIT_ULTRA_BWD=torch), and for every Conv2d_Q layer at its shape in the network the weight
gradient (qvit_conv_wgrad against torch.nn.grad.conv2d_weight) and the input gradient (qvit_conv_wonly on the
transposed, flipped codes against torch.nn.grad.conv2d_input), each alone. Layer 0 reads the float image: it has
no code input and needs no input gradient, so it is not listed.

The fused BatchNorm2d -> quantizer -> max pool node (QVIT_ULTRA_TRAIN_FUSE): the default mix
with the flag on against the flag off (the routes alternated in the same way), torch.cuda.max_memory_allocated of
one step per route, and for each of the 8 blocks the chain alone at its shape in the network, forward + backward,
the three modules against bn_act_pool. --sections step,convs,chain selects what runs (default: all)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantized_vit_amd import _lib, quant_ultra as Q   # noqa: E402
from quantized_vit_amd.ultranet import UltraNetQua, _aten_batch_norm   # noqa: E402


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def _alternate(fns, reps):
    """Median ms of each fn, one repetition of each in turn."""
    for f in fns:
        _ms(f, 1)
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            ts[i] += _ms(f, 1)
    return [statistics.median(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sections", default="step,convs,chain")
    a = ap.parse_args()
    sections = set(a.sections.split(","))
    assert sections <= {"step", "convs", "chain"}, a.sections
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = UltraNetQua().to(dev).train()
    x = torch.rand(a.batch, 3, a.size, a.size, device=dev)
    lines = [f"UltraNet training, {a.size} x {a.size} b{a.batch}, median of {a.reps} (ms), {torch.cuda.get_device_name(0)}"]

    def step(route, force_all=False, fuse="0"):
        def run():
            prev = Q.ULTRA_BWD, Q.ULTRA_BWD_DEFAULT_TORCH, Q.DGRAD_HIP_MAX_PIXELS, Q.ULTRA_TRAIN_FUSE
            Q.ULTRA_BWD, Q.ULTRA_TRAIN_FUSE = route, fuse
            if force_all:
                Q.ULTRA_BWD_DEFAULT_TORCH, Q.DGRAD_HIP_MAX_PIXELS = (), 1 << 62
            try:
                model.zero_grad(set_to_none=True)
                model.forward_modules(x)[0].square().mean().backward()
            finally:
                Q.ULTRA_BWD, Q.ULTRA_BWD_DEFAULT_TORCH, Q.DGRAD_HIP_MAX_PIXELS, Q.ULTRA_TRAIN_FUSE = prev
        return run

    def peak_mib(fn):
        fn()
        torch.cuda.synchronize()
        model.zero_grad(set_to_none=True)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() / 2 ** 20, base / 2 ** 20

    if "step" in sections:
        both, dflt, lib, fused = _alternate([step("hip", True), step("hip"), step("torch"), step("hip", fuse="1")],
                                            a.reps)
        lines.append(f"forward_modules fwd+bwd: both ops on HIP {both:.3f} (x{lib / both:.2f})  default mix "
                     f"{dflt:.3f} (x{lib / dflt:.2f})  torch {lib:.3f}")
        lines.append(f"forward_modules fwd+bwd, default mix: QVIT_ULTRA_TRAIN_FUSE=0 {dflt:.3f}  =1 {fused:.3f} "
                     f"(x{dflt / fused:.2f})")
        (p0, b0), (p1, b1) = peak_mib(step("hip")), peak_mib(step("hip", fuse="1"))
        lines.append(f"max_memory_allocated of one step (MiB; {b0:.0f} allocated before it): "
                     f"QVIT_ULTRA_TRAIN_FUSE=0 {p0:.0f}  =1 {p1:.0f} (x{p0 / p1:.2f})")

    # each conv's operands at its place in the network
    convs = []
    with torch.no_grad(), _aten_batch_norm():
        h, levels = x, None
        for m in model.layers:
            if isinstance(m, torch.nn.Conv2d):
                convs.append((m, h, levels))
            h = m(h)
            if isinstance(m, Q.activation_quantize_fn):
                levels = 2 ** m.a_bit - 1
    if "convs" in sections:
        lines.append("layer (B, C, H, W -> N, k) | wgrad hip | wgrad torch | x | dgrad hip | dgrad torch | x")
    for m, h, levels in convs:
        if levels is None or "convs" not in sections:
            continue
        with torch.no_grad():
            G = torch.randn_like(m(h))
            wq = m.quantize_fn(m.weight)
        c = m._codes.get(m.weight, m.bias, m.w_bit)
        img, rows, npad_t, kpad_t = c.packed_t(m.weight)
        ks, st, pd, dl = m.kernel_size, m.stride, m.padding, m.dilation
        pad_t = tuple(d * (k - 1) - p for d, k, p in zip(dl, ks, pd))
        t = _alternate([
            lambda: _lib.conv_wgrad(G, h, ks, st, pd, dl, levels),
            lambda: torch.nn.grad.conv2d_weight(h, m.weight.shape, G, st, pd, dl, 1),
            lambda: _lib.conv_wonly(G, ks, st, pad_t, dl, img, c.wfmt, rows, npad_t, kpad_t, c.d_wt, None),
            lambda: torch.nn.grad.conv2d_input(h.shape, wq, G, st, pd, dl, 1)], a.reps)
        lines.append(f"{tuple(h.shape)} -> {m.out_channels}, {ks[0]} | {t[0]:.3f} | {t[1]:.3f} | {t[1] / t[0]:.2f} | "
                     f"{t[2]:.3f} | {t[3]:.3f} | {t[3] / t[2]:.2f}")
    if "chain" in sections:
        # each BatchNorm2d -> quantizer (-> max pool) run on its conv's output, forward + backward, alone
        lines.append("chain input (B, C, H, W), pool | modules fwd+bwd | fused fwd+bwd | x | modules peak MiB | "
                     "fused peak MiB")
        mods = list(model.layers)
        for i, bn in enumerate(mods):
            if not isinstance(bn, torch.nn.BatchNorm2d):
                continue
            act = mods[i + 1]
            pool = mods[i + 2] if i + 2 < len(mods) and isinstance(mods[i + 2], torch.nn.MaxPool2d) else None
            conv, hin, _ = next(c for c in convs if c[0] is mods[i - 1])
            with torch.no_grad():
                y = conv(hin).requires_grad_(True)
                G = torch.randn_like(act(y) if pool is None else pool(act(y)))

            def chain_modules():
                y.grad = None
                bn.zero_grad(set_to_none=True)
                with _aten_batch_norm():
                    o = act(bn(y))
                    o = o if pool is None else pool(o)
                o.backward(G)

            def chain_fused():
                y.grad = None
                bn.zero_grad(set_to_none=True)
                Q.bn_act_pool(y, bn, act, pool).backward(G)

            tm, tf = _alternate([chain_modules, chain_fused], a.reps)
            pm, pf = peak_mib(chain_modules)[0], peak_mib(chain_fused)[0]
            lines.append(f"{tuple(y.shape)}, {'pool' if pool is not None else 'no pool'} | {tm:.3f} | {tf:.3f} | "
                         f"{tm / tf:.2f} | {pm:.0f} | {pf:.0f}")
            del y, G
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
