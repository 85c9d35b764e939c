"""The patch embedding's input step from a uint8 image against the fp32 route, kernels alone (buffers allocated
outside the timed region):
  fp32      : qvit_im2col_quant_i8 on the normalised fp32 NCHW image (the route without set_uint8_input)
  u8 nchw   : qvit_im2col_u8_i8 on contiguous bytes
  u8 nhwc   : qvit_im2col_u8_i8 on channels_last bytes (a decoder's [B, H, W, C])
  normalize : qvit_u8_normalize_f32 (what the routes off the integer path run first)
with the algorithmic traffic of each (image read once, output written once) as GB/s, and, for information, the time
to copy one batch from pinned host memory as uint8 and as fp32. Routes alternated in one process, HIP events, median
of 20 after 3 warm-up rounds.
Usage: python tools/u8_input_bench.py [--out profiles/u8_input_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quantized_vit_amd import _lib, build  # noqa: E402

# (name, image shape, patch)
SHAPES = [("ViT-B/16 b256", (256, 3, 224, 224), 16),
          ("ViT-L/16 @384 b128", (128, 3, 384, 384), 16),
          ("ViT-H/14 b64 (scalar arm)", (64, 3, 224, 224), 14)]
REPS, WARM = 20, 3
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternated(routes):
    t = {key: [] for key, _ in routes}
    for r in range(WARM + REPS):
        for key, fn in routes:
            ms = timed(fn)
            if r >= WARM:
                t[key].append(ms)
    return {key: (statistics.median(v), min(v)) for key, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    build.build()
    dev = torch.device("cuda:0")
    scal = lambda v: torch.tensor([v], dtype=torch.float32, device=dev)
    q = (_lib.QT_LINEAR, scal(2.64 / 127), scal(2.64), None, 0)
    mean, std = torch.tensor(MEAN), torch.tensor(STD)
    V = ((torch.arange(256, dtype=torch.float32).div(255)[None, :] - mean[:, None]) / std[:, None]).contiguous().to(dev)
    T = torch.empty((3, 256), dtype=torch.int8, device=dev)
    _lib.quantize_act_i8(V, *q, T, 256)
    lines = [f"device: {torch.cuda.get_device_name(0)}; median of {REPS} (min in brackets), HIP events, routes "
             f"alternated in one process; GB/s = image bytes read once + output bytes written once"]
    for name, shape, k in SHAPES:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(0)
        img = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        x_nchw = img.to(dev)
        x_nhwc = img.permute(0, 2, 3, 1).contiguous().to(dev).permute(0, 3, 1, 2)
        x32 = _lib.u8_normalize_f32(x_nchw, V)
        OH, OW = _lib.conv_out_hw(H, W, (k, k), (k, k), (0, 0), (1, 1))
        K = C * k * k
        kpad = (K + _lib.TILE_K - 1) // _lib.TILE_K * _lib.TILE_K
        rows = B * OH * OW
        codes = torch.empty((rows, kpad), dtype=torch.int8, device=dev)
        ref = torch.empty_like(codes)
        out32 = torch.empty(shape, dtype=torch.float32, device=dev)
        geo = (k, k, k, k, 0, 0, 1, 1)
        n = img.numel()
        lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream

        def normalize():   # the entry point itself, into a buffer allocated outside
            _lib._check(lib.qvit_u8_normalize_f32(x_nhwc.data_ptr(), B, C, H, W, _lib.U8_NHWC, V.data_ptr(),
                                                  out32.data_ptr(), stream), "qvit_u8_normalize_f32")

        routes = [("fp32", lambda: _lib.im2col_quant_i8(x32, *geo, *q, ref, kpad)),
                  ("u8 nchw", lambda: _lib.im2col_u8_i8(x_nchw, *geo, T, codes, kpad)),
                  ("u8 nhwc", lambda: _lib.im2col_u8_i8(x_nhwc, *geo, T, codes, kpad)),
                  ("normalize", normalize)]
        traffic = {"fp32": 4 * n + rows * kpad, "u8 nchw": n + rows * kpad, "u8 nhwc": n + rows * kpad,
                   "normalize": n + 4 * n}
        res = alternated(routes)
        # the three im2col routes wrote the same codes
        _lib.im2col_u8_i8(x_nchw, *geo, T, codes, kpad)
        assert torch.equal(codes, ref)
        _lib.im2col_u8_i8(x_nhwc, *geo, T, codes, kpad)
        assert torch.equal(codes, ref) and torch.equal(out32, x32)
        lines.append(f"{name}: image {shape} patch {k}   rows={rows} K={K} kpad={kpad}")
        for key, _ in routes:
            med, mn = res[key]
            lines.append(f"  {key:10s} {med * 1e3:8.1f} us [{mn * 1e3:8.1f}]  {traffic[key] / 2**20:7.1f} MiB -> "
                         f"{traffic[key] / med / 1e6:7.1f} GB/s")
        lines.append(f"  fp32 / u8 nchw = {res['fp32'][0] / res['u8 nchw'][0]:.2f}x   "
                     f"fp32 / u8 nhwc = {res['fp32'][0] / res['u8 nhwc'][0]:.2f}x")
        # for information: one batch from pinned host memory
        h8, h32 = img.pin_memory(), x32.cpu().pin_memory()
        d8, d32 = torch.empty_like(x_nchw), torch.empty_like(x32)
        res = alternated([("copy u8", lambda: d8.copy_(h8, non_blocking=True)),
                          ("copy fp32", lambda: d32.copy_(h32, non_blocking=True))])
        for key, nbytes in (("copy u8", n), ("copy fp32", 4 * n)):
            med, mn = res[key]
            lines.append(f"  {key:10s} {med * 1e3:8.1f} us [{mn * 1e3:8.1f}]  {nbytes / 2**20:7.1f} MiB -> "
                         f"{nbytes / med / 1e6:7.1f} GB/s  (pinned host -> device, for information)")
        del x_nchw, x_nhwc, x32, codes, ref, out32, h8, h32, d8, d32
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
