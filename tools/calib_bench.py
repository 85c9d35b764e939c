"""One qvit_quant_error call against the torch loop it replaces in a clip search over 32 candidates:
  hip   : _lib.quant_error(x, ...) into preallocated err / nclip (two launches; x read once per block of 16 candidates)
  torch : for each candidate, _lib.fake_quant_f32 and (x - fq).double().square().sum() (no clip count)
at the fc1 and fc2 input shapes of ViT-B/16 b256 and at the fc1 weight, both quantizer types (nonlinear at t = 0.9).
GB/s counts what the kernel has to read: x once per candidate block (2 blocks for 32 candidates). Routes alternated in
one process, HIP events, median of 20 after 3 warm-up rounds.
Usage: python tools/calib_bench.py [--out profiles/quant_error_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quantized_vit_amd import _lib, build, calibrate  # noqa: E402

SHAPES = [("fc1 input  [50432, 768]", (50432, 768), 8), ("fc2 input  [50432, 3072]", (50432, 3072), 8),
          ("fc1 weight [3072, 768]", (3072, 768), 4)]
QTYPES = [("linear", _lib.QT_LINEAR, 1.0), ("nonlinear t=0.9", _lib.QT_NONLINEAR, 0.9)]
NUM, CAND_BLOCK = 32, 16
REPS, WARM = 20, 3


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
    lines = [f"device: {torch.cuda.get_device_name(0)}; {NUM} candidates; median of {REPS} (min in brackets), HIP events, "
             f"routes alternated in one process; GB/s = 4 bytes x numel x {NUM // CAND_BLOCK} candidate blocks / time"]
    for name, shape, bits in SHAPES:
        g = torch.Generator().manual_seed(0)
        x = torch.randn(shape, generator=g)
        x = (x * (0.02 if "weight" in name else 1.0)).to(dev)
        absmax = float(x.abs().max())
        for qname, qtype, t in QTYPES:
            q_m, d = calibrate.clip_candidates(absmax, bits, t, NUM)
            q_m, d = q_m.to(dev), d.to(dev)
            td = torch.tensor([t], dtype=torch.float32, device=dev) if qtype == _lib.QT_NONLINEAR else None
            err = torch.empty(NUM, dtype=torch.float64, device=dev)
            nclip = torch.empty(NUM, dtype=torch.int64, device=dev)
            terr = torch.empty(NUM, dtype=torch.float64, device=dev)

            def hip():
                _lib.quant_error(x, qtype, d, q_m, td, err, nclip)

            def loop():
                for c in range(NUM):
                    fq = _lib.fake_quant_f32(x, qtype, d[c:c + 1], q_m[c:c + 1], td)
                    terr[c] = (x - fq).double().square().sum()

            res = alternated([("hip", hip), ("torch", loop)])
            # the two routes agree, up to the loop's fp32 subtraction (the nonlinear kernel scores against
            # sign(x) |x|^t, the loop against x: linear only)
            if qtype == _lib.QT_LINEAR:
                assert float(((err - terr).abs() / terr).max()) < 1e-6
            nbytes = 4 * x.numel() * (NUM // CAND_BLOCK)
            (hm, hn), (tm, tn) = res["hip"], res["torch"]
            lines.append(f"{name} b{bits} {qname:16s} hip {hm * 1e3:9.1f} us [{hn * 1e3:9.1f}] {nbytes / hm / 1e6:7.1f} "
                         f"GB/s   torch loop {tm * 1e3:10.1f} us [{tn * 1e3:10.1f}]   torch / hip = {tm / hm:6.1f}x   "
                         f"argmin {int(err.argmin())}")
        del x
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
