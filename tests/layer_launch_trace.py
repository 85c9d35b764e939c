"""Launch recorder for the layer modules (a helper, not a test; the pattern of tests/fused_block_trace.py).

run_case(dev, name) builds the case's layer afresh from a fixed CPU seed with constant quantizer scalars, replaces the
`_lib` wrappers in WRAPPERS by recorders, runs the forward and (where the case says so) the backward, and returns
    {"launches": [[wrapper, {parameter: value}], ...], "tensors": {name: {"dtype", "shape", "bits" | "sha256"}}, "outcome": ...}
Arguments are bound to the wrapper's own signature (defaults applied). A tensor is recorded as
"dtype[shape](strides)", with its value when it holds one element (the quantizer scalars, the overflow word) and
"|unaligned" when its base address is no multiple of 16; never the address itself. "tensors" holds the output and
every gradient (the input's and each parameter's): "bits" is the hex of its bytes in memory order (eight digits per
fp32 element: its bit pattern, little-endian) for a tensor of at most BITS_MAX elements, "sha256" the digest of those
same bytes for a larger one (equal digests: equal bit patterns; the file stays small). "outcome" is "ok", or for the
M == 0 cases what happened: the result's shape or the exception's type and message, for the forward and, where that
returned, the backward.

tests/golden/layer_launches_parent.json holds run_case's result for every case at the commit before the exact code
packing, the weight-only GEMM rows and the backward switch were shared through _lib (pack_codes, gemm_wonly_rows,
backward_ops):
    python tests/layer_launch_trace.py tests/golden/layer_launches_parent.json
"""
import hashlib
import inspect
import json
import os
import sys

import torch

WRAPPERS = ("pack_weight", "pad_bias", "gemm_wonly", "conv_wonly", "gemm", "gemm_wgrad", "quantize_act_i8",
            "fake_quant_f32", "quant_backward", "ultra_weight_codes", "ultra_weight_quant_backward",
            "im2col_quant_i8", "col2im_quant_backward", "conv_wgrad")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_launches_parent.json")
M_ROWS = 3
BITS_MAX = 64


def _describe(v):
    if isinstance(v, torch.Tensor):
        s = f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}{tuple(v.stride())}"
        if v.numel() == 1:
            s += f"={v.item()!r}"
        if v.data_ptr() % 16:
            s += "|unaligned"
        return s
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (tuple, list, torch.Size)):
        return [_describe(e) for e in v]
    if isinstance(v, torch.device):
        return str(v)
    raise TypeError(f"layer_launch_trace: cannot record a {type(v).__name__}")


class recording:
    """Context: the `_lib` wrappers of WRAPPERS record into .launches while it is open."""

    def __enter__(self):
        from quantized_vit_amd import _lib
        self.launches, self._saved = [], {}

        def recorder(name, fn):
            sig = inspect.signature(fn)

            def call(*args, **kwargs):
                bound = sig.bind(*args, **kwargs)
                bound.apply_defaults()
                self.launches.append([name, {k: _describe(v) for k, v in bound.arguments.items()}])
                return fn(*args, **kwargs)
            return call

        for name in WRAPPERS:
            self._saved[name] = getattr(_lib, name)
            setattr(_lib, name, recorder(name, self._saved[name]))
        return self

    def __exit__(self, *exc):
        from quantized_vit_amd import _lib
        for name, fn in self._saved.items():
            setattr(_lib, name, fn)
        return False


def tensor_bits(t):
    c = t.detach().contiguous().cpu()
    raw = bytes(c.reshape(-1).view(torch.uint8).tolist())
    out = {"dtype": str(c.dtype).replace("torch.", ""), "shape": list(c.shape)}
    if c.numel() <= BITS_MAX:
        out["bits"] = raw.hex()
    else:
        out["sha256"] = hashlib.sha256(raw).hexdigest()
    return out


# ---- the layers: constructor weights replaced by CPU-seeded values, constant quantizer scalars ---------------------
W4_Q = (2.0 ** -6, 7 * 2.0 ** -6)            # (d, q_m): levels +-7, int4 codes
W16_Q = (2.0 ** -16, 32767 * 2.0 ** -16)     # levels +-32767, the default num_bits = 16: base-256 digits (W16)
ACT_Q = (2.0 ** -5, 127 * 2.0 ** -5)         # int8 activation codes


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def quantize_linear(dev, k, n, wq, aq=None, seed=3):
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeLinear
    mode = QuantizationMode.WEIGHT_ONLY if aq is None else QuantizationMode.WEIGHT_AND_ACTIVATION
    layer = QuantizeLinear(k, n, bias=True, quant_type=QuantizationType.SYMMETRIC_LINEAR, quant_mode=mode)
    g = _gen(seed)
    layer.weight.data.copy_(0.05 * torch.randn((n, k), generator=g))
    layer.bias.data.copy_(0.1 * torch.randn(n, generator=g))
    layer.d_quant_wt.data.fill_(wq[0])
    layer.q_m_wt.data.fill_(wq[1])
    if aq is not None:
        layer.d_quant_act.data.fill_(aq[0])
        layer.q_m_act.data.fill_(aq[1])
    return layer.to(dev).eval()


def quantize_conv(dev, seed=5):
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeConv2d
    layer = QuantizeConv2d(3, 5, 3, stride=1, padding=1, bias=True, quant_type=QuantizationType.SYMMETRIC_LINEAR,
                           quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    g = _gen(seed)
    layer.weight.data.copy_(0.05 * torch.randn(layer.weight.shape, generator=g))
    layer.bias.data.copy_(0.1 * torch.randn(5, generator=g))
    layer.d_quant_wt.data.fill_(W4_Q[0])
    layer.q_m_wt.data.fill_(W4_Q[1])
    layer.d_quant_act.data.fill_(ACT_Q[0])
    layer.q_m_act.data.fill_(ACT_Q[1])
    return layer.to(dev).eval()


def ultra_linear(dev, k, n, w_bit, seed=7):
    from quantized_vit_amd.quant_ultra import linear_Q_fn
    layer = linear_Q_fn(w_bit)(k, n, bias=True)
    g = _gen(seed)
    layer.weight.data.copy_(0.5 * torch.randn((n, k), generator=g))
    layer.bias.data.copy_(0.1 * torch.randn(n, generator=g))
    return layer.to(dev)


def ultra_conv(dev, seed=9):
    from quantized_vit_amd.quant_ultra import conv2d_Q_fn
    layer = conv2d_Q_fn(4)(3, 5, 3, stride=1, padding=1, bias=True)
    g = _gen(seed)
    layer.weight.data.copy_(0.5 * torch.randn(layer.weight.shape, generator=g))
    layer.bias.data.copy_(0.1 * torch.randn(5, generator=g))
    return layer.to(dev)


def rows_input(dev, k, how="plain", m=M_ROWS, seed=11):
    """The [m, k] input of a linear case, a leaf that requires grad: "plain" contiguous fp32; "stride" the first k
    columns of a [m, k + 2] buffer (row stride no multiple of 4); "offset" starting one float into its storage (base
    not 16-byte aligned); "half" float16."""
    x = torch.randn((m, k), generator=_gen(seed))
    if how == "stride":
        buf = torch.zeros((m, k + 2), device=dev)
        buf[:, :k] = x.to(dev)
        x = buf[:, :k]
    elif how == "offset":
        buf = torch.zeros(m * k + 4, device=dev)
        buf[1:1 + m * k] = x.reshape(-1).to(dev)
        x = buf[1:1 + m * k].view(m, k)
    elif how == "half":
        x = x.to(dev).half()
    else:
        x = x.to(dev)
    return x.detach().requires_grad_(True)


def _collect(layer, x, y):
    out = {"output": tensor_bits(y)}
    if x.grad is not None:
        out["grad_input"] = tensor_bits(x.grad)
    for name, p in layer.named_parameters():
        if p.grad is not None:
            out["grad_" + name] = tensor_bits(p.grad)
    return out


def _forward_backward(layer, x, call=None, seed=13):
    """Forward, then backward on a fixed output gradient: the case's "tensors"."""
    y = layer(x) if call is None else call(layer, x)
    G = torch.randn(tuple(y.shape), generator=_gen(seed)).to(device=y.device, dtype=y.dtype)
    y.backward(G)
    torch.cuda.synchronize()
    return _collect(layer, x, y)


def _outcome(fn):
    try:
        r = fn()
        torch.cuda.synchronize()
        return r, "shape " + str(list(r.shape)) if isinstance(r, torch.Tensor) else "returned"
    except Exception as e:   # recorded, not judged: whatever the parent does is what the change must do
        return None, f"{type(e).__name__}: {e}"


def _empty_rows(layer, x):
    """The M == 0 outcome: forward, and the backward where the forward returned."""
    y, fwd = _outcome(lambda: layer(x))
    out = {"forward": fwd}
    if y is not None:
        _, out["backward"] = _outcome(lambda: y.backward(torch.zeros_like(y)))
        if x.grad is not None:
            out["grad_input"] = "shape " + str(list(x.grad.shape))
    return out


class _switch:
    """A module attribute set for the case and put back."""

    def __init__(self, module, name, value):
        self.module, self.name, self.value = module, name, value

    def __enter__(self):
        import importlib
        self.mod = importlib.import_module("quantized_vit_amd." + self.module)
        self.saved = getattr(self.mod, self.name)
        setattr(self.mod, self.name, self.value)

    def __exit__(self, *exc):
        setattr(self.mod, self.name, self.saved)
        return False


def _cases():
    """name -> function(dev) returning (tensors, outcome); the layer is built inside it, under the recorder."""
    cases = {}

    def add(name, fn, switch=None):
        cases[name] = (fn, switch)

    # QuantizeLinear, weight-only, 4-bit: each arm of the padding predicate of the forward and of the dgrad
    for k, n, how in ((128, 8, "plain"), (100, 6, "plain"), (128, 128, "plain"), (128, 8, "stride"),
                      (128, 8, "offset"), (128, 8, "half")):
        add(f"qlinear-wonly-w4-{k}x{n}-{how}",
            lambda dev, k=k, n=n, how=how: _forward_backward(quantize_linear(dev, k, n, W4_Q), rows_input(dev, k, how)))
    add("qlinear-wonly-w16-128x8",
        lambda dev: _forward_backward(quantize_linear(dev, 128, 8, W16_Q), rows_input(dev, 128)))

    # QuantizeLinear, weight and activation, int path: packed_t from the plan's codes (eval), from t_src (training),
    # and the bound-codes branch of _build_plan (load_weight_codes)
    def int_path(dev, k, n, how):
        layer = quantize_linear(dev, k, n, W4_Q, ACT_Q)
        if how == "train":
            layer.train()
        elif how == "codes":
            layer.load_weight_codes(torch.randint(-7, 8, (n, k), generator=_gen(17)))
        return _forward_backward(layer, rows_input(dev, k))

    for k, n in ((128, 8), (100, 6)):
        for how in ("eval", "train", "codes"):
            add(f"qlinear-int-{k}x{n}-{how}", lambda dev, k=k, n=n, how=how: int_path(dev, k, n, how))
    for value in ("hip", "torch", "dgrad", "wgrad"):
        add(f"qlinear-int-128x8-BACKWARD_GEMM-{value}", lambda dev: int_path(dev, 128, 8, "eval"),
            ("quant_layers", "BACKWARD_GEMM", value))

    # QuantizeConv2d, weight and activation, int path, on each value of its own switch (None: unset)
    def qconv(dev):
        x = torch.randn((2, 3, 8, 8), generator=_gen(19)).to(dev).requires_grad_(True)
        return _forward_backward(quantize_conv(dev), x)

    for value in (None, "hip", "torch", "dgrad", "wgrad"):
        add(f"qconv-int-3to5-CONV_BACKWARD_GEMM-{value}", qconv, ("quant_layers", "CONV_BACKWARD_GEMM", value))

    # Linear_Q / Conv2d_Q (UltraNet's modules)
    for w_bit in (4, 8):
        for k, n in ((128, 8), (100, 6), (128, 128)):
            add(f"linear_q-w{w_bit}-{k}x{n}",
                lambda dev, k=k, n=n, w_bit=w_bit: _forward_backward(ultra_linear(dev, k, n, w_bit), rows_input(dev, k)))
        for value in ("torch", "dgrad"):
            add(f"linear_q-w{w_bit}-128x8-ULTRA_BWD-{value}",
                lambda dev, w_bit=w_bit: _forward_backward(ultra_linear(dev, 128, 8, w_bit), rows_input(dev, 128)),
                ("quant_ultra", "ULTRA_BWD", value))

    def conv_q(dev):
        x = (torch.randint(0, 16, (2, 3, 8, 8), generator=_gen(23)).float() / 15).to(dev).requires_grad_(True)
        return _forward_backward(ultra_conv(dev), x, call=lambda layer, x: layer(x, _in_levels=15))

    add("conv2d_q-w4-3to5", conv_q)

    # M == 0
    add("qlinear-wonly-w4-128x8-empty",
        lambda dev: _empty_rows(quantize_linear(dev, 128, 8, W4_Q), rows_input(dev, 128, m=0)))
    add("linear_q-w4-128x8-empty",
        lambda dev: _empty_rows(ultra_linear(dev, 128, 8, 4), rows_input(dev, 128, m=0)))
    return cases


CASES = _cases()


def run_case(dev, name):
    fn, switch = CASES[name]
    with recording() as rec:
        if switch is not None:
            with _switch(*switch):
                got = fn(dev)
        else:
            got = fn(dev)
    if name.endswith("-empty"):
        return {"launches": rec.launches, "tensors": {}, "outcome": got}
    return {"launches": rec.launches, "tensors": got, "outcome": "ok"}


def main(path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dev = torch.device("cuda:0")
    lines = ["{", ' "cases": {']
    for i, name in enumerate(CASES):
        c = run_case(dev, name)
        print(name, len(c["launches"]), sorted(c["tensors"]), c["outcome"])
        lines.append(f'  {json.dumps(name)}: {{"outcome": {json.dumps(c["outcome"])}, "tensors": {{')
        lines += ["   " + json.dumps(k) + ": " + json.dumps(v) + ("," if j + 1 < len(c["tensors"]) else "")
                  for j, (k, v) in enumerate(c["tensors"].items())]
        lines.append('  }, "launches": [')
        lines += ["   " + json.dumps(l) + ("," if j + 1 < len(c["launches"]) else "")
                  for j, l in enumerate(c["launches"])]
        lines.append("  ]}" + ("," if i + 1 < len(CASES) else ""))
    lines += [" }", "}"]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    json.load(open(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
