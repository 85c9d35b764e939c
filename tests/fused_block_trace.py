"""Launch recorder for the fused ViT block (a helper, not a test).

record(model, img) runs one forward under torch.no_grad() with the `_lib` wrappers the fused block calls replaced by
recorders, and returns (launches, logits): the ordered list of [wrapper name, {parameter name: value}] and the fp32
logits. Arguments are bound to the wrapper's own signature (defaults applied), so a call reads the same whether an
argument was passed by position or by name. A tensor is recorded as "dtype[shape](strides)", with its value when it
holds one element (the quantizer scalars) and "@resid" when it lives in the residual buffer; scalars by value; no
addresses. The residual buffer is the storage norm1 of the first block reads (the first LayerNorm launch).

CASES names the models and switch settings of tests/test_gpu_fused_routes.py; run_case(dev, name) builds the case's
model afresh (so the per-plan code tables are built inside the recorded forward), sets the switches, records, and
restores them. tests/golden/fused_block_launches_parent.json holds what run_case returned for every case (launches,
logit bits, KERNEL_TIMING events per name) at the commit before forward_fused_chain_ was given one route decision and one tail:
    python tests/fused_block_trace.py tests/golden/fused_block_launches_parent.json
"""
import inspect
import json
import os
import sys

import torch

WRAPPERS = ("layernorm_quant_i8", "layernorm_quant_i8_t32", "gemm", "gemm_a32", "gemm_resid_ln", "gemm_qkv_split",
            "attention", "attention_split", "qkv_attention", "qkv_attention_q", "quantize_act_i8", "epi_table_build")
SWITCHES = ("LAST_BLOCK_CLS_ONLY", "FUSE_RESID_LN", "FC1_WEIGHT_STATIONARY")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_block_launches_parent.json")


def _describe(v, resid):
    if isinstance(v, torch.Tensor):
        s = f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}{tuple(v.stride())}"
        if v.numel() == 1:
            s += f"={v.item()!r}"
        if resid and v.untyped_storage().data_ptr() == resid[0].untyped_storage().data_ptr():
            s += "@resid"
        return s
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, torch.device):
        return str(v)
    raise TypeError(f"fused_block_trace: cannot record a {type(v).__name__}")


def record(model, img):
    """One forward of `model` on `img` under no_grad: (launches, logits on the CPU)."""
    from quantized_vit_amd import _lib
    launches, resid, saved = [], [], {}

    def recorder(name, fn):
        sig = inspect.signature(fn)

        def call(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            if name == "layernorm_quant_i8" and not resid:
                resid.append(bound.arguments["x2d"])   # held: its storage is not reused while recording
            launches.append([name, {k: _describe(v, resid) for k, v in bound.arguments.items()}])
            return fn(*args, **kwargs)
        return call

    for name in WRAPPERS:
        saved[name] = getattr(_lib, name)
        setattr(_lib, name, recorder(name, saved[name]))
    try:
        with torch.no_grad():
            logits = model(img)
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(_lib, name, fn)
    return launches, logits.float().cpu()


# name: (embed_dim, num_heads, distilled, split_ok patched to False, {switch: value})
def _cases():
    models = {"fused": (256, 4, False, False), "split128": (128, 2, False, False), "split_hd80": (160, 2, False, False),
              "attention_i8": (128, 2, False, True), "core": (64, 2, False, False)}
    out = {}
    for m, spec in models.items():
        for last in (True, False):
            out[f"{m}-cls{int(last)}"] = spec + ({"LAST_BLOCK_CLS_ONLY": last},)
            if m in ("fused", "split128"):
                out[f"{m}-cls{int(last)}-fuse_ln"] = spec + ({"LAST_BLOCK_CLS_ONLY": last, "FUSE_RESID_LN": True},)
    # the weight-stationary fc1 (qvit_gemm_a32_fits) takes K = 768 or 1024 with N = 3072 only: dim 768 is the smallest
    out["fused768-cls1-fc1_a32"] = (768, 12, False, False, {"LAST_BLOCK_CLS_ONLY": True, "FC1_WEIGHT_STATIONARY": True})
    out["fused-distilled-cls1"] = (256, 4, True, False, {"LAST_BLOCK_CLS_ONLY": True})
    return out


CASES = _cases()
IMG, PATCH, DEPTH, BATCH, CLASSES = 32, 16, 2, 2, 10
# max |input| of every quantized layer, by the last two parts of its module name
ACT_ABSMAX = {"patch_embed.proj": 1.0, "attn.qkv": 3.5, "attn.proj": 0.25, "mlp.fc1": 3.5, "mlp.fc2": 0.5,
              "head": 3.5, "head_dist": 3.5}


def build_model(dev, dim, heads, distilled):
    """The depth-2 W4A8 ViT of a case: constructor weights from CPU seed 21, 4-bit nonlinear weight quantizers, 8-bit
    activation quantizers with the fixed clip values ACT_ABSMAX (what a calibration batch gives these models, rounded:
    constants, so that the recording does not depend on the host's fp32 matmul)."""
    from quantized_vit_amd import vit_model
    from quantized_vit_amd.calibrate import redraw_init_artifacts, set_activation_quant
    from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType
    from quantized_vit_amd.quant_model import model_to_quantize_model
    torch.manual_seed(21)
    m = vit_model.VisionTransformer(img_size=IMG, patch_size=PATCH, embed_dim=dim, depth=DEPTH, num_heads=heads,
                                    num_classes=CLASSES, distilled=distilled)
    redraw_init_artifacts(m)
    m = m.eval()
    absmax = {name: ACT_ABSMAX[".".join(name.split(".")[-2:])]
              for name, mod in m.named_modules() if isinstance(mod, (torch.nn.Linear, torch.nn.Conv2d))}
    m = model_to_quantize_model(m, num_bits=4, quant_type=QuantizationType.SYMMETRIC_NONLINEAR,
                                quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    set_activation_quant(m, absmax, bits=8)
    return m.eval().to(dev)


def block_plans(model):
    """The four linears' plans of every block, in launch order."""
    return [l.quant_plan() for b in model.blocks for l in (b.attn.qkv, b.attn.proj, b.mlp.fc1, b.mlp.fc2)]


TIMING_NAMES = ("qkv_attn", "proj", "ln", "fc1", "fc2", "qkv_attn_cls", "proj_cls", "ln_cls", "fc1_cls", "fc2_cls")


def run_case(dev, name, event_counts=None):
    """(launches, logits, model) of case `name`; every switch and the patched split_ok are restored. With a dict
    `event_counts`, the forward runs with every KERNEL_TIMING name armed and the dict receives name -> events."""
    from quantized_vit_amd import vit_model
    from quantized_vit_amd.calibrate import synthetic_images
    dim, heads, distilled, no_split, switches = CASES[name]
    model = build_model(dev, dim, heads, distilled)
    img = synthetic_images(BATCH, IMG, seed=4).to(dev)
    saved = {s: getattr(vit_model, s) for s in SWITCHES}
    split_ok = vit_model.ViTAttention.split_ok
    try:
        for s in SWITCHES:
            setattr(vit_model, s, switches.get(s, False))
        if no_split:
            vit_model.ViTAttention.split_ok = lambda self, p_qkv: False
        if event_counts is not None:
            vit_model.KERNEL_TIMING.update({n: [] for n in TIMING_NAMES})
        launches, logits = record(model, img)
    finally:
        if event_counts is not None:
            event_counts.update({n: len(vit_model.KERNEL_TIMING.pop(n, ())) for n in TIMING_NAMES})
        vit_model.ViTAttention.split_ok = split_ok
        for s, v in saved.items():
            setattr(vit_model, s, v)
    return launches, logits, model


def logits_bits(logits):
    return logits.contiguous().view(torch.int32).flatten().tolist()


def main(path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from quantized_vit_amd import _lib
    dev = torch.device("cuda:0")
    cases = {}
    for name in CASES:
        events = {}
        launches, logits, model = run_case(dev, name, events)
        assert all(p.int_path and p.wfmt == _lib.W4 for p in block_plans(model)), name
        assert torch.isfinite(logits).all(), name
        cases[name] = {"logits_shape": list(logits.shape), "logits_bits": logits_bits(logits), "events": events,
                       "launches": launches}
        print(name, len(launches), events)
    lines = ["{", ' "cases": {']
    for i, (name, c) in enumerate(cases.items()):
        lines.append(f'  {json.dumps(name)}: {{"logits_shape": {json.dumps(c["logits_shape"])}, '
                     f'"logits_bits": {json.dumps(c["logits_bits"])}, "events": {json.dumps(c["events"])}, '
                     '"launches": [')
        lines += ["   " + json.dumps(l) + ("," if j + 1 < len(c["launches"]) else "")
                  for j, l in enumerate(c["launches"])]
        lines.append("  ]}" + ("," if i + 1 < len(cases) else ""))
    lines += [" }", "}"]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    json.load(open(path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
