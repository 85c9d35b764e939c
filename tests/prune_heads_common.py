"""What the head-pruning tests share: the kernel-level net (two head groups and one BASIC group), the two-block ViT
of the schedule and compression tests, and the reference's groups for both (tests/prune_heads_ref.py's permutation on
tests/prune_step_ref.py's forms).

Net: l0 a head group of H = 3, hd = 4 and width 50 (36 rows, the scalar path); l1 a head group of H = 2, hd = 64 and
width 128 (384 rows, the 16-byte path); l2 a BASIC group of 33 rows of width 48 and l3 a head group of H = 2, hd = 4
and width 48 (24 rows), the weights of both starting 4 bytes into their storage (the 16-byte path must fall back, in
the one-row and in the head geometry)."""
import torch
import torch.nn as nn

from prune_heads_ref import HeadSpec, rows_of_units
from prune_step_ref import Group

HEADS = {0: (3, 4), 1: (2, 64), 3: (2, 4)}   # layer index -> (H, hd)
ROWS, WIDTHS = (3 * 3 * 4, 3 * 2 * 64, 33, 3 * 2 * 4), (50, 128, 48, 48)
UNITS = (3, 2, 33, 2)
OFFSET = (2, 3)                              # layers whose weight starts 4 bytes into its storage
NGROUPS = len(ROWS)
SPECS = [HeadSpec([f"l{i}.weight", f"l{i}.bias"], *HEADS[i]) for i in HEADS]


class Net(nn.Module):
    def __init__(self, nonlinear=True):
        super().__init__()
        from quantized_vit_amd import QuantizationMode as M, QuantizationType as T, QuantizeLinear
        qt = T.SYMMETRIC_NONLINEAR if nonlinear else T.SYMMETRIC_LINEAR
        for i, (r, w) in enumerate(zip(ROWS, WIDTHS)):
            setattr(self, f"l{i}", QuantizeLinear(w, r, bias=True, quant_type=qt, quant_mode=M.WEIGHT_AND_ACTIVATION))
        self.other = nn.Parameter(torch.zeros(5, 7))


def make_net(dev, seed=0, nonlinear=True):
    g = torch.Generator().manual_seed(seed)
    net = Net(nonlinear).to(dev)
    for i in OFFSET:
        ly = getattr(net, f"l{i}")
        ly.weight = nn.Parameter(torch.zeros(ROWS[i] * WIDTHS[i] + 1, device=dev)[1:].view(ROWS[i], WIDTHS[i]))
        assert ly.weight.data_ptr() % 16 == 4 and ly.weight.is_contiguous() and WIDTHS[i] % 4 == 0
    assert net.l1.weight.data_ptr() % 16 == 0
    with torch.no_grad():
        for name, p in net.named_parameters():
            leaf = name.split(".")[-1]
            if leaf.startswith("q_m"):
                v = 0.9 + 0.2 * torch.rand(1, generator=g)
            elif leaf.startswith("t_quant"):
                v = 0.95 + 0.1 * torch.rand(1, generator=g)
            elif leaf.startswith("d_quant"):
                v = (1.0 + 0.1 * torch.rand(1, generator=g)) / 127.0
            else:
                v = torch.randn(p.shape, generator=g) * 0.3
            p.copy_(v.to(dev))
    return net


def dev_groups(net):
    from quantized_vit_amd import PruneGroup
    out = []
    for i in range(NGROUPS):
        ly = getattr(net, f"l{i}")
        geom = dict(sections=3, unit_rows=HEADS[i][1]) if i in HEADS else {}
        out.append(PruneGroup(f"g{i}", ly, [ly.weight, ly.bias], **geom))
    return out


def ref_groups():
    """On the permuted copy every group is BASIC."""
    return [Group(f"g{i}", f"l{i}", [f"l{i}.weight", f"l{i}.bias"]) for i in range(NGROUPS)]


def physical_rows(units_per_layer):
    """Per layer: the physical rows of the listed units (the units themselves for the BASIC group)."""
    return [rows_of_units(u, *HEADS[i]) if i in HEADS else list(u) for i, u in enumerate(units_per_layer)]


# ---- the two-block ViT: N = 5 tokens, 4 heads of 64, hidden 384 ---------------------------------------------------------
VIT = dict(img_size=32, patch_size=16, embed_dim=256, depth=2, num_heads=4, mlp_ratio=1.5, num_classes=10)
VIT_HEADS, VIT_HD, VIT_HIDDEN = 4, 64, 384


def head_vit(dev, seed=0):
    """W4A8, quantized and calibrated as tests/test_gpu_prune_step.py's small_vit is."""
    from quantized_vit_amd import QuantizationMode, QuantizationType, collect_input_absmax, model_to_quantize_model, \
        set_activation_quant
    from quantized_vit_amd.calibrate import redraw_init_artifacts, synthetic_images
    from quantized_vit_amd.vit_model import VisionTransformer
    torch.manual_seed(seed)
    model = VisionTransformer(representation_size=None, **VIT)
    redraw_init_artifacts(model)
    model = model.to(dev).eval()
    absmax = collect_input_absmax(model, synthetic_images(2, 32, seed=1, device=dev))
    model = model_to_quantize_model(model, num_bits=4, quant_type=QuantizationType.SYMMETRIC_NONLINEAR,
                                    quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    set_activation_quant(model, absmax, bits=8, t=1.0)
    return model.eval()


VIT_SPECS = [HeadSpec([f"blocks.{i}.attn.qkv.weight", f"blocks.{i}.attn.qkv.bias"], VIT_HEADS, VIT_HD)
             for i in range(2)]


def vit_ref_groups():
    """vit_head_prune_groups + vit_mlp_prune_groups, in that order, on the permuted copy."""
    heads = [Group(f"blocks.{i}.attn", f"blocks.{i}.attn.qkv",
                   [f"blocks.{i}.attn.qkv.weight", f"blocks.{i}.attn.qkv.bias"]) for i in range(2)]
    mlps = [Group(f"blocks.{i}.mlp", f"blocks.{i}.mlp.fc1",
                  [f"blocks.{i}.mlp.fc1.weight", f"blocks.{i}.mlp.fc1.bias"]) for i in range(2)]
    return heads + mlps


GRAD_SEED = 500


def vit_grads(start, s, seed=GRAD_SEED):
    g = torch.Generator().manual_seed(seed + s)
    return {k: torch.randn(v.shape, generator=g) * (0.002 if v.numel() == 1 else 0.02) for k, v in start.items()}

# The default criteria never rank a head below an MLP unit on this model (tests/test_prune_heads_cpu.py measures it),
# so the schedule is run twice: with the default weights, and with the cosine criterion alone, under which heads are
# pruned.
COSINE = {"cosine_similarity": 1.0}
