"""The last block computes only the token rows the heads read (vit_model.LAST_BLOCK_CLS_ONLY).

Kernel: qvit_qkv_attention_q (the class-token query arm of the fused qkv + attention kernel) against the same rows
of qvit_qkv_attention, bit for bit, with its output embedded in a poisoned arena (tests/footprint_tools.py).
Strided residual GEMM: qvit_gemm with EPI_F32_RESID on the class rows of a residual buffer (ldc = N*C).
Model: logits with the pruned last block equal the full ones bit for bit; tracing and the timing hooks keep their
meaning. Every bar here is equality: the pruned path runs the same arithmetic on the same inputs.
"""
import pytest
import torch

from footprint_tools import Arena, scalar as _p
from quantized_vit_amd import _lib, vit_model
from quantized_vit_amd import quant_layers as ql
from quantized_vit_amd.calibrate import (build_quantized_vit, collect_input_absmax, redraw_init_artifacts,
                                         set_activation_quant, synthetic_images)
from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType
from quantized_vit_amd.quant_model import model_to_quantize_model

pytestmark = pytest.mark.gpu

MB = 1 << 20
QM, QT_T = 0.5, 0.9
QD = QM ** QT_T / 127
QVIT_EINVAL = -1   # include/qvit_hip.h


def _quant_kw(dev, table):
    from quantized_vit_amd.quant_layers import epilogue_table_geometry, saturation_level
    kw = dict(out_qtype=_lib.QT_NONLINEAR, out_d=_p(QD, dev), out_qm=_p(QM, dev), out_t=_p(QT_T, dev))
    if table:
        geo = epilogue_table_geometry(_lib.QT_NONLINEAR, QD, QM, QT_T,
                                      saturation_level(_lib.QT_NONLINEAR, QD, QM, QT_T), False)
        kw["epi_table"] = _lib.epi_table_build(_lib.EPI_I8, _lib.QT_NONLINEAR, kw["out_d"], kw["out_qm"], kw["out_t"],
                                               0, *geo, dev)
        assert int(kw["epi_table"][12:16].view(torch.int32).item()) == 1
    return kw


def _units_past_grid(dev):
    """B with B * 3 (image, head) units > 2 x the workgroups of the launch (one per CU): every workgroup walks more
    than one unit, some three."""
    return (2 * torch.cuda.get_device_properties(dev).multi_processor_count + 8) // 3 + 1


# N: one key block of < 32 rows (5), a full block + a remainder of 1 (33), the model's own (197: 7 blocks, the
# balanced 13-tile projection plan), the maximum (208). K = 256 runs the runtime-K projection loop, 768 the unrolled
# one. B = 0 stands for _units_past_grid.
SHAPES = [(1, 5, 1, 256, 1), (3, 5, 3, 256, 2), (1, 33, 3, 768, 2), (3, 33, 1, 256, 1), (3, 197, 12, 768, 1),
          (1, 197, 3, 256, 2), (3, 197, 3, 768, 2), (3, 208, 3, 768, 2), (1, 208, 1, 256, 1), (0, 33, 3, 256, 2)]


@pytest.mark.parametrize("mode", ["f32", "i8", "i8_table"])
@pytest.mark.parametrize("B,N,H,K,NQ", SHAPES)
def test_qkv_attention_q_equals_full_rows(dev, B, N, H, K, NQ, mode):
    """Row b*NQ + i of qvit_qkv_attention_q == row b*N + i of qvit_qkv_attention (torch.equal on the bits), and no
    byte outside the [B*NQ][H*64] block of `out` changes (pad columns [H*64, ldo), guard rows). The int8 output runs
    once on the 4-byte stores (ldo % 16 != 0, "i8") and once on the 16-byte ones ("i8_table")."""
    from test_gpu_attention import _fused_case
    B = B or _units_past_grid(dev)
    A, packed, npad, kpad, bias_pad, da, dw = _fused_case(dev, B, N, H, seed=31 * N + 7 * H + NQ, K=K)
    i8 = mode != "f32"
    odt = torch.int8 if i8 else torch.float32
    amode = _lib.ATT_I8 if i8 else _lib.ATT_F32
    s = 1.0 if i8 else 2.0 ** -2
    kw = _quant_kw(dev, mode == "i8_table") if i8 else {}
    full = torch.full((B * N, 64 * H), 99, dtype=odt, device=dev)
    _lib.qkv_attention(A, B, N, kpad, packed, npad, da, dw, bias_pad, H, 0.125, full, amode, s, **kw)
    ar = Arena(dev, 2 * MB)
    out = ar.carve(B * NQ, 64 * H, 64 * H + (16 if mode == "i8_table" else 4), odt, writable=True, name="out")
    ar.seal()
    _lib.qkv_attention_q(A, B, N, NQ, kpad, packed, npad, da, dw, bias_pad, H, 0.125, out, amode, s, **kw)
    torch.cuda.synchronize()
    ar.assert_untouched()
    want = full.view(B, N, 64 * H)[:, :NQ].reshape(B * NQ, 64 * H).cpu()
    got = out.cpu()
    if not i8:
        assert torch.isfinite(want).all()
        want, got = want.view(torch.int32), got.view(torch.int32)
    assert torch.equal(got, want)


@pytest.mark.parametrize("NQ", [0, 33, 6, -1])
def test_qkv_attention_q_invalid_nq(dev, NQ):
    """NQ outside 1 .. min(N, 32) (N = 5 here; 33 with N = 40 as well): the ABI's invalid-argument status, nothing
    launched, `out` untouched."""
    from test_gpu_attention import _fused_case
    for N in (5, 40) if NQ == 33 else (5,):
        B, H = 2, 1
        A, packed, npad, kpad, bias_pad, da, dw = _fused_case(dev, B, N, H, seed=3, K=256)
        out = torch.full((B * 32, 64 * H), -7.0, device=dev)
        code = _lib.load().qvit_qkv_attention_q(A.data_ptr(), B, N, NQ, kpad, A.stride(0), packed.data_ptr(), _lib.W4,
                                                npad, da.data_ptr(), dw.data_ptr(), bias_pad.data_ptr(), H, 64, 0.125,
                                                1.0, _lib.ATT_F32, out.data_ptr(), out.stride(0), 0, None, None, None,
                                                0, None, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        assert code == QVIT_EINVAL
        assert bool((out == -7.0).all())
        with pytest.raises(_lib.QvitError):
            _lib.qkv_attention_q(A, B, N, NQ, kpad, packed, npad, da, dw, bias_pad, H, 0.125, out)


def test_gemm_resid_strided_class_rows(dev):
    """qvit_gemm with EPI_F32_RESID at M = B on the class rows of a [B, N, C] residual buffer (ldc = N*C, the codes
    with lda = N*K) == the same rows of the full-M launch; the other rows keep their values. B = 3, N = 5, C = 256,
    K = 256."""
    from test_gpu_kernels import pack_codes
    B, N, C, K = 3, 5, 256, 256
    g = torch.Generator().manual_seed(11)
    a = torch.randint(-127, 128, (B * N, K), generator=g).to(torch.int8).to(dev)
    w = torch.randint(-7, 8, (C, K), generator=g)
    bias = torch.randn(C, generator=g) * 0.3
    base = torch.randn(B * N, C, generator=g).to(dev)
    packed, npad, kpad = pack_codes(w, _lib.W4, dev)
    assert kpad == K
    bias_pad = _lib.pad_bias(bias.to(dev), C, npad, dev)
    da, dw = _p(0.01, dev), _p(0.002, dev)
    full = base.clone()
    _lib.gemm(a, B * N, K, packed, _lib.W4, C, npad, da, dw, bias_pad, _lib.EPI_F32_RESID, full)
    x = base.clone()
    rows, a_rows = x.view(B, N, C)[:, 0], a.view(B, N, K)[:, 0]
    assert rows.stride(0) == N * C and a_rows.stride(0) == N * K
    _lib.gemm(a_rows, B, K, packed, _lib.W4, C, npad, da, dw, bias_pad, _lib.EPI_F32_RESID, rows)
    torch.cuda.synchronize()
    x3, f3, b3 = x.view(B, N, C).cpu(), full.view(B, N, C).cpu(), base.view(B, N, C).cpu()
    assert not torch.equal(f3[:, 0], b3[:, 0])
    assert torch.equal(x3[:, 0].view(torch.int32), f3[:, 0].view(torch.int32))
    assert torch.equal(x3[:, 1:].view(torch.int32), b3[:, 1:].view(torch.int32))


# ---- model ----------------------------------------------------------------------------------------------
def _direct_vit(dev, distilled):
    """A depth-2, 3-head, 192-wide ViT on 64 x 64 images (N = 17, or 18 distilled) built from the constructor,
    quantized and calibrated as calibrate.build_quantized_vit does."""
    torch.manual_seed(21)
    m = vit_model.VisionTransformer(img_size=64, patch_size=16, embed_dim=192, depth=2, num_heads=3, num_classes=10,
                                    distilled=distilled)
    redraw_init_artifacts(m)
    m = m.eval()
    absmax = collect_input_absmax(m, synthetic_images(2, 64, seed=1))
    m = model_to_quantize_model(m, num_bits=4, quant_type=QuantizationType.SYMMETRIC_NONLINEAR,
                                quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    set_activation_quant(m, absmax, bits=8)
    return m.eval().to(dev)


_models = {}


def _model(dev, name):
    if name not in _models:
        if name == "tiny":
            _models[name] = (build_quantized_vit("vit_tiny_patch16_224", seed=8).to(dev), 224)
        else:
            _models[name] = (_direct_vit(dev, distilled=name == "distilled"), 64)
    return _models[name]


def _forward(model, img, prune, timing=()):
    saved = vit_model.LAST_BLOCK_CLS_ONLY
    vit_model.LAST_BLOCK_CLS_ONLY = prune
    for n in timing:
        vit_model.KERNEL_TIMING[n] = []
    try:
        with torch.no_grad():
            out = model(img)
        torch.cuda.synchronize()
    finally:
        vit_model.LAST_BLOCK_CLS_ONLY = saved
        events = {n: vit_model.KERNEL_TIMING.pop(n) for n in timing}
    return out.cpu(), events


CLS_NAMES = ("qkv_attn_cls", "proj_cls", "ln_cls", "fc1_cls", "fc2_cls")
FULL_NAMES = ("qkv_attn", "proj", "ln", "fc1", "fc2")


@pytest.mark.parametrize("name", ["tiny", "direct", "distilled"])
def test_vit_logits_bit_identical(dev, name):
    """Logits with the pruned last block == logits with the whole one (torch.equal), and the pruned forward did go
    through the class-token launches: one event under each *_cls name, depth - 1 under fc1 (2 depth - 1 under ln:
    the last block's norm1 still runs on every row)."""
    model, size = _model(dev, name)
    img = synthetic_images(2, size, seed=4).to(dev)
    depth = len(model.blocks)
    full, ev_full = _forward(model, img, False, FULL_NAMES + CLS_NAMES)
    pruned, ev = _forward(model, img, True, FULL_NAMES + CLS_NAMES)
    assert torch.isfinite(full).all()
    assert torch.equal(pruned.view(torch.int32), full.view(torch.int32))
    assert all(len(ev_full[n]) == 0 for n in CLS_NAMES) and len(ev_full["fc1"]) == depth
    assert all(len(ev[n]) == 1 for n in CLS_NAMES)
    assert [len(ev[n]) for n in FULL_NAMES] == [depth - 1, depth - 1, 2 * depth - 1, depth - 1, depth - 1]


def test_vit_fc1_events_per_forward(dev):
    """With KERNEL_TIMING["fc1"] = [] one forward appends depth - 1 events (the benchmark divides the full-M fc1 work
    by their mean, so the class-row fc1 must not be among them)."""
    model, size = _model(dev, "direct")
    _, ev = _forward(model, synthetic_images(2, size, seed=4).to(dev), True, ("fc1",))
    assert len(ev["fc1"]) == len(model.blocks) - 1


@pytest.mark.parametrize("name", ["direct", "distilled"])
def test_vit_trace_sees_full_last_block(dev, name):
    """With CODE_TRACE set the whole last block runs: every traced layer of it holds B * N rows, and the logits are
    the same bits."""
    model, size = _model(dev, name)
    img = synthetic_images(2, size, seed=4).to(dev)
    ref, _ = _forward(model, img, False)
    assert vit_model.LAST_BLOCK_CLS_ONLY, "the switch defaults to on"
    ql.CODE_TRACE = {}
    try:
        with torch.no_grad():
            out = model(img)
        trace = ql.CODE_TRACE
    finally:
        ql.CODE_TRACE = None
    M = 2 * (model.patch_embed.num_patches + model.num_tokens)
    blk = model.blocks[-1]
    for layer in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
        assert trace[layer].shape[0] == M
    assert torch.equal(out.cpu().view(torch.int32), ref.view(torch.int32))
