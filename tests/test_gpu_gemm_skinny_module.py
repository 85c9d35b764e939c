"""quant_layers.GEMM_SKINNY: with the switch on, QuantizeMixin.gemm_codes runs the int path's GEMMs of the modules and
of the fused block on qvit_gemm_skinny, and the logits do not change by a bit."""
import pytest
import torch

from quantized_vit_amd import _lib, quant_layers
from quantized_vit_amd.calibrate import build_quantized_vit, synthetic_images

pytestmark = pytest.mark.gpu


def test_vit_skinny_gemm_bit_identical(dev, monkeypatch):
    model = build_quantized_vit("vit_base_patch16_224", seed=7, depth=2).to(dev)
    img = synthetic_images(2, 224, seed=3).to(dev)
    calls = []
    skinny = _lib.gemm_skinny
    monkeypatch.setattr(_lib, "gemm_skinny", lambda *a, **k: (calls.append(a[1]), skinny(*a, **k))[1])
    # every row count of the B = 2 forward (394 rows, the class-token tail's 2), whatever the measured threshold is
    monkeypatch.setattr(quant_layers, "GEMM_SKINNY_MAX_M", 4096)
    outs = []
    for on in (False, True):
        monkeypatch.setattr(quant_layers, "GEMM_SKINNY", on)
        with torch.no_grad():
            outs.append(model(img).cpu())
        assert bool(calls) == on
    assert torch.equal(outs[0], outs[1])
    assert 2 * 197 in calls
