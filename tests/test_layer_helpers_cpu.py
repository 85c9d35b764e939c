"""The stateless host helpers the layer modules share (_lib.round_up, _lib.backward_ops) and the bit-width
properties of QuantizeMixin behind their one _bit_width, on the CPU: no device, no library."""
import math

import pytest
import torch

from quantized_vit_amd import _lib
from quantized_vit_amd.quant_layers import QuantizationMode, QuantizationType, QuantizeConv2d, QuantizeLinear


@pytest.mark.parametrize("m", [1, 4, 16, 128, 256])
def test_round_up(m):
    assert _lib.round_up(0, m) == 0
    assert _lib.round_up(1, m) == m
    assert _lib.round_up(m - 1, m) == (m if m > 1 else 0)
    assert _lib.round_up(m, m) == m
    assert _lib.round_up(m + 1, m) == 2 * m
    assert isinstance(_lib.round_up(m + 1, m), int)


def test_backward_ops_table():
    assert _lib.BACKWARD_OPS == {"hip": ("dgrad", "wgrad"), "torch": (), "dgrad": ("dgrad",), "wgrad": ("wgrad",)}
    for value, ops in _lib.BACKWARD_OPS.items():
        assert _lib.backward_ops(value, "BACKWARD_GEMM") == ops
        assert _lib.backward_ops(value, "QVIT_BWD_GEMM") == ops


# the messages of the commit before the helper, one per site
@pytest.mark.parametrize("what,text", [
    ("QVIT_BWD_GEMM", "QVIT_BWD_GEMM='cuda': expected hip, torch, dgrad or wgrad"),
    ("QVIT_CONV_BWD_GEMM", "QVIT_CONV_BWD_GEMM='cuda': expected hip, torch, dgrad or wgrad"),
    ("QVIT_ULTRA_BWD", "QVIT_ULTRA_BWD='cuda': expected hip, torch, dgrad or wgrad"),
    ("BACKWARD_GEMM", "BACKWARD_GEMM = 'cuda': expected hip, torch, dgrad or wgrad"),
    ("CONV_BACKWARD_GEMM", "CONV_BACKWARD_GEMM = 'cuda': expected hip, torch, dgrad or wgrad"),
    ("ULTRA_BWD", "ULTRA_BWD = 'cuda': expected hip, torch, dgrad or wgrad"),
])
def test_backward_ops_rejects_with_the_sites_wording(what, text):
    with pytest.raises(ValueError) as e:
        _lib.backward_ops("cuda", what)
    assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        _lib.backward_ops(None, what)
    assert str(e.value) == text.replace("'cuda'", "None")


def test_an_assigned_switch_is_validated_where_it_is_used(monkeypatch):
    from quantized_vit_amd import quant_layers as ql, quant_ultra as qu
    monkeypatch.setattr(ql, "BACKWARD_GEMM", "cuda")
    monkeypatch.setattr(ql, "CONV_BACKWARD_GEMM", "cuda")
    monkeypatch.setattr(qu, "ULTRA_BWD", "cuda")
    for fn, text in ((ql._backward_gemm_ops, "BACKWARD_GEMM = 'cuda'"),
                     (lambda: ql._conv_backward_gemm_ops(False), "CONV_BACKWARD_GEMM = 'cuda'"),
                     (qu._backward_gemm_ops, "ULTRA_BWD = 'cuda'")):
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == text + ": expected hip, torch, dgrad or wgrad"
    # the conv switch unset: the measured default by tap overlap; UltraNet under "hip": wgrad stays on the library
    monkeypatch.setattr(ql, "CONV_BACKWARD_GEMM", None)
    assert ql._conv_backward_gemm_ops(True) == () and ql._conv_backward_gemm_ops(False) == ("dgrad", "wgrad")
    monkeypatch.setattr(qu, "ULTRA_BWD", "hip")
    assert qu._backward_gemm_ops() == ("dgrad",)
    monkeypatch.setattr(qu, "ULTRA_BWD", "wgrad")
    assert qu._backward_gemm_ops() == ("wgrad",)


def _bits(d, qm, t):
    """quant_layers.py:383-410 of the reference: round(log2(|q_m|^t / |d| + 1) + 1)."""
    return round(math.log2(math.exp(t * math.log(abs(qm))) / abs(d) + 1) + 1)


def _layer(cls, qtype, mode):
    if cls is QuantizeLinear:
        return QuantizeLinear(12, 5, quant_type=qtype, quant_mode=mode)
    return QuantizeConv2d(3, 4, 3, quant_type=qtype, quant_mode=mode)


def _set(layer, side, d, qm, t):
    getattr(layer, f"d_quant_{side}").data.fill_(d)
    getattr(layer, f"q_m_{side}").data.fill_(qm)
    if hasattr(layer, f"t_quant_{side}"):
        getattr(layer, f"t_quant_{side}").data.fill_(t)


WT = (0.0371, -0.93, 1.31)      # a negative q_m and d: the properties take magnitudes
ACT = (-0.011, 3.7, 0.83)


@pytest.mark.parametrize("cls", [QuantizeLinear, QuantizeConv2d])
@pytest.mark.parametrize("qtype", [QuantizationType.SYMMETRIC_LINEAR, QuantizationType.SYMMETRIC_NONLINEAR])
def test_bit_widths_follow_the_closed_form(cls, qtype):
    layer = _layer(cls, qtype, QuantizationMode.WEIGHT_AND_ACTIVATION)
    _set(layer, "wt", *WT)
    _set(layer, "act", *ACT)
    f = lambda v: torch.tensor(v, dtype=torch.float32).item()   # the parameters hold fp32
    nonlinear = qtype == QuantizationType.SYMMETRIC_NONLINEAR
    want_w = _bits(f(WT[0]), f(WT[1]), f(WT[2]) if nonlinear else 1.0)
    want_a = _bits(f(ACT[0]), f(ACT[1]), f(ACT[2]) if nonlinear else 1.0)
    assert want_w != want_a
    assert (layer.weight_bit, layer.activation_bit) == (want_w, want_a)
    assert isinstance(layer.weight_bit, int) and isinstance(layer.activation_bit, int)


@pytest.mark.parametrize("bits", [2, 4, 8, 16])
def test_bit_widths_of_an_initialised_layer(bits):
    from quantized_vit_amd.quant_layers import initialize_quant_layer
    layer = _layer(QuantizeLinear, QuantizationType.SYMMETRIC_LINEAR, QuantizationMode.WEIGHT_AND_ACTIVATION)
    initialize_quant_layer(layer, num_bits=bits, quant_mode=QuantizationMode.WEIGHT_AND_ACTIVATION)
    assert (layer.weight_bit, layer.activation_bit) == (bits, bits)


def test_weight_only_mode_reports_32_activation_bits():
    for qtype in (QuantizationType.SYMMETRIC_LINEAR, QuantizationType.SYMMETRIC_NONLINEAR, QuantizationType.DGE):
        assert _layer(QuantizeLinear, qtype, QuantizationMode.WEIGHT_ONLY).activation_bit == 32


def test_dge_has_no_bit_width():
    layer = _layer(QuantizeLinear, QuantizationType.DGE, QuantizationMode.WEIGHT_AND_ACTIVATION)
    with pytest.raises(NotImplementedError):
        layer.weight_bit
    with pytest.raises(NotImplementedError):
        layer.activation_bit
