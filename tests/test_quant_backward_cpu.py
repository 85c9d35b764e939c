"""The quantizer backward without a GPU: the restatement (tests/quant_backward_ref.py) against the reference's
known answer, the reference's own float32 arithmetic against the error bound the GPU tests use, and the
argument validation of the new C-ABI exports (rejected before any launch)."""
import ctypes

import pytest
import torch

import quant_backward_ref as R
from quantized_vit_amd import _lib, build

PARAM_SETS, CLIPS, SIZES = R.PARAM_SETS, R.CLIPS, R.SIZES


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dge_known_answer(dtype):
    """The reference's test_dge_quantizer (tests/quantization/test_quant_layers.py:80-112): x = 0.3, d = 0.2,
    q_m = 1, k = 5 gives grad_x = (1/5) |0.3 - 0.1|^(1/5 - 1) = 0.2^0.2, at allclose's defaults."""
    x, g = torch.tensor([0.3]), torch.tensor([1.0])
    r = R.quant_backward_ref(x, g, R.LINEAR, 0.2, 1.0, clip=(-1.0, 1.0), dge_k=5.0, dtype=dtype)
    assert torch.allclose(r["grad_x"].float(), torch.tensor([0.2 ** 0.2]))
    # the forward is the plain quantizer: d * round(x / d)
    y = R.quant_forward_ref(x, R.LINEAR, 0.2, 1.0, dtype=dtype)
    assert torch.allclose(y.float(), torch.tensor([0.2]) * torch.round(x / 0.2))
    # d_quant and q_m still get their straight-through sums: sgn (rne(1.5) - 1.5) = 0.5 and 0 (|x| < q_m)
    assert float(r["sums"][0]) == pytest.approx(0.5, abs=1e-6) and float(r["sums"][1]) == 0.0


def test_masks_select():
    """x = 0 under the nonlinear quantizer computes 0 * -inf before the mask: no NaN may reach a sum; a NaN in
    grad_out must."""
    x = torch.tensor([0.0, -0.0, 0.11, 0.5])
    g = torch.tensor([1.0, -2.0, 0.5, 0.25])
    for dtype in (torch.float64, torch.float32):
        r = R.quant_backward_ref(x, g, R.NONLINEAR, 0.05, 0.37, 0.9, dtype=dtype)
        assert all(torch.isfinite(s) for s in r["sums"])
        gn = g.clone()
        gn[2] = float("nan")
        rn = R.quant_backward_ref(x, gn, R.NONLINEAR, 0.05, 0.37, 0.9, dtype=dtype)
        assert all(torch.isnan(s) for s in rn["sums"])


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("params", PARAM_SETS, ids=lambda p: f"{p[0]}-qm{p[2]}-t{p[3]}")
def test_reference_float32_meets_the_bound(params, clip):
    """|ref32 - ref64| <= 4 floor on the tie-free inputs: the reference's own float32 arithmetic stays inside
    the floor, so the GPU bound 4 max(|ref32 - ref64|, floor) asks nothing of the kernel that the reference
    does not deliver.
    Measured |ref32 - ref64| / floor over these cases (largest per sum): d 0.13, q_m 0.017, t 0.003; the floor's
    c needs no raise."""
    kind, d, q_m, t = params
    worst = [0.0, 0.0, 0.0]
    for n in SIZES:
        x, g = R.make_inputs(n, kind, d, q_m, t, clip)
        r64, r32, floor, _ = R.sum_bounds(x, g, kind, d, q_m, t, clip)
        assert floor > 0.0
        # grad_x is a masked copy: identical in both precisions
        assert torch.equal(r32["grad_x"], r64["grad_x"].float())
        for i in range(3):
            err = abs(float(r32["sums"][i]) - float(r64["sums"][i]))
            worst[i] = max(worst[i], err / floor)
            print(f"n={n} sum{i}: ref64 {float(r64['sums'][i]):+.6e} |ref32-ref64| {err:.3e} floor {floor:.3e}")
            assert err <= 4.0 * floor, (n, i, err, floor)
    print("worst |ref32 - ref64| / floor:", worst)


def test_inputs_hold_every_region():
    x, _ = R.make_inputs(4099, R.LINEAR, 0.05, 0.37, None, (-0.2, 0.3))
    a = x.abs()
    assert (a == 0).sum() >= 2 and (a == torch.tensor(0.37)).sum() >= 2
    assert ((a > 0) & (a < 0.37)).any() and (a > 0.37).any()
    assert (x == 0.3).any() and (x == -0.2).any() and (x > 0.3).any() and (x < -0.2).any()
    assert ((x > -0.2) & (x < 0.3) & (a > 0)).any()


# ---- C-ABI ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_workspace_bytes(lib):
    ws = lib.qvit_quant_backward_workspace_bytes
    assert ws(-1) == -1
    assert ws(0) > 0 and ws(0) % 8 == 0
    assert ws(1) == ws(0)
    big = ws(1 << 40)
    assert ws(1 << 20) <= big == ws(1 << 41)   # the grid is capped: so is the workspace
    assert all(ws(n) <= ws(n + 1) for n in (0, 1023, 1024, 4099, (1 << 20) - 1))


def test_argument_validation_without_launch(lib):
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: validation rejects before any launch
    odd = ctypes.c_void_p(0x1008)
    n = 4099
    nbytes = lib.qvit_quant_backward_workspace_bytes(n)

    def call(x=fake, g=fake, n=n, qtype=_lib.QT_LINEAR, d=fake, qm=fake, t=None, k=0.0, gx=fake, sc=fake, ws=fake,
             wsb=nbytes):
        return lib.qvit_quant_backward(x, g, n, qtype, d, qm, t, -2.0, 2.0, k, gx, sc, ws, wsb, None)

    for name in ("x", "g", "gx", "sc", "d", "qm", "ws"):
        assert call(**{name: None}) == -3, name
    assert call(qtype=_lib.QT_NONLINEAR, t=None) == -3
    assert call(n=-1) == -1
    assert call(qtype=_lib.QT_ULTRA_ACT) == -1
    assert call(qtype=7) == -1
    assert call(qtype=_lib.QT_NONLINEAR, t=fake, k=5.0) == -1    # DGE has the linear forward only
    assert call(k=-1.0) == -1
    assert call(k=float("nan")) == -1
    assert call(wsb=nbytes - 1) == -1
    assert call(wsb=0) == -1
    for name in ("x", "g", "gx"):
        assert call(**{name: odd}) == -2, name
