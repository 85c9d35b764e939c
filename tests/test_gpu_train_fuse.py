"""The train-fusion kernels on the device (qvit_layernorm_quant_backward, qvit_gelu_quant_i8,
qvit_gelu_quant_backward) against the float64 restatements of tests/train_fuse_ref.py, on inputs that keep their
distance from every branch point (tests/test_train_fuse_cpu.py checks that >= 90 % of the drawn rows survive).

Pass criteria: grad_x is zero exactly where the reference's clip mask covers a whole term (GELU: the element;
LayerNorm mixes a row, so there the mask shows in gy, through grad_beta); elsewhere, and for the column and scalar
sums, |got - ref64| <= C max(|ref32 - ref64|, floor) with the floors of train_fuse_ref. C is the smallest power of
two at least twice the worst ratio measured on the MI355X: C_LN = 2 (worst ratio 0.963,
grad_beta of the 5 x 1024 case), C_GELU = 4 (worst 1.526, grad_h at n = 2101251, nonlinear)."""
import pytest
import torch

import quant_backward_ref as R
import train_fuse_ref as T
from footprint_tools import Arena
from quant_backward_ref import CLIPS

pytestmark = pytest.mark.gpu

C_LN, C_GELU = 2.0, 4.0
QT = {R.LINEAR: 0, R.NONLINEAR: 1}
EALIGN = -2
_ids = lambda p: f"{p[0]}-t{p[3]}"


def _dev_params(dev, d, q_m, t):
    f = lambda v: None if v is None else torch.tensor([v], dtype=torch.float32, device=dev)
    return f(d), f(q_m), f(t)


def _ln(dev, x, gamma, beta, g, params, clip, **kw):
    from quantized_vit_amd import _lib
    kind, d, q_m, t = params
    dd, dq, dt = _dev_params(dev, d, q_m, t)
    return _lib.layernorm_quant_backward(x, gamma, beta, T.LN_EPS, QT[kind], dd, dq, dt, clip[0], clip[1], g, **kw)


def _check(name, got, ref64, ref32, floor, c, worst):
    err = (got.double().cpu() - ref64).abs()
    bound = torch.maximum((ref32.double() - ref64).abs(), floor)
    ratio = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    worst[name] = max(worst.get(name, 0.0), ratio)
    assert bool((err <= c * bound).all()), (name, ratio)


def _ln_case(dev, rows, cols, params, clip):
    kind, d, q_m, t = params
    x, gamma, beta, g, _ = T.ln_inputs(rows, cols, kind, d, q_m, t, clip)
    r64 = T.ln_quant_backward_ref(x, gamma, beta, g, kind, d, q_m, t, clip)
    r32 = T.ln_quant_backward_ref(x, gamma, beta, g, kind, d, q_m, t, clip, dtype=torch.float32)
    return (x, gamma, beta, g), r64, r32


def _ln_compare(out, ops, r64, r32, params, worst, cols_wanted=True):
    kind, d, q_m, t = params
    x, gamma, beta, g = ops
    gx, gg, gb, scal = out
    _check("grad_x", gx, r64["grad_x"], r32["grad_x"], T.ln_grad_x_floor(r64, gamma), C_LN, worst)
    if cols_wanted:
        fg, fb = T.ln_col_floors(r64)
        _check("grad_gamma", gg, r64["grad_gamma"], r32["grad_gamma"], fg, C_LN, worst)
        _check("grad_beta", gb, r64["grad_beta"], r32["grad_beta"], fb, C_LN, worst)
    fl = T.sum_floors(r64, g, kind, d, q_m, t, T.ln_input_delta(r64, gamma, beta))
    for i, name in enumerate(("d", "q_m", "t")):
        _check(f"sum_{name}", scal[i:i + 1], r64["sums"][i].reshape(1), r32["sums"][i].reshape(1),
               torch.tensor([fl[i]], dtype=torch.float64), C_LN, worst)
    if kind == R.LINEAR:
        assert float(scal[2]) == 0.0


@pytest.mark.parametrize("shape", T.LN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("params", T.QUANTIZERS, ids=_ids)
def test_layernorm_backward(dev, params, shape):
    """Every shape with both quantizers: the wide clip, a clip interval that masks an interior share, and NULL
    grad_gamma / grad_beta (same grad_x and sums, bit for bit)."""
    rows, cols = shape
    worst = {}
    for clip in CLIPS:
        ops, r64, r32 = _ln_case(dev, rows, cols, params, clip)
        dops = [v.to(dev) for v in ops]
        out = _ln(dev, *dops, params, clip)
        _ln_compare(out, ops, r64, r32, params, worst)
        if clip == CLIPS[1]:
            masked = int(r64["masked"].sum())
            assert 0 < masked < rows * cols or rows * cols <= 4
            # a column whose every row is masked gets an exact zero; gy is zero exactly where the reference masks
            allm = r64["masked"].all(0)
            assert bool((out[2].cpu()[allm] == 0).all()) and bool((out[1].cpu()[allm] == 0).all())
        bare = _ln(dev, *dops, params, clip, want_gamma=False, want_beta=False)
        assert bare[1] is None and bare[2] is None
        assert torch.equal(bare[0], out[0]) and torch.equal(bare[3].view(torch.int32), out[3].view(torch.int32))
    print(f"ln {rows}x{cols} {params[0]}: worst ratios " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f" (C_LN = {C_LN})")


def test_layernorm_backward_masks_whole_rows_exactly(dev):
    """A clip interval no value reaches from inside: every gy is zero, so grad_x, grad_gamma and grad_beta are
    exact zeros while the scalar sums still see every element."""
    params, clip = T.QUANTIZERS[0], (-1e-9, 1e-9)
    ops, r64, _ = _ln_case(dev, 5, 64, params, CLIPS[0])
    gx, gg, gb, scal = _ln(dev, *[v.to(dev) for v in ops], params, clip)
    assert float(gx.abs().max()) == 0.0 and float(gg.abs().max()) == 0.0 and float(gb.abs().max()) == 0.0
    assert float(scal[0]) != 0.0


@pytest.mark.parametrize("shape", [(5, 64), (3, 260), (7, 768), (3, 1280)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_layernorm_backward_in_a_poisoned_arena(dev, shape):
    """ldx, ldg, ldo > cols inside the poisoned arena: nothing outside the outputs changes, and the result equals
    the tight-buffer result bit for bit."""
    from quantized_vit_amd import _lib
    rows, cols = shape
    params, clip = T.QUANTIZERS[1], CLIPS[1]
    ops, _, _ = _ln_case(dev, rows, cols, params, clip)
    x, gamma, beta, g = [v.to(dev) for v in ops]
    tight = _ln(dev, x, gamma, beta, g, params, clip)
    kind, d, q_m, t = params
    dd, dq, dt = _dev_params(dev, d, q_m, t)
    lib = _lib.load()
    nbytes = int(lib.qvit_layernorm_quant_backward_workspace_bytes(rows, cols))
    ar = Arena(dev, 16 * (rows + 8) * (cols + 64) + nbytes + 8192)
    ax = ar.put(x, ld=cols + 12, name="x")
    ag = ar.put(g, ld=cols + 4, name="grad_y")
    agam, abet = ar.put(gamma, name="gamma"), ar.put(beta, name="beta")
    ao = ar.carve(rows, cols, cols + 8, torch.float32, writable=True, name="grad_x")
    agg = ar.carve_flat(cols, torch.float32, writable=True, name="grad_gamma")
    agb = ar.carve_flat(cols, torch.float32, writable=True, name="grad_beta")
    asc = ar.carve_flat(3, torch.float32, misalign=4, writable=True, name="scalars")
    aws = ar.carve_flat(nbytes // 4, torch.float32, writable=True, name="workspace")
    ar.seal()
    rc = lib.qvit_layernorm_quant_backward(ax.data_ptr(), rows, cols, ax.stride(0), agam.data_ptr(), abet.data_ptr(),
                                           T.LN_EPS, QT[kind], dd.data_ptr(), dq.data_ptr(), dt.data_ptr(), clip[0],
                                           clip[1], ag.data_ptr(), ag.stride(0), ao.data_ptr(), ao.stride(0),
                                           agg.data_ptr(), agb.data_ptr(), asc.data_ptr(), aws.data_ptr(), nbytes,
                                           torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    ar.assert_untouched()
    i32 = lambda v: v.contiguous().view(torch.int32)
    assert torch.equal(i32(ao), i32(tight[0])) and torch.equal(i32(agg), i32(tight[1]))
    assert torch.equal(i32(agb), i32(tight[2])) and torch.equal(i32(asc), i32(tight[3]))


@pytest.mark.parametrize("params", T.QUANTIZERS, ids=_ids)
def test_layernorm_backward_deterministic_aliased_nan(dev, params):
    rows, cols = T.LN_SHAPES[-1]   # more than one trip of every wave
    clip = CLIPS[0]
    ops, _, _ = _ln_case(dev, rows, cols, params, clip)
    x, gamma, beta, g = [v.to(dev) for v in ops]
    a = _ln(dev, x, gamma, beta, g, params, clip)
    b = _ln(dev, x, gamma, beta, g, params, clip)
    i32 = lambda v: v.view(torch.int32)
    for u, v in zip(a, b):
        assert torch.equal(i32(u), i32(v))
    alias = g.clone()
    c = _ln(dev, x, gamma, beta, alias, params, clip, grad_x=alias)
    assert c[0].data_ptr() == alias.data_ptr()
    for u, v in zip(a, c):
        assert torch.equal(i32(u), i32(v))
    # a NaN in one grad_y element: the scalar sums, and its own row of grad_x only
    gn = g.clone()
    gn[3, 5] = float("nan")
    n = _ln(dev, x, gamma, beta, gn, params, clip)
    assert bool(torch.isnan(n[3][0])) and bool(torch.isnan(n[0][3]).all())
    rest = torch.ones(rows, dtype=torch.bool, device=dev)
    rest[3] = False
    assert torch.equal(i32(n[0][rest]), i32(a[0][rest]))
    cols_ok = torch.ones(cols, dtype=torch.bool, device=dev)
    cols_ok[5] = False
    assert bool(torch.isnan(n[1][5])) and bool(torch.isnan(n[2][5]))
    assert torch.equal(i32(n[1][cols_ok]), i32(a[1][cols_ok])) and torch.equal(i32(n[2][cols_ok]), i32(a[2][cols_ok]))


def test_layernorm_backward_empty_and_misaligned(dev):
    from quantized_vit_amd import _lib
    lib = _lib.load()
    dd, dq, _ = _dev_params(dev, 0.05, 0.37, None)
    st = torch.cuda.current_stream(dev).cuda_stream
    buf = torch.zeros(64, device=dev)
    gam, bet = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    gg, gb = torch.full((8,), 7.0, device=dev), torch.full((8,), 7.0, device=dev)
    scal = torch.full((3,), 7.0, device=dev)
    nb = int(lib.qvit_layernorm_quant_backward_workspace_bytes(0, 8))
    ws = torch.empty(nb // 8 + 1, dtype=torch.float64, device=dev)
    call = lambda rows, cols, ld, out, g=buf: lib.qvit_layernorm_quant_backward(
        buf.data_ptr(), rows, cols, ld, gam.data_ptr(), bet.data_ptr(), 1e-6, 0, dd.data_ptr(), dq.data_ptr(), None,
        -2.0, 2.0, g.data_ptr(), ld, out.data_ptr(), ld, gg.data_ptr(), gb.data_ptr(), scal.data_ptr(), ws.data_ptr(),
        ws.numel() * 8, st)
    assert call(0, 8, 8, buf) == 0
    assert scal.cpu().tolist() == [0.0] * 3 and gg.cpu().tolist() == [0.0] * 8 and gb.cpu().tolist() == [0.0] * 8
    # misaligned: QVIT_EALIGN and nothing written
    out = torch.full((64,), 5.0, device=dev)
    scal.fill_(7.0)
    gg.fill_(7.0)
    assert call(1, 6, 8, out) == EALIGN                       # cols % 4
    assert call(1, 4, 6, out) == EALIGN                       # leading dimensions % 4
    assert call(1, 4, 8, out[1:]) == EALIGN                   # grad_x off 16 bytes
    assert call(1, 4, 8, out, g=buf[1:]) == EALIGN            # grad_y off 16 bytes
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and scal.cpu().tolist() == [7.0] * 3 and bool((gg == 7.0).all())


# ---- GELU ---------------------------------------------------------------------------------------------------------
def _gelu_bwd(dev, h, g, params, clip, **kw):
    from quantized_vit_amd import _lib
    kind, d, q_m, t = params
    dd, dq, dt = _dev_params(dev, d, q_m, t)
    return _lib.gelu_quant_backward(h, g, QT[kind], dd, dq, dt, clip[0], clip[1], **kw)


@pytest.mark.parametrize("shape", [(1, 1), (3, 63), (5, 64), (7, 65), (4, 1023), (257, 4099 // 7)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("params", T.QUANTIZERS, ids=_ids)
def test_gelu_quant_codes_bit_equal(dev, params, shape):
    """codes == quantize_act_i8(gelu_f32(h)) byte for byte, zero fill of [cols, kpad), nothing past kpad; h spans
    +-6 and includes values next to the quantizer's ties (no filter here: both sides run the same functions)."""
    from quantized_vit_amd import _lib
    kind, d, q_m, t = params
    dd, dq, dt = _dev_params(dev, d, q_m, t)
    rows, cols = shape
    gen = torch.Generator().manual_seed(rows * 131 + cols)
    ld = cols + (4 if cols % 2 == 0 else 3)   # even widths take the 16-byte loads, odd ones the scalar path
    hbuf = ((torch.rand(rows, ld, generator=gen) * 12.0 - 6.0).float()).to(dev)
    h = hbuf[:, :cols]
    kpad = (cols + 15) // 16 * 16
    got = torch.full((rows, kpad + 16), 99, dtype=torch.int8, device=dev)
    ref = torch.full((rows, kpad + 16), 99, dtype=torch.int8, device=dev)
    _lib.gelu_quant_i8(h, QT[kind], dd, dq, dt, 0, got, kpad)
    a = _lib.gelu_f32(h.contiguous()).view(rows, cols)
    _lib.quantize_act_i8(a, QT[kind], dd, dq, dt, 0, ref, kpad)
    assert torch.equal(got, ref)
    assert bool((got[:, cols:kpad] == 0).all()) and bool((got[:, kpad:] == 99).all())
    assert int(got[:, :cols].abs().max()) > 0 or cols * rows < 4


@pytest.mark.parametrize("n", T.GELU_SIZES)
@pytest.mark.parametrize("params", T.QUANTIZERS, ids=_ids)
def test_gelu_backward(dev, params, n):
    kind, d, q_m, t = params
    clip = CLIPS[1] if n % 2 else CLIPS[0]   # the odd sizes run the clip interval that masks an interior share
    h, g, _ = T.gelu_inputs(n, kind, d, q_m, t, clip)
    r64 = T.gelu_quant_backward_ref(h, g, kind, d, q_m, t, clip)
    r32 = T.gelu_quant_backward_ref(h, g, kind, d, q_m, t, clip, dtype=torch.float32)
    gh, scal = _gelu_bwd(dev, h.to(dev), g.to(dev), params, clip)
    worst = {}
    assert bool((gh.cpu()[r64["masked"]] == 0).all())          # zero exactly where the reference masks
    if clip == CLIPS[1] and n > 64:
        assert 0 < int(r64["masked"].sum()) < n
    _check("grad_h", gh, r64["grad_h"], r32["grad_h"], T.gelu_grad_h_floor(r64, h), C_GELU, worst)
    fl = T.sum_floors(r64, g, kind, d, q_m, t, T.gelu_input_delta(r64, h))
    for i, name in enumerate(("d", "q_m", "t")):
        _check(f"sum_{name}", scal[i:i + 1], r64["sums"][i].reshape(1), r32["sums"][i].reshape(1),
               torch.tensor([fl[i]], dtype=torch.float64), C_GELU, worst)
    print(f"gelu n={n} {kind}: worst ratios " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f" (C_GELU = {C_GELU})")


@pytest.mark.parametrize("params", T.QUANTIZERS, ids=_ids)
def test_gelu_backward_deterministic_aliased_nan(dev, params):
    kind, d, q_m, t = params
    clip, n = CLIPS[0], 1024 * 256 * 4 + 4099
    h, g, _ = T.gelu_inputs(n, kind, d, q_m, t, clip)
    hd, gd = h.to(dev), g.to(dev)
    i32 = lambda v: v.view(torch.int32)
    g1, s1 = _gelu_bwd(dev, hd, gd, params, clip)
    g2, s2 = _gelu_bwd(dev, hd, gd, params, clip)
    assert torch.equal(i32(g1), i32(g2)) and torch.equal(i32(s1), i32(s2))
    alias = gd.clone()
    g3, s3 = _gelu_bwd(dev, hd, alias, params, clip, grad_h=alias)
    assert g3.data_ptr() == alias.data_ptr()
    assert torch.equal(i32(g3), i32(g1)) and torch.equal(i32(s3), i32(s1))
    gn = gd.clone()
    gn[77] = float("nan")
    g4, s4 = _gelu_bwd(dev, hd, gn, params, clip)
    assert bool(torch.isnan(s4[0])) and bool(torch.isnan(g4[77]))
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    keep[77] = False
    assert torch.equal(i32(g4[keep]), i32(g1[keep]))


def test_gelu_backward_empty_and_misaligned(dev):
    from quantized_vit_amd import _lib
    lib = _lib.load()
    dd, dq, _ = _dev_params(dev, 0.05, 0.37, None)
    st = torch.cuda.current_stream(dev).cuda_stream
    buf = torch.zeros(16, device=dev)
    out = torch.full((16,), 5.0, device=dev)
    scal = torch.full((3,), 7.0, device=dev)
    ws = torch.empty(8, dtype=torch.float64, device=dev)
    call = lambda h, g, n, o: lib.qvit_gelu_quant_backward(h.data_ptr(), g.data_ptr(), n, 0, dd.data_ptr(),
                                                          dq.data_ptr(), None, -2.0, 2.0, o.data_ptr(),
                                                          scal.data_ptr(), ws.data_ptr(), 64, st)
    assert call(buf, buf, 0, out) == 0
    assert scal.cpu().tolist() == [0.0] * 3
    scal.fill_(7.0)
    assert call(buf[1:], buf, 4, out) == EALIGN and call(buf, buf[1:], 4, out) == EALIGN
    assert call(buf, buf, 4, out[1:]) == EALIGN
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and scal.cpu().tolist() == [7.0] * 3
