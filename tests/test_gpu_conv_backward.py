"""qvit_col2im_quant_backward on the device: the fold against the float64 references of tests/conv_backward_ref.py on
the 16-case geometry table, the 16-byte arm against the scalar arm, the 64-bit instantiation, and the fused mode
against qvit_quant_backward applied to the fold's own output.

Bars: integer P (|v| <= 1024, at most kh kw <= 1024 taps: every partial sum below 2^24) bit for bit; N(0, 1) P within
kh kw 2^-24 fold(|P|) elementwise (a sequential fp32 sum of at most kh kw terms); grad_x of the fused mode bit for bit
(the quantizer backward only masks grad_out); its three sums within quant_backward_ref.sum_bounds."""
import pytest
import torch

import conv_backward_ref as CB
import conv_geometry_ref as G
import quant_backward_ref as R

pytestmark = pytest.mark.gpu

BY_ID = dict(zip(G.CASE_IDS, G.CASES))
QT = {R.LINEAR: 0, R.NONLINEAR: 1}
# (kind, d, q_m, t) of quant_backward_ref.PARAM_SETS and the clip inside the inputs' range: tie_free_values runs to
# d (L + 2.45) = 0.47, past saturation (0.37) and past the clip on both sides
FUSED_PARAMS = [R.PARAM_SETS[0], R.PARAM_SETS[4]]
CLIP = R.CLIPS[1]
# vec arm (F4 the patch embedding, F1 with overlapping rows), scalar arm (A1 all asymmetric, G6 dilated columns)
FUSED_CASES = ["F4", "F1", "A1", "G6"]


def _geom(case):
    return case.k, case.s, case.p, case.d


def _vec_arm(case, ldp):
    """The header's conditions of the 16-byte arm (pointers aside)."""
    return (case.p[1] == 0 and case.d[1] == 1 and case.k[1] % 4 == 0 and case.s[1] % 4 == 0
            and case.s[1] >= case.k[1] and case.W % 4 == 0 and ldp % 4 == 0)


def _on_device(t, dev, shifted=False):
    """t on the device, 16-byte aligned, or starting 4 bytes into a larger buffer."""
    if not shifted:
        td = t.to(dev)
        assert td.data_ptr() % 16 == 0
        return td
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    td = base[1:].view(t.shape)
    td.copy_(t)
    assert td.is_contiguous() and td.data_ptr() % 16 == 4
    return td


def _fold(Pd, case, **kw):
    from quantized_vit_amd import _lib
    out, scal = _lib.col2im_quant_backward(Pd, None, case.xshape, *_geom(case), **kw)
    assert scal is None
    return out


def _fused(dev, Pd, xd, case, params, clip=CLIP, **kw):
    from quantized_vit_amd import _lib
    kind, d, q_m, t = params
    f = lambda v: None if v is None else torch.tensor([v], dtype=torch.float32, device=dev)
    return _lib.col2im_quant_backward(Pd, xd, case.xshape, *_geom(case), QT[kind], f(d), f(q_m), f(t), clip[0], clip[1],
                                      **kw)


# ---- fold only ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES, ids=G.CASE_IDS)
def test_fold_geometry(dev, case):
    i = G.CASE_IDS.index(case.id)
    unread = CB.tap_counts(case) == 0
    Pi = CB.make_rows(case, seed=i, integer=True)
    got = _fold(_on_device(Pi, dev, case.shifted), case).cpu()
    assert torch.equal(got.double(), CB.fold_ref(Pi, case))                  # exact sums: bit for bit
    Pn = CB.make_rows(case, seed=100 + i)
    # a row stride past K, its padding columns poisoned: they are never read
    ldp = (case.K + 3) // 4 * 4 + 4
    buf = torch.full((case.rows, ldp), float("nan"), dtype=torch.float32)
    buf[:, :case.K] = Pn
    got = _fold(_on_device(buf, dev, case.shifted)[:, :case.K], case).cpu()
    ref = CB.fold_ref(Pn, case)
    bound = case.k[0] * case.k[1] * 2.0 ** -24 * CB.fold_ref(Pn.abs(), case)
    err = (got.double() - ref).abs()
    print(f"{case.id}: vec arm {_vec_arm(case, ldp) and not case.shifted}, max err {float(err.max()):.3e}, "
          f"worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, unread {int(unread.sum())}")
    assert bool((err <= bound).all())
    assert bool((got[unread] == 0).all()) and not bool(torch.isnan(got).any())   # no tap: exactly 0


def test_unread_elements_are_zero_in_a_dirty_output(dev):
    """F4's trailing columns and A6's skipped pixels are written (as zeros), not left as they were."""
    for cid in ("F4", "A6"):
        case = BY_ID[cid]
        P = CB.make_rows(case, seed=3)
        out = torch.full(case.xshape, float("nan"), dtype=torch.float32, device=dev)
        got = _fold(P.to(dev), case, grad_x=out).cpu()
        unread = CB.tap_counts(case) == 0
        assert bool(unread.any()) and bool((got[unread] == 0).all()) and not bool(torch.isnan(got).any())


@pytest.mark.parametrize("cid", [c.id for c in G.CASES if c.fast])
def test_vec_arm_equals_scalar_arm(dev, cid):
    """The same call on a 16-byte aligned P and on a P shifted by 4 bytes (which takes the scalar arm), fold only
    and fused: identical bits. F1 and F4 meet the 16-byte arm's conditions when aligned; F2 and F3 (sw < kw: kernel
    columns overlap) take the scalar arm both times."""
    case = BY_ID[cid]
    assert _vec_arm(case, case.K) == (cid in ("F1", "F4"))
    P = CB.make_rows(case, seed=11)
    Pa, Ps = _on_device(P, dev), _on_device(P, dev, shifted=True)
    a, s = _fold(Pa, case), _fold(Ps, case)
    assert torch.equal(a.view(torch.int32), s.view(torch.int32))
    for params in FUSED_PARAMS:
        x = R.tie_free_values(case.xshape, *params, seed=12).to(dev)
        ga, _ = _fused(dev, Pa, x, case, params)
        gs, _ = _fused(dev, Ps, x, case, params)
        gx, _ = _fused(dev, Pa, _on_device(x.cpu(), dev, shifted=True), case, params)   # a shifted x alone
        assert torch.equal(ga.view(torch.int32), gs.view(torch.int32))
        assert torch.equal(ga.view(torch.int32), gx.view(torch.int32))


def test_int64_arm(dev):
    """M ldp == 2^31 takes the 64-bit instantiation; the same rows in a compact P take the 32-bit one. P's 8 GiB are
    never initialised: only the K valid columns of each row are written."""
    case, ldp = G.INT64_CASE, G.INT64_LDC
    P = CB.make_rows(case, seed=21)
    compact = P.to(dev)
    want = _fold(compact, case)
    x = R.tie_free_values(case.xshape, *FUSED_PARAMS[0], seed=22).to(dev)
    want_gx, want_sc = _fused(dev, compact, x, case, FUSED_PARAMS[0])
    big = torch.empty((case.rows - 1) * ldp + case.K, dtype=torch.float32, device=dev)
    wide = torch.as_strided(big, (case.rows, case.K), (ldp, 1))
    try:
        assert wide.stride(0) * case.rows == 2 ** 31
        wide.copy_(compact)
        got = _fold(wide, case)
        got_gx, got_sc = _fused(dev, wide, x, case, FUSED_PARAMS[0])
        torch.cuda.synchronize()
    finally:
        del wide, big
        torch.cuda.empty_cache()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got_gx.view(torch.int32), want_gx.view(torch.int32))
    assert torch.equal(got_sc.view(torch.int32), want_sc.view(torch.int32))
    err = (want.cpu().double() - CB.fold_ref(P, case)).abs()
    assert bool((err <= case.k[0] * case.k[1] * 2.0 ** -24 * CB.fold_ref(P.abs(), case)).all())


# ---- fused with the quantizer backward ------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", FUSED_CASES)
@pytest.mark.parametrize("params", FUSED_PARAMS, ids=lambda p: p[0])
def test_fused_mode(dev, params, cid):
    from quantized_vit_amd import _lib
    kind, d, q_m, t = params
    case = BY_ID[cid]
    assert _vec_arm(case, case.K) == (cid in ("F4", "F1"))
    P = CB.make_rows(case, seed=31 + FUSED_CASES.index(cid)).to(dev)
    x = R.tie_free_values(case.xshape, kind, d, q_m, t, seed=41)
    assert float(x.max()) > CLIP[1] and float(x.min()) < CLIP[0] and float(x.abs().max()) > abs(q_m)
    xd = x.to(dev)
    gq = _fold(P, case)
    gx, scal = _fused(dev, P, xd, case, params)
    f = lambda v: None if v is None else torch.tensor([v], dtype=torch.float32, device=dev)
    want_gx, _ = _lib.quant_backward(xd, gq, QT[kind], f(d), f(q_m), f(t), CLIP[0], CLIP[1])
    assert torch.equal(gx.view(torch.int32), want_gx.view(xd.shape).view(torch.int32))
    assert 0 < int((gx == 0).sum()) < gx.numel()
    r64, r32, floor, bounds = R.sum_bounds(x.reshape(-1), gq.cpu().reshape(-1), kind, d, q_m, t, CLIP)
    got = scal.cpu().double().tolist()
    for i, name in enumerate(("d", "q_m", "t")):
        err = abs(got[i] - float(r64["sums"][i]))
        print(f"{cid} {kind} grad_{name}: got {got[i]:+.6e} ref64 {float(r64['sums'][i]):+.6e} err {err:.3e} "
              f"bound {bounds[i]:.3e} floor {floor:.3e}")
        assert err <= bounds[i], (name, err, bounds[i])
    if kind == R.LINEAR:
        assert got[2] == 0.0
    # two calls, and a workspace and an output that held NaN: the same bits
    query = _lib.load().qvit_col2im_quant_backward_workspace_bytes
    nbytes = int(query(*case.xshape, *case.k, *case.s, *case.p, *case.d))
    assert nbytes > 0
    dirty = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device=dev)
    out = torch.full(case.xshape, float("nan"), dtype=torch.float32, device=dev)
    gx2, scal2 = _fused(dev, P, xd, case, params, workspace=dirty, grad_x=out)
    assert gx2.data_ptr() == out.data_ptr()
    assert torch.equal(gx2.view(torch.int32), gx.view(torch.int32))
    assert torch.equal(scal2.view(torch.int32), scal.view(torch.int32))


@pytest.mark.parametrize("cid", ["F4", "A1"])
def test_nan_in_p_reaches_its_taps_and_the_sums(dev, cid):
    """One NaN in P: NaN in exactly the image elements that add that entry (one, here inside the clip range, where
    grad_out passes), NaN in the d_quant sum. An entry on the zero padding (A1's top taps) reaches nothing."""
    params = FUSED_PARAMS[0]
    case = BY_ID[cid]
    P = CB.make_rows(case, seed=51)
    x = R.tie_free_values(case.xshape, *params, seed=52)
    inside = ((x > CLIP[0]) & (x < CLIP[1])).reshape(-1)
    hit = None
    for r in range(case.rows // 2, case.rows):
        taps = CB.tap_elements(case, r, case.K // 2)
        if taps.numel() == 1 and bool(inside[taps[0]]):
            hit = (r, case.K // 2, taps)
            break
    assert hit is not None
    Pn = P.clone()
    Pn[hit[0], hit[1]] = float("nan")
    gx, scal = _fused(dev, Pn.to(dev), x.to(dev), case, params)
    assert torch.equal(torch.isnan(gx.cpu()).reshape(-1).nonzero().reshape(-1), hit[2])
    assert bool(torch.isnan(scal[0]))
    if cid == "A1":   # row 0 is output (0, 0, 0): its ky = 0 taps lie on the top padding
        assert CB.tap_elements(case, 0, 0).numel() == 0
        Pn = P.clone()
        Pn[0, 0] = float("nan")
        gx, scal = _fused(dev, Pn.to(dev), x.to(dev), case, params)
        assert not bool(torch.isnan(gx).any()) and not bool(torch.isnan(scal).any())
