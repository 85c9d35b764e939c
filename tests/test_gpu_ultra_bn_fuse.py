"""ultra_bn_fuse.hip at kernel level through the C ABI: statistics, forward codes and flag bytes, the two backward
kernels, against the float64 restatement (tests/ultra_bn_fuse_ref.py). Every output sits between guard bands, every
workspace starts NaN-filled, and every case runs on 16-byte aligned tensors and on tensors offset by one element
(the scalar arm)."""
import pytest
import torch

import ultra_bn_fuse_ref as R
from ultra_ref import assert_codes_tie_proven
from quantized_vit_amd import _lib

pytestmark = pytest.mark.gpu

EPS = float(torch.finfo(torch.float32).eps)
BN_EPS = 1e-5
GUARD = 64
SENTINEL = {torch.float32: -12345.0, torch.float64: -12345.0, torch.uint8: 0xA5}


class Guarded:
    """A tensor inside a larger buffer: GUARD sentinel elements on both sides, `off` more in front (off = 1 breaks
    the 16-byte alignment)."""

    def __init__(self, shape, dtype, dev, off=0, src=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD + off,), SENTINEL[dtype], dtype=dtype, device=dev)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.buf[self.lo:self.hi].view(shape)
        if src is not None:
            self.t.copy_(src)

    def intact(self) -> bool:
        s = SENTINEL[self.buf.dtype]
        return bool((self.buf[:self.lo] == s).all()) and bool((self.buf[self.hi:] == s).all())


def _nan_ws(nbytes, dev):
    assert nbytes >= 0
    return torch.full((nbytes // 8 + 1,), float("nan"), dtype=torch.float64, device=dev)


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def dev_stats(x, dev, factor=0.1, running=None, off=0):
    """qvit_bn_stats -> (mean, var, invstd, running_mean, running_var) device tensors; asserts guards and that a
    second call on another NaN workspace gives the same bits."""
    B, C, H, W = x.shape
    lib = _lib.load()
    xg = Guarded(x.shape, torch.float32, dev, off, x)
    res = []
    for _ in range(2):
        outs = [Guarded((C,), torch.float32, dev, off) for _ in range(3)]
        run = [None, None] if running is None else [Guarded((C,), torch.float32, dev, off, r) for r in running]
        nb = int(lib.qvit_bn_stats_workspace_bytes(B, C, H, W))
        ws = _nan_ws(nb, dev)
        rc = lib.qvit_bn_stats(xg.t.data_ptr(), B, C, H, W, BN_EPS, factor,
                               *(None if r is None else r.t.data_ptr() for r in run),
                               *(o.t.data_ptr() for o in outs), ws.data_ptr(), nb, _st(dev))
        assert rc == 0
        torch.cuda.synchronize()
        assert all(o.intact() for o in outs) and all(r is None or r.intact() for r in run) and xg.intact()
        assert bool(torch.isnan(ws[nb // 8:]).all())
        res.append([o.t.clone() for o in outs] + [None if r is None else r.t.clone() for r in run])
    for a, b in zip(*res):
        assert a is None or torch.equal(a, b)
    return res[0]


def dev_forward(x, mean, invstd, gamma, beta, levels, pool, dev, off=0):
    B, C, H, W = x.shape
    oshape = (B, C, H // 2, W // 2) if pool else (B, C, H, W)
    xg = Guarded(x.shape, torch.float32, dev, off, x)
    out, flags = Guarded(oshape, torch.float32, dev, off), Guarded(oshape, torch.uint8, dev, off)
    gm = None if gamma is None else gamma.to(dev)
    bt = None if beta is None else beta.to(dev)
    rc = _lib.load().qvit_bn_act_pool_forward(xg.t.data_ptr(), B, C, H, W, mean.data_ptr(), invstd.data_ptr(),
                                              _lib._ptr(gm), _lib._ptr(bt), levels, int(pool), out.t.data_ptr(),
                                              flags.t.data_ptr(), _st(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert out.intact() and flags.intact() and xg.intact()
    return out.t.clone(), flags.t.clone()


def dev_backward(x, g, flags, mean, invstd, gamma, pool, dev, off=0, want=(True, True)):
    """The two backward kernels -> (dx, dgamma, dbeta, sums); guards, and two calls give the same bits."""
    B, C, H, W = x.shape
    lib = _lib.load()
    xg = Guarded(x.shape, torch.float32, dev, off, x)
    gg = Guarded(g.shape, torch.float32, dev, off, g)
    fg = Guarded(flags.shape, torch.uint8, dev, off, flags)
    gm = None if gamma is None else gamma.to(dev)
    res = []
    for _ in range(2):
        sums = Guarded((2 * C,), torch.float64, dev)
        dx = Guarded(x.shape, torch.float32, dev, off)
        dgamma = Guarded((C,), torch.float32, dev, off) if want[0] else None
        dbeta = Guarded((C,), torch.float32, dev, off) if want[1] else None
        nb = int(lib.qvit_bn_act_pool_backward_workspace_bytes(B, C, H, W, int(pool)))
        ws = _nan_ws(nb, dev)
        rc = lib.qvit_bn_act_pool_backward_reduce(xg.t.data_ptr(), gg.t.data_ptr(), fg.t.data_ptr(), B, C, H, W,
                                                  mean.data_ptr(), invstd.data_ptr(), int(pool), sums.t.data_ptr(),
                                                  ws.data_ptr(), nb, _st(dev))
        assert rc == 0
        rc = lib.qvit_bn_act_pool_backward_dx(xg.t.data_ptr(), gg.t.data_ptr(), fg.t.data_ptr(), B, C, H, W,
                                              mean.data_ptr(), invstd.data_ptr(), _lib._ptr(gm), sums.t.data_ptr(),
                                              int(pool), dx.t.data_ptr(),
                                              None if dgamma is None else dgamma.t.data_ptr(),
                                              None if dbeta is None else dbeta.t.data_ptr(), _st(dev))
        assert rc == 0
        torch.cuda.synchronize()
        for t in (sums, dx, dgamma, dbeta, xg, gg, fg):
            assert t is None or t.intact()
        assert bool(torch.isnan(ws[nb // 8:]).all())
        res.append((dx.t.clone(), None if dgamma is None else dgamma.t.clone(),
                    None if dbeta is None else dbeta.t.clone(), sums.t.clone()))
    for a, b in zip(*res):
        assert a is None or torch.equal(a, b)
    return res[0]


def _within(name, got, ref64, ref32, c, scale=0.0):
    err, err32 = R.rel(got, ref64, scale), R.rel(ref32, ref64, scale)
    ratio = err / max(err32, EPS)
    print(f"{name}: err {err:.3e}, fp32 restatement err {err32:.3e}, ratio {ratio:.3f}")
    assert err <= c * max(err32, EPS), (name, err, err32)
    return ratio


# ---- statistics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_statistics(dev, shape, off):
    x, _, _ = R.gen_case(shape, 15)
    C = shape[1]
    g = torch.Generator().manual_seed(7)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    for factor in (0.1, 1.0 / 3.0):
        mean, var, invstd, rm, rv = dev_stats(x.to(dev), dev, factor, (rm0.to(dev), rv0.to(dev)), off)
        ref64 = R.stats(x, BN_EPS, factor, rm0, rv0)
        ref32 = R.stats(x, BN_EPS, factor, rm0, rv0, dtype=torch.float32)
        for name, got, r64, r32 in zip(("mean", "var", "invstd", "running_mean", "running_var"),
                                       (mean, var, invstd, rm, rv), ref64, ref32):
            _within(f"{shape} off {off} factor {factor:.3f} {name}", got, r64, r32, R.C_STATS)
    # without running statistics: the same mean / var / invstd bits
    plain = dev_stats(x.to(dev), dev, 0.0, None, off)
    assert torch.equal(plain[0], mean) and torch.equal(plain[1], var) and torch.equal(plain[2], invstd)


def test_statistics_of_a_large_offset(dev):
    """|mean| / std = 4096: the shifted accumulation keeps the variance."""
    x = torch.randn(4, 2, 16, 16, generator=torch.Generator().manual_seed(3)) + 4096.0
    mean, var, invstd, _, _ = dev_stats(x.to(dev), dev)
    ref64, ref32 = R.stats(x, BN_EPS), R.stats(x, BN_EPS, dtype=torch.float32)
    for i, name in enumerate(("mean", "var", "invstd")):
        _within(f"offset 4096 {name}", (mean, var, invstd)[i], ref64[i], ref32[i], R.C_STATS)


# ---- forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("shape,levels", R.CASES)
def test_forward_codes_and_flags(dev, shape, levels, off):
    pool = shape[4]
    for affine in (True, False):
        x, gamma, beta = R.gen_case(shape, levels, affine)
        mean, _, invstd, _, _ = dev_stats(x.to(dev), dev)
        out, flags = dev_forward(x.to(dev), mean, invstd, gamma, beta, levels, pool, dev, off)
        codes, rflags, tie = R.forward(x, mean.cpu(), invstd.cpu(), gamma, beta, levels, pool)
        got = torch.round(out.cpu() * levels).to(torch.int64)
        assert torch.equal(out.cpu(), R.values(got, levels))          # k / levels, one fp32 division
        assert_codes_tie_proven(got, codes, tie, R.TIE_CAP)
        assert torch.equal(flags.cpu()[~tie], rflags[~tie])
        assert int(flags.max()) <= (7 if pool else 1)


@pytest.mark.parametrize("off", [0, 1])
def test_forward_constructed_windows(dev, off):
    """All-equal windows keep the top-left element; a window whose only maximum is its last element selects it; NaN
    quantizes to code 0 and fails the mask. Values sit far from every tie: bit for bit."""
    levels = 15
    g = torch.Generator().manual_seed(11)
    B, C, H, W = 2, 3, 8, 12
    base = (torch.randint(-3, 19, (B, C, H // 2, W // 2), generator=g).float() + 0.25) / levels   # some outside [0, 1]
    equal = base.repeat_interleave(2, 2).repeat_interleave(2, 3)
    last = equal.clone()
    last[:, :, 1::2, 1::2] += 2.0 / levels                      # the bottom-right element alone is larger
    nan = equal.clone()
    nan[0, 0, 0, 0] = float("nan")
    mean, invstd = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    for name, x in (("equal", equal), ("last", last), ("nan", nan)):
        for pool in (True, False):
            out, flags = dev_forward(x.to(dev), mean, invstd, None, None, levels, pool, dev, off)
            codes, rflags, tie = R.forward(x, mean.cpu(), invstd.cpu(), None, None, levels, pool)
            assert not bool(tie.any())
            assert torch.equal(out.cpu(), R.values(codes, levels)), (name, pool)
            assert torch.equal(flags.cpu(), rflags), (name, pool)
            if pool and name == "equal":
                assert bool(((flags.cpu() >> 1) == 0).all())
            if pool and name == "last":   # wherever the clamp leaves the last element the larger code
                assert int(((flags.cpu() >> 1) == 3).sum()) >= flags.numel() // 2
    out, flags = dev_forward(nan.to(dev), mean, invstd, None, None, levels, False, dev, off)
    assert float(out[0, 0, 0, 0]) == 0.0 and int(flags[0, 0, 0, 0]) == 0


# ---- backward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("shape,levels", R.CASES)
def test_backward(dev, shape, levels, off):
    pool = shape[4]
    affine = levels != 3   # levels 3: the non-affine form (gamma NULL, no parameter gradients wanted)
    x, gamma, beta = R.gen_case(shape, levels, affine)
    g = R.gen_grad(shape, R.case_seed(shape, levels) + 1)
    mean, _, invstd, _, _ = dev_stats(x.to(dev), dev)
    _, flags = dev_forward(x.to(dev), mean, invstd, gamma, beta, levels, pool, dev)
    dx, dgamma, dbeta, sums = dev_backward(x.to(dev), g.to(dev), flags, mean, invstd, gamma, pool, dev, off,
                                           want=(affine, affine))
    args = (x, g, flags.cpu(), mean.cpu(), invstd.cpu(), gamma, pool)
    r64, r32 = R.backward(*args), R.backward(*args, dtype=torch.float32)
    tag = f"{shape} levels {levels} off {off}"
    _within(f"{tag} dx", dx, r64[0], r32[0], R.C_BWD, R.dx_scale(g, invstd, gamma))
    if affine:
        _within(f"{tag} dgamma", dgamma, r64[1], r32[1], R.C_BWD)
        _within(f"{tag} dbeta", dbeta, r64[2], r32[2], R.C_BWD)
    else:
        assert dgamma is None and dbeta is None
    _within(f"{tag} S1", sums[:shape[1]], r64[2], r32[2], R.C_BWD)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("pool", [False, True])
def test_backward_exact_on_dyadic_data(dev, pool, off):
    """Integer g, a = 1/2 and invstd = 2, x and mean on a grid of eighths, M = 256: every intermediate is exact in
    fp32 and in the double sums, so the kernels reproduce float64 bit for bit."""
    shape = (4, 2, 8, 8, pool)
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(-8, 13, shape[:4], generator=gen).float() / 8
    g = torch.randint(-4, 5, (4, 2, 4, 4) if pool else shape[:4], generator=gen).float()
    mean, invstd = torch.full((2,), 0.5, device=dev), torch.full((2,), 2.0, device=dev)
    gamma, beta = torch.full((2,), 0.25), torch.full((2,), 0.4)
    _, flags = dev_forward(x.to(dev), mean, invstd, gamma, beta, 15, pool, dev)
    dx, dgamma, dbeta, _ = dev_backward(x.to(dev), g.to(dev), flags, mean, invstd, gamma, pool, dev, off)
    rdx, rdgamma, rdbeta = R.backward(x, g, flags.cpu(), mean.cpu(), invstd.cpu(), gamma, pool)
    assert torch.equal(rdx.float().double(), rdx)                  # the truth is an fp32 value
    assert torch.equal(dx.cpu().double(), rdx)
    assert torch.equal(dgamma.cpu().double(), rdgamma) and torch.equal(dbeta.cpu().double(), rdbeta)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7, True), (3, 5, 4, 6, False), (2, 16, 40, 40, True),
                                   (1, 1, 91, 93, True)])
def test_masks_select(dev, shape, off):
    """A NaN gradient behind a cleared pass bit reaches nothing. With zero gradient at every passing position as
    well, S1 = S2 = 0 and dx, dgamma and dbeta are exactly 0 everywhere: masked elements, pooled-away elements and
    the dropped last row and column included."""
    pool = shape[4]
    x, gamma, beta = R.gen_case(shape, 15)
    mean, _, invstd, _, _ = dev_stats(x.to(dev), dev)
    _, flags = dev_forward(x.to(dev), mean, invstd, gamma, beta, 15, pool, dev)
    passing = (flags.cpu() & 1).bool()
    assert 0 < int(passing.sum()) < passing.numel()
    g = R.gen_grad(shape, 9)
    g_nan = torch.where(passing, g, torch.full_like(g, float("nan")))
    g_zero = torch.where(passing, g, torch.zeros_like(g))
    a = dev_backward(x.to(dev), g_nan.to(dev), flags, mean, invstd, gamma, pool, dev, off)
    b = dev_backward(x.to(dev), g_zero.to(dev), flags, mean, invstd, gamma, pool, dev, off)
    for u, v in zip(a, b):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v)
    only_nan = torch.where(passing, torch.zeros_like(g), torch.full_like(g, float("nan")))
    dx, dgamma, dbeta, sums = dev_backward(x.to(dev), only_nan.to(dev), flags, mean, invstd, gamma, pool, dev, off)
    for t in (dx, dgamma, dbeta, sums):
        assert bool((t == 0).all())
