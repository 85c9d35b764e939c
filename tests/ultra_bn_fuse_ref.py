"""CPU restatements of ultra_bn_fuse.hip in plain torch, any dtype (float64 is the truth,
float32 the yardstick's own error), the flag bytes included, and the input generators of the GPU tests. Nothing
here touches the HIP library.

Flag bytes: unpooled, bit 0 = 0 <= y <= 1. Pooled, bit 0 = that test on the window's winner, bits 1-2 = the winner
2 dy + dx, the first maximum code in row-major order.

Possible ties (forward comparison): the kernel computes, in fp32, d = x - mean, a = gamma invstd, y = fmaf(d, a,
beta), v = clamp(y) levels: four roundings of at most 2^-24 relative, on d (which a then scales), on a (scaling d),
on y and on v. So |y_kernel - y| <= 2^-24 (2 |d a| + |y|) and |v_kernel - v| <= levels 2^-24 (2 |d a| + 2 |y|).
The margin used is twice that bound: my = 2^-22 (|d a| + |y|) for the clamp's edges, levels my for the rounding ties.
An element is a possible tie if v is within levels my of a half-integer or y within my of 0 or 1; a pooled output
is one if any element of its window is (its code, winner or pass bit may then differ).
"""
import torch
import torch.nn.functional as F

# Accuracy constants of the GPU tests: err <= c * max(err of the float32 restatement, eps) with err =
# max|got - ref64| / max|ref64|; each c the next power of two at or above twice the worst ratio measured on an
# MI355X (DESIGN.md section 18 holds the table).
C_STATS = 1.0     # mean, var, invstd, running statistics; worst measured ratio 0.443 (invstd, (1, 1, 91, 93)). The
#                   device rounds a double result once: at most 2^-24 of the value, half of eps, whatever the input
C_BWD = 2.0       # dx (against max|a| max|g|, the size of its terms), dgamma, dbeta at kernel level; worst measured
#                   ratio 1.000 (dx, (1, 1, 91, 93) pooled, levels 15), dgamma 0.742, dbeta 0.359
C_MODULE = 2.0    # bn_act_pool's gradients at module level; worst measured ratio 0.725 (input.grad, (2, 4, 8, 8)
#                   a_bit 7), gamma.grad 0.668 ((2, 16, 40, 40)), beta.grad 0.243
TIE_CAP = 1e-2    # possible ties allowed per GPU parametrisation

# (B, C, H, W, pool) of tests/test_gpu_ultra_bn_fuse.py and what each is there for
SHAPES = [
    (2, 1, 1, 1, False),     # smallest valid M
    (1, 2, 2, 2, True),      # pooled to 1 x 1
    (2, 3, 5, 7, True),      # odd H and W, scalar arm
    (3, 5, 4, 6, False),     # planes not 16 B aligned once the base is offset
    (1, 16, 9, 9, False),    # many channels, single image, odd map
    (2, 64, 6, 6, True),     # 64 channels with pooling on a small map
    (2, 16, 40, 40, True),   # many workgroups, 32 partials per channel
    (4, 2, 64, 64, True),    # a reduction spanning many partials
    # a workgroup owns 8192 elements of a plane (2048 pooled windows): planes of more than one slice, each arm
    (1, 2, 96, 96, True),    # 9216 elements, 2304 windows: two slices, 16-byte arm
    (1, 2, 96, 96, False),
    (1, 1, 91, 93, True),    # 8463 elements, 2070 windows: two slices, scalar arm, dropped row and column
    (1, 1, 91, 93, False),
]
LEVELS = (3, 15, 127)
CASES = [(s, lv) for s in SHAPES for lv in LEVELS]


def case_seed(shape, levels) -> int:
    B, C, H, W, pool = shape
    return ((B * 131 + C) * 131 + H) * 131 + W * 7 + int(pool) * 3 + levels * 1009


def gen_case(shape, levels, affine: bool = True, seed: int = None):
    """(x, gamma, beta): x ~ N(o_c, s_c^2) per channel; gamma ~ U(0.35, 0.55), beta ~ U(0.35, 0.65), which put about
    an eighth of the normalised values below 0 and as many above 1 and spread the rest over every code."""
    B, C, H, W, _ = shape
    g = torch.Generator().manual_seed(case_seed(shape, levels) if seed is None else seed)
    s = torch.rand(C, generator=g) * 1.5 + 0.5
    o = torch.rand(C, generator=g) * 2 - 1
    x = torch.randn(B, C, H, W, generator=g) * s.view(1, C, 1, 1) + o.view(1, C, 1, 1)
    if not affine:
        return x, None, None
    return x, torch.rand(C, generator=g) * 0.2 + 0.35, torch.rand(C, generator=g) * 0.3 + 0.35


def gen_tied(shape, seed: int):
    """x on a grid of half-integers: many elements of a window are equal, so their codes tie."""
    B, C, H, W, _ = shape
    g = torch.Generator().manual_seed(seed)
    return torch.round(torch.randn(B, C, H, W, generator=g) * 2) / 2


def gen_grad(shape, seed: int) -> torch.Tensor:
    B, C, H, W, pool = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, C, H // 2, W // 2) if pool else (B, C, H, W), generator=g)


def _c(t, dtype):
    return t.to(dtype).view(1, -1, 1, 1)


def stats(x, eps, factor=0.0, running_mean=None, running_var=None, dtype=torch.float64):
    """(mean, biased var, invstd, new running_mean, new running_var) of qvit_bn_stats; the running values are None
    when not given."""
    xd = x.to(dtype)
    M = x.shape[0] * x.shape[2] * x.shape[3]
    mean = xd.mean((0, 2, 3))
    var = (xd - mean.view(1, -1, 1, 1)).square().mean((0, 2, 3))
    invstd = 1 / torch.sqrt(var + eps)
    rm = rv = None
    if running_mean is not None:
        rm = (1 - factor) * running_mean.to(dtype) + factor * mean
    if running_var is not None:
        rv = (1 - factor) * running_var.to(dtype) + factor * (var * (M / (M - 1)))
    return mean, var, invstd, rm, rv


def _windows(t: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W] -> [B, C, H/2, W/2, 4], each window row-major (floor: an odd last row / column is dropped)."""
    B, C, H, W = t.shape
    v = t[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2)
    return v.permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def forward(x, mean, invstd, gamma, beta, levels: int, pool: bool):
    """(codes int64, flag bytes uint8, possible-tie mask), each shaped as the output, in float64."""
    d = x.double() - _c(mean, torch.float64)
    a = _c(invstd, torch.float64) * (1.0 if gamma is None else _c(gamma, torch.float64))
    y = d * a + (0.0 if beta is None else _c(beta, torch.float64))
    v = y.clamp(0, 1) * levels
    codes = torch.where(torch.isnan(y), torch.zeros_like(v), torch.round(v)).to(torch.int64)
    passed = (y >= 0) & (y <= 1)
    my = 2.0 ** -22 * ((d * a).abs() + y.abs())
    tie = ((v - (torch.floor(v) + 0.5)).abs() <= levels * my) | (torch.minimum(y.abs(), (y - 1).abs()) <= my)
    if not pool:
        return codes, passed.to(torch.uint8), tie
    kw, pw, tw = _windows(codes), _windows(passed), _windows(tie)
    best = kw.amax(-1)
    idx = (kw == best.unsqueeze(-1)).to(torch.int8).argmax(-1)        # the first maximum
    pwin = pw.gather(-1, idx.unsqueeze(-1)).squeeze(-1)
    return best, (pwin.to(torch.uint8) | (idx.to(torch.uint8) << 1)), tw.any(-1)


def values(codes: torch.Tensor, levels: int) -> torch.Tensor:
    """The fp32 output of the kernel for these codes: k / levels, one IEEE fp32 division."""
    return codes.float() / float(levels)


def grad_y(g, flags, in_shape, pool: bool) -> torch.Tensor:
    """g_y at full size: g where the flag byte's pass bit is set (pooled: at the winner), else 0. Selected: a NaN g
    behind a cleared bit does not appear."""
    zero = torch.zeros((), dtype=g.dtype)
    if not pool:
        return torch.where((flags & 1).bool(), g, zero)
    B, C, H, W = in_shape
    gy = torch.zeros(in_shape, dtype=g.dtype)
    ok, idx = (flags & 1).bool(), (flags >> 1) & 3
    for e in range(4):
        gy[:, :, e // 2:H // 2 * 2:2, e % 2:W // 2 * 2:2] = torch.where(ok & (idx == e), g, zero)
    return gy


def backward(x, g, flags, mean, invstd, gamma, pool: bool, dtype=torch.float64):
    """(dx, dgamma = S2, dbeta = S1) of the two backward kernels."""
    xd = x.to(dtype)
    M = x.shape[0] * x.shape[2] * x.shape[3]
    gy = grad_y(g.to(dtype), flags, x.shape, pool)
    xhat = (xd - _c(mean, dtype)) * _c(invstd, dtype)
    S1, S2 = gy.sum((0, 2, 3)), (gy * xhat).sum((0, 2, 3))
    a = _c(invstd, dtype) * (1.0 if gamma is None else _c(gamma, dtype))
    dx = a * (gy - S1.view(1, -1, 1, 1) / M - xhat * (S2.view(1, -1, 1, 1) / M))
    return dx, S2, S1


def autograd_truth(x, gamma, beta, eps, levels: int, pool: bool, g):
    """float64 autograd of F.batch_norm(training=True) -> clamp(0, 1) -> straight-through round -> F.max_pool2d:
    (output, dx, dgamma, dbeta)."""
    xd = x.double().requires_grad_(True)
    gm = None if gamma is None else gamma.double().requires_grad_(True)
    bt = None if beta is None else beta.double().requires_grad_(True)
    y = F.batch_norm(xd, None, None, gm, bt, True, 0.1, eps)
    c = torch.clamp(y, 0, 1)
    q = c + (torch.round(c * levels) / levels - c).detach()
    out = F.max_pool2d(q, 2, 2) if pool else q
    out.backward(g.double())
    return out.detach(), xd.grad, None if gm is None else gm.grad, None if bt is None else bt.grad


def rel(got, ref, scale: float = 0.0) -> float:
    """max|got - ref| / max(max|ref|, scale). `scale`: the magnitude of the terms that meet in the result, for
    results that cancel (dx of a two-value channel is 0 in exact arithmetic)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(max(scale, 1e-300)))


def dx_scale(g, invstd, gamma) -> float:
    """max|a| max|g| with a = gamma invstd: the size of the three terms of dx = a (g_y - S1 / M - xhat S2 / M)."""
    a = invstd.double().cpu() * (1.0 if gamma is None else gamma.double().cpu())
    g = g.double().cpu()
    return float(a.abs().max() * torch.nan_to_num(g, nan=0.0).abs().max())
