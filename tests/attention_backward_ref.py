"""Restatement of the reference attention core (QViT_with_GETA/vit_model.py:133-149) for the backward tests:
    q, k, v = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    attn = softmax((q @ k^T) * scale);  out = (attn @ v).transpose(1, 2).reshape(B, N, H * hd)
in float64 (the truth; gradients from torch autograd on the CPU) and, the same expression, in float32 on the CPU
(the accuracy yardstick: what the parent's torch branch computes, up to summation order)."""
import functools

import torch

HD = 64
EPS32 = float(torch.finfo(torch.float32).eps)


def attention(qkv: torch.Tensor, B: int, N: int, H: int, scale: float) -> torch.Tensor:
    """[B*N, 3*H*64] -> [B*N, H*64], in qkv's dtype."""
    x = qkv.reshape(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    attn = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B * N, H * HD)


def grads(qkv: torch.Tensor, dO: torch.Tensor, B: int, N: int, H: int, scale: float, dtype) -> torch.Tensor:
    """d(sum(out * dO)) / d(qkv) by CPU autograd in `dtype`; returned as float64."""
    x = qkv.detach().cpu().to(dtype).clone().requires_grad_(True)
    out = attention(x, B, N, H, scale)
    out.backward(dO.detach().cpu().to(dtype))
    return x.grad.double()


def closed_form(qkv: torch.Tensor, dO: torch.Tensor, B: int, N: int, H: int, scale: float):
    """The formulas the kernel implements, in float64. Returns (dqkv, dP, dS)."""
    x = qkv.double().reshape(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]                                   # [B, H, N, hd]
    g = dO.double().reshape(B, N, H, HD).permute(0, 2, 1, 3)      # [B, H, N, hd]
    P = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    O = P @ v
    D = (g * O).sum(-1, keepdim=True)
    dV = P.transpose(-2, -1) @ g
    dP = g @ v.transpose(-2, -1)
    dS = P * (dP - D)
    dq = scale * (dS @ k)
    dk = scale * (dS.transpose(-2, -1) @ q)
    d = torch.stack([dq, dk, dV], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * HD)
    return d, dP, dS


def make_inputs(B: int, N: int, H: int, seed: int, qk_std: float = 1.0, v_std: float = 1.0, g_std: float = 1.0):
    """Seeded on the CPU. q and k rows are N(0, qk_std^2): logits q.k / 8 of std ~ qk_std^2."""
    gen = torch.Generator().manual_seed(seed)
    C = H * HD
    qkv = torch.randn(B * N, 3 * C, generator=gen, dtype=torch.float32)
    qkv[:, :2 * C] *= qk_std
    qkv[:, 2 * C:] *= v_std
    dO = torch.randn(B * N, C, generator=gen, dtype=torch.float32) * g_std
    return qkv, dO


def sections(d: torch.Tensor, H: int):
    C = H * HD
    return d[:, :C], d[:, C:2 * C], d[:, 2 * C:3 * C]


def section_errs(g: torch.Tensor, g64: torch.Tensor, H: int, denoms=None):
    """max |g - g64| / max |g64| per section (dq, dk, dv); `denoms` replaces the denominators where given."""
    out = []
    for i, (a, b) in enumerate(zip(sections(g.double().cpu(), H), sections(g64, H))):
        den = float(b.abs().max()) if denoms is None or denoms[i] is None else float(denoms[i])
        out.append(float((a - b).abs().max()) / den if den > 0 else float((a - b).abs().max()))
    return out


def cancel_scales(qkv: torch.Tensor, dO: torch.Tensor, B: int, N: int, H: int, scale: float):
    """Magnitude of the terms that cancel in dq and dk: scale max|dP| max|k| and scale max|dP| max|q|. The
    denominator for cases whose true dq, dk are zero by cancellation (one key; dO constant along a row of P)."""
    _, dP, _ = closed_form(qkv, dO, B, N, H, scale)
    q, k, _ = sections(qkv.double(), H)
    m = float(dP.abs().max())
    return scale * m * float(k.abs().max()), scale * m * float(q.abs().max())


@functools.lru_cache(maxsize=None)
def case(B: int, N: int, H: int, seed: int = 0, qk_std: float = 1.0, v_std: float = 1.0, g_std: float = 1.0,
         scale: float = HD ** -0.5):
    """(qkv, dO, g64, g32) for a seeded case, computed once per session and shared (do not modify)."""
    qkv, dO = make_inputs(B, N, H, seed, qk_std, v_std, g_std)
    return qkv, dO, grads(qkv, dO, B, N, H, scale, torch.float64), grads(qkv, dO, B, N, H, scale, torch.float32)
