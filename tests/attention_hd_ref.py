"""attention_backward_ref.py with the head width as a parameter (that helper fixes 64): the float64 restatement of
the reference attention core (QViT_with_GETA/vit_model.py:133-149)
    q, k, v = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    attn = softmax((q @ k^T) * scale);  out = (attn @ v).transpose(1, 2).reshape(B, N, H * hd)
its closed-form gradients, and the same expression in float32 on the CPU (the accuracy yardstick). At hd = 64 every
function here returns what attention_backward_ref returns for the same inputs (test_attention_hd_ref_cpu.py)."""
import functools

import torch

EPS32 = float(torch.finfo(torch.float32).eps)


def attention(qkv: torch.Tensor, B: int, N: int, H: int, scale: float, hd: int) -> torch.Tensor:
    """[B*N, 3*H*hd] -> [B*N, H*hd], in qkv's dtype."""
    x = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    attn = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B * N, H * hd)


def forward(qkv: torch.Tensor, B: int, N: int, H: int, scale: float, hd: int, dtype) -> torch.Tensor:
    """The forward on the CPU in `dtype`; returned as float64."""
    return attention(qkv.detach().cpu().to(dtype), B, N, H, scale, hd).double()


def grads(qkv: torch.Tensor, dO: torch.Tensor, B: int, N: int, H: int, scale: float, hd: int, dtype) -> torch.Tensor:
    """d(sum(out * dO)) / d(qkv) by CPU autograd in `dtype`; returned as float64."""
    x = qkv.detach().cpu().to(dtype).clone().requires_grad_(True)
    out = attention(x, B, N, H, scale, hd)
    out.backward(dO.detach().cpu().to(dtype))
    return x.grad.double()


def closed_form(qkv: torch.Tensor, dO: torch.Tensor, B: int, N: int, H: int, scale: float, hd: int):
    """The formulas the kernel implements, in float64. Returns (dqkv, dP, dS)."""
    x = qkv.double().reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]                                   # [B, H, N, hd]
    g = dO.double().reshape(B, N, H, hd).permute(0, 2, 1, 3)      # [B, H, N, hd]
    P = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    O = P @ v
    D = (g * O).sum(-1, keepdim=True)
    dV = P.transpose(-2, -1) @ g
    dP = g @ v.transpose(-2, -1)
    dS = P * (dP - D)
    dq = scale * (dS @ k)
    dk = scale * (dS.transpose(-2, -1) @ q)
    d = torch.stack([dq, dk, dV], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * hd)
    return d, dP, dS


def make_inputs(B: int, N: int, H: int, hd: int, seed: int, qk_std: float = 1.0, v_std: float = 1.0,
                g_std: float = 1.0):
    """Seeded on the CPU, drawn as attention_backward_ref.make_inputs draws them."""
    gen = torch.Generator().manual_seed(seed)
    C = H * hd
    qkv = torch.randn(B * N, 3 * C, generator=gen, dtype=torch.float32)
    qkv[:, :2 * C] *= qk_std
    qkv[:, 2 * C:] *= v_std
    dO = torch.randn(B * N, C, generator=gen, dtype=torch.float32) * g_std
    return qkv, dO


def sections(d: torch.Tensor, H: int, hd: int):
    C = H * hd
    return d[:, :C], d[:, C:2 * C], d[:, 2 * C:3 * C]


def rel_err(a: torch.Tensor, b64: torch.Tensor, den=None) -> float:
    """max |a - b64| / max |b64| (`den` replaces the denominator where given)."""
    d = float(b64.abs().max()) if den is None else float(den)
    e = float((a.double().cpu() - b64).abs().max())
    return e / d if d > 0 else e


def section_errs(g: torch.Tensor, g64: torch.Tensor, H: int, hd: int, denoms=None):
    """rel_err per section (dq, dk, dv); `denoms` replaces the denominators where given."""
    return [rel_err(a, b, None if denoms is None else denoms[i])
            for i, (a, b) in enumerate(zip(sections(g.double().cpu(), H, hd), sections(g64, H, hd)))]


def cancel_scales(qkv: torch.Tensor, dO: torch.Tensor, B: int, N: int, H: int, scale: float, hd: int):
    """Magnitude of the terms that cancel in dq and dk: scale max|dP| max|k| and scale max|dP| max|q| (the
    denominators where the true dq, dk are zero by cancellation: one key)."""
    _, dP, _ = closed_form(qkv, dO, B, N, H, scale, hd)
    q, k, _ = sections(qkv.double(), H, hd)
    m = float(dP.abs().max())
    return scale * m * float(k.abs().max()), scale * m * float(q.abs().max())


@functools.lru_cache(maxsize=None)
def case(B: int, N: int, H: int, hd: int, seed: int = 0, qk_std: float = 1.0, v_std: float = 1.0, g_std: float = 1.0,
         scale=None):
    """(qkv, dO, o64, o32, g64, g32) for a seeded case, computed once per session and shared (do not modify)."""
    scale = hd ** -0.5 if scale is None else scale
    qkv, dO = make_inputs(B, N, H, hd, seed, qk_std, v_std, g_std)
    return (qkv, dO, forward(qkv, B, N, H, scale, hd, torch.float64), forward(qkv, B, N, H, scale, hd, torch.float32),
            grads(qkv, dO, B, N, H, scale, hd, torch.float64), grads(qkv, dO, B, N, H, scale, hd, torch.float32))
