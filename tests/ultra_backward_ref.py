"""CPU restatements of UltraNet's training backward in plain torch, written from the formulas:
the straight-through quantizers of the reference's quant_ultra.py, the closed-form backward of its weight quantizer,
the clamp mask of its activation quantizer, the two gradients of a convolution as explicit patch contractions, and
a torch-only UltraNet module stack. Any dtype (the tests use float64 as the truth and float32 as the yardstick's
own error); nothing here touches the HIP library."""
import torch
import torch.nn.functional as F

# Accuracy constants of the GPU tests: err <= c * max(err of the float32 restatement, eps), each c the next power
# of two at or above twice the worst ratio measured on an MI355X (DESIGN.md section 17 holds the tables).
C_WGRAD = 4.0     # qvit_conv_wgrad; worst 1.252 at (3, 64, 4, 4, 36, 1, ...); Conv2d_Q's weight.grad: 0.72
C_DGRAD = 8.0     # qvit_conv_wonly on the flipped image; worst 2.110 at (2, 16, 40, 40, 16, 3, ...)
C_LINEAR = 2.0    # Linear_Q's three gradients; worst 0.766 (the input gradient)
C_NET = 8.0       # UltraNetQua's output and gradients on every route, against the float64 restatement; worst 2.008
#                   (layers.17.weight, default route; the float32 restatement on the device is the unit)
NET_TORCH_VS_DEFAULT = 2.0 ** -16   # QVIT_ULTRA_BWD=torch against the default, max|a - b| / max|b|: the next power
#                   of two at or above twice the measured worst 7.45e-6 (layers.12.weight)


def ste_round(x: torch.Tensor, n: float) -> torch.Tensor:
    """round(x n) / n forward, identity backward (uniform_quantize, quant_ultra.py:8-27)."""
    return x + (torch.round(x * n) / n - x).detach()


def weight_quantize(w: torch.Tensor, w_bit: int) -> torch.Tensor:
    """weight_quantize_fn.forward for 2 <= w_bit <= 8 (quant_ultra.py:50-55) with the straight-through rounding."""
    t = torch.tanh(w)
    return ste_round(t / t.abs().max(), float(2 ** (w_bit - 1) - 1))


def act_quantize(x: torch.Tensor, a_bit: int) -> torch.Tensor:
    """activation_quantize_fn.forward (quant_ultra.py:71) with the straight-through rounding."""
    return ste_round(torch.clamp(x, 0, 1), float(2 ** a_bit - 1))


def weight_quant_backward(w: torch.Tensor, g: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """g_w of weight_quantize given g, the gradient of its output: t = tanh(w), m = max|t|, c ties,
    g_t = g / m - sgn(t) [|t| == m] (sum g t) / (m^2 c), g_w = g_t (1 - t^2). Masks select."""
    w, g = w.to(dtype), g.to(dtype)
    t = torch.tanh(w)
    m = t.abs().max()
    tie = t.abs() == m
    coef = (g * t).sum() / (m * m * tie.sum())
    g_t = g / m - torch.where(tie, torch.sign(t) * coef, torch.zeros_like(t))
    return g_t * (1 - t * t)


def weight_quant_bound(w: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """Elementwise error bound of an fp32 evaluation of weight_quant_backward against float64:
    2^-19 (|g| / m + [tie] sum|g t| / (m^2 c)). Reasoning: t and m are fp32 tanh values (taken as within 4 ulp,
    2^-21 relative), so g / m, the sum's terms and 1 - t^2 (absolute 2 |t| 2^-21 on a factor <= 1) are each within
    about 2^-21 of the magnitude flowing through them, and at most four such errors and four roundings of 2^-24
    meet in one element: 4 * 2^-21 + 4 * 2^-24 < 2^-19 of |g| / m plus the tie term's magnitude, the latter taken
    with sum|g t| because the sum's error does not cancel where the sum does."""
    w, g = w.double(), g.double()
    t = torch.tanh(w)
    m = t.abs().max()
    tie = (t.abs() == m).double()
    return 2.0 ** -19 * (g.abs() / m + tie * (g * t).abs().sum() / (m * m * tie.sum()))


def act_quant_backward(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """g where 0 <= x <= 1 (both boundaries pass; a NaN x fails both tests), else 0."""
    return torch.where((x >= 0) & (x <= 1), g, torch.zeros_like(g))


def conv_wgrad(G: torch.Tensor, x: torch.Tensor, kernel_size, stride, padding, dilation,
               dtype=torch.float64) -> torch.Tensor:
    """dW[n][c][ky][kx] = sum_{b,oy,ox} G[b][n][oy][ox] x[b][c][oy sh - ph + ky dh][ox sw - pw + kx dw] (zero
    padding) as one contraction of G with the patch matrix."""
    B, C = x.shape[:2]
    N = G.shape[1]
    cols = F.unfold(x.to(dtype), kernel_size, dilation, padding, stride)        # [B, C kh kw, OH OW]
    return torch.einsum("bnl,bkl->nk", G.to(dtype).reshape(B, N, -1), cols).reshape(N, C, *kernel_size)


def conv_dgrad(G: torch.Tensor, wq: torch.Tensor, in_hw, stride, padding, dilation,
               dtype=torch.float64) -> torch.Tensor:
    """dX[b][c][iy][ix] = sum over (n, ky, kx, oy, ox) hitting (iy, ix) of G[b][n][oy][ox] wq[n][c][ky][kx]: the
    patch-matrix gradient scattered back to the image."""
    B, N = G.shape[:2]
    cols = torch.einsum("nk,bnl->bkl", wq.to(dtype).reshape(N, -1), G.to(dtype).reshape(B, N, -1))
    return F.fold(cols, in_hw, wq.shape[2:], dilation, padding, stride)


ULTRA_STACK = ((3, 16, True), (16, 32, True), (32, 64, True), (64, 64, True), (64, 64, False), (64, 64, False),
               (64, 64, False), (64, 64, False))   # mymodel.py:71-121: (cin, cout, max pool) of the 8 blocks


def ultranet_params(state: dict) -> dict:
    """The trainable tensors of an UltraNetQua state_dict (conv weights, BN affine, the head's bias), cloned."""
    return {k: v.detach().clone() for k, v in state.items()
            if k.endswith(".weight") or k.endswith(".bias")}


def ultranet_forward(params: dict, x: torch.Tensor, w_bit: int = 4, a_bit: int = 4, na: int = 6, no: int = 6,
                     pre_quant: list = None) -> torch.Tensor:
    """UltraNetQua.forward in training mode (mymodel.py:134-144) on plain torch: F.conv2d on the straight-through
    fake-quant weight, batch-statistics BatchNorm, the straight-through activation quantizer, max pool, the 1x1
    head, and YOLOLayer's training output p [B, na, ny, nx, no]. `pre_quant` collects the quantizers' inputs."""
    i = 0
    for _, _, pool in ULTRA_STACK:
        x = F.conv2d(x, weight_quantize(params[f"layers.{i}.weight"], w_bit), None, 1, 1)
        x = F.batch_norm(x, None, None, params[f"layers.{i + 1}.weight"], params[f"layers.{i + 1}.bias"], True, 0.1,
                         1e-5)
        if pre_quant is not None:
            pre_quant.append(x)
        x = act_quantize(x, a_bit)
        i += 3
        if pool:
            x = F.max_pool2d(x, 2, 2)
            i += 1
    x = F.conv2d(x, weight_quantize(params[f"layers.{i}.weight"], w_bit), params[f"layers.{i}.bias"])
    bs, _, ny, nx = x.shape
    return x.view(bs, na, no, ny, nx).permute(0, 1, 3, 4, 2).contiguous()


def round_tie_distance(v: torch.Tensor, levels: float) -> torch.Tensor:
    """|v levels - (k + 1/2)| / levels to the nearest rounding tie of round(v levels)."""
    s = v.double() * levels
    return ((s - torch.floor(s)) - 0.5).abs() / levels


def tie_distance(v: torch.Tensor, levels: float) -> torch.Tensor:
    """Distance of v to the nearest point where clamp-then-round (or its mask) switches: the rounding ties
    (k + 1/2) / levels inside [0, 1], and the clamp's boundaries 0 and 1 from either side."""
    v = v.double()
    s = v * levels
    tie = ((s - torch.floor(s)) - 0.5).abs() / levels
    edge = torch.minimum(v.abs(), (v - 1).abs())
    return torch.where((v >= 0) & (v <= 1), torch.minimum(tie, edge), edge)
