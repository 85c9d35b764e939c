"""qvit_gemm_wgrad against the float64 CPU product G^T @ (d_act codes): exact on integer data, within the fp32-GEMM
bound 4 M 2^-24 (|G|^T |x_q|) on random data (the bound tests/test_gpu_layer_autograd.py applies to weight.grad),
deterministic, exactly homogeneous under power-of-two scaling, NaN confined to its row, padding inert."""
import pytest
import torch

from quantized_vit_amd import _lib

pytestmark = pytest.mark.gpu

# (M, N, K): one element; one tile; N and K off every alignment (padded copies); more than one tile each way with
# ragged edges; one tile with 16 M-splits and a ragged last stage; the classifier head
SHAPES = [(1, 1, 1), (10, 48, 64), (65, 10, 100), (129, 257, 130), (1000, 48, 64), (513, 1000, 768)]
D_ACT = 0.25


def _codes(M, K, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-127, 128, (M, K), generator=gen, dtype=torch.int32).to(torch.int8)


def _int_g(M, N, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (M, N), generator=gen, dtype=torch.int32).float()


def _ref(G, codes, d_act=D_ACT):
    return G.t().double() @ (d_act * codes.double())


def _run(dev, G, codes, K=None, d_act=D_ACT, **kw):
    d = torch.tensor([d_act], dtype=torch.float32, device=dev)
    return _lib.gemm_wgrad(G.to(dev), codes.to(dev), K or codes.shape[1], d, **kw)


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_on_integers(dev, shape):
    M, N, K = shape
    G, codes = _int_g(M, N, 1), _codes(M, K, 2)
    got = _run(dev, G, codes).cpu()
    assert got.shape == (N, K)
    assert torch.equal(got.double(), _ref(G, codes))          # every partial sum is an integer below 2^24
    if shape == (1000, 48, 64):
        assert _lib.gemm_wgrad_splits(M, N, K) > 1            # several M-splits, the last one ragged (1000 % 32)


@pytest.mark.parametrize("scale", [1.0, 1e-6, 1e4])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_within_fp32_gemm_bound(dev, shape, scale):
    M, N, K = shape
    gen = torch.Generator().manual_seed(3)
    G = torch.randn(M, N, generator=gen) * scale
    codes = _codes(M, K, 4)
    got = _run(dev, G, codes).cpu().double()
    ref = _ref(G, codes)
    bound = 4 * M * 2.0 ** -24 * (G.abs().t().double() @ (D_ACT * codes.double().abs()))
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"wgrad {shape} scale {scale:g}: max err {float(err.max()):.3e}, worst err / bound {worst:.4f}")
    assert bool((err <= bound).all()), (float(err.max()), worst)


def test_deterministic_scaling_and_dirty_workspace(dev):
    M, N, K = 1000, 48, 64
    gen = torch.Generator().manual_seed(5)
    G = torch.randn(M, N, generator=gen)
    codes = _codes(M, K, 6)
    a = _run(dev, G, codes)
    b = _run(dev, G, codes)
    assert torch.equal(a, b)
    for e in (-20, 12):
        assert torch.equal(_run(dev, G * 2.0 ** e, codes), a * 2.0 ** e), e
    nbytes = int(_lib.load().qvit_gemm_wgrad_workspace_bytes(M, N, K))
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    assert torch.equal(_run(dev, G, codes, workspace=ws), a)


def test_nan_stays_in_its_row(dev):
    M, N, K = 130, 48, 64
    gen = torch.Generator().manual_seed(7)
    G = torch.randn(M, N, generator=gen)
    codes = _codes(M, K, 8)
    codes[:, 5] = 0                                           # NaN times a zero code is still NaN
    clean = _run(dev, G, codes).cpu()
    m0, n0 = 129, 17
    Gn = G.clone()
    Gn[m0, n0] = float("nan")
    got = _run(dev, Gn, codes).cpu()
    assert bool(torch.isnan(got[n0]).all())
    keep = torch.arange(N) != n0
    assert bool(torch.isfinite(got[keep]).all()) and torch.equal(got[keep], clean[keep])
    Gi = G.clone()
    Gi[m0, n0] = float("inf")
    got = _run(dev, Gi, codes).cpu()
    assert not bool(torch.isfinite(got[n0]).any()) and torch.equal(got[keep], clean[keep])


def test_padding_is_inert(dev):
    M, N, K = 65, 10, 100
    G, codes = _int_g(M, N, 9), _codes(M, K, 10)
    want = _ref(G, codes)
    # codes with lda > K: zeros in [K, kpad) as qvit_quantize_act_i8 writes them, garbage in [kpad, lda)
    kpad, lda = 112, 144
    wide = torch.zeros(M, lda, dtype=torch.int8)
    wide[:, :K] = codes
    wide[:, kpad:] = 77
    assert torch.equal(_run(dev, G, wide, K=K).cpu().double(), want)
    # garbage right behind K as well: columns past K never reach dW
    wide[:, K:] = -99
    assert torch.equal(_run(dev, G, wide, K=K).cpu().double(), want)
    # dW with ldw > K: columns [K, ldw) keep the sentinel
    out = torch.full((N, 128), -7.5, dtype=torch.float32, device=dev)
    _run(dev, G, codes, out=out)
    assert torch.equal(out[:, :K].cpu().double(), want)
    assert bool((out[:, K:] == -7.5).all())
    # G as a column slice of a wider tensor (row stride 16, garbage behind N) and an unaligned one (copied)
    Gw = torch.full((M, 16), float("nan"))
    Gw[:, :N] = G
    assert torch.equal(_run(dev, Gw.to(dev)[:, :N], codes).cpu().double(), want)
    G1 = torch.zeros(M, N + 1)
    G1[:, 1:] = G
    assert torch.equal(_run(dev, G1.to(dev)[:, 1:], codes).cpu().double(), want)


def test_no_rows_writes_zeros(dev):
    d = torch.tensor([D_ACT], dtype=torch.float32, device=dev)
    out = torch.full((4, 8), 3.0, dtype=torch.float32, device=dev)
    # M == 0 at the C entry point: the reduction alone runs and writes zeros
    g = torch.zeros(4, 4, dtype=torch.float32, device=dev)      # valid pointers, no rows read
    c = torch.zeros(16, dtype=torch.int8, device=dev)
    ws = torch.full((128 * 128,), float("nan"), dtype=torch.float32, device=dev)
    st = _lib.load().qvit_gemm_wgrad(g.data_ptr(), 0, 4, 4, c.data_ptr(), 8, 16, d.data_ptr(), out.data_ptr(), 8,
                                     ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream(dev).cuda_stream)
    assert st == 0
    assert bool((out == 0).all())
