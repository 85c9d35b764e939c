"""qvit_pack_weight_b3 + qvit_gemm_f32w against the float64 product. TERMS 6: exact on integers whose dropped terms
vanish and within gemm_f32's bound (4 K + 9) 2^-24 (|A||W|); TERMS 3: within that bound plus (2^-13 + 2^-20) (|A||W|)
for the dropped products a2b2, a1b3, a3b1 and below. The fused epilogues equal the separate ops bit for bit; the same
call gives the same bits; NaN / Inf in A stay in their row; columns of C past N are not written."""
import pytest
import torch

from quantized_vit_amd import _lib

pytestmark = pytest.mark.gpu

# (K, M, N): one element; one tile; ragged last stage and padded rows; ragged multi-tile with an odd stage count for
# the two-buffer ring; many stages
SHAPES = [(1, 1, 1), (10, 48, 64), (65, 10, 100), (129, 257, 130), (1000, 48, 64)]
TERMS = [6, 3]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _run(dev, A, W, terms, **kw):
    image = _lib.pack_weight_b3(W.to(dev), 3 if terms == 6 else 2)
    return _lib.gemm_f32w(A.to(dev), image, W.shape[0], terms, **kw)


def _bound(A, W, terms):
    K = A.shape[1]
    rel = (4 * K + 9) * 2.0 ** -24 + (2.0 ** -13 + 2.0 ** -20 if terms == 3 else 0.0)
    return rel * (A.double().abs() @ W.double().abs().t())


# (K, M, N, max |A|, max |W|): partial sums below 2^24, dropped cross terms zero; 12 x 9 bits: two terms on each side
@pytest.mark.parametrize("case", [(K, M, N, 8, 127) for K, M, N in SHAPES] +
                         [(K, 65, 130, 4095, 511) for K in (1, 2, 3, 4)])
def test_terms6_exact_on_integers(dev, case):
    K, M, N, ta, tw = case
    gen = torch.Generator().manual_seed(1)
    A = torch.randint(-ta, ta + 1, (M, K), generator=gen).float()
    W = torch.randint(-tw, tw + 1, (N, K), generator=gen).float()
    got = _run(dev, A, W, 6).cpu()
    assert got.shape == (M, N)
    assert torch.equal(got.double(), A.double() @ W.double().t())


@pytest.mark.parametrize("scale", [1.0, 1e-6, 1e4])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("terms", TERMS)
def test_random_within_bound(dev, terms, shape, scale):
    K, M, N = shape
    A, W = _randn((M, K), 3) * scale, _randn((N, K), 4)
    err = (_run(dev, A, W, terms).cpu().double() - A.double() @ W.double().t()).abs()
    bound = _bound(A, W, terms)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"gemm_f32w terms {terms} {shape} scale {scale:g}: max err {float(err.max()):.3e}, err / bound {worst:.4f}")
    assert bool((err <= bound).all()), (float(err.max()), worst)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("terms", TERMS)
def test_epilogues_equal_the_separate_ops(dev, terms, with_bias):
    K, M, N = 129, 257, 130
    A, W = _randn((M, K), 5).to(dev), _randn((N, K), 6)
    bias = _randn((N,), 7).to(dev) if with_bias else None
    image = _lib.pack_weight_b3(W.to(dev), 3 if terms == 6 else 2)
    plain = _lib.gemm_f32w(A, image, N, terms, bias)
    if with_bias:
        assert torch.equal(plain, _lib.gemm_f32w(A, image, N, terms) + bias)   # one fp32 add behind the product
    gelu = _lib.gemm_f32w(A, image, N, terms, bias, _lib.EPI_F32_GELU)
    assert torch.equal(gelu, _lib.gelu_f32(plain.contiguous()))
    resid = _randn((M, 132), 8).to(dev)        # 130 columns of a 132-wide buffer
    want = resid.clone()
    want[:, :N] += plain
    got = _lib.gemm_f32w(A, image, N, terms, bias, _lib.EPI_F32_RESID, out=resid[:, :N])
    assert got.data_ptr() == resid.data_ptr() and torch.equal(resid, want)


@pytest.mark.parametrize("terms", TERMS)
def test_deterministic_nan_inf_rows_and_untouched_columns(dev, terms):
    K, M, N = 129, 257, 130
    A, W = _randn((M, K), 9), _randn((N, K), 10)
    out = torch.full((M, 136), -7.0, device=dev)
    clean = _run(dev, A, W, terms, out=out[:, :N]).cpu()
    assert bool((out[:, N:] == -7.0).all())
    assert torch.equal(clean, _run(dev, A, W, terms).cpu())
    Ab = A.clone()
    Ab[200, 77], Ab[3, 128] = float("nan"), float("inf")
    got = _run(dev, Ab, W, terms).cpu()
    keep = torch.ones(M, dtype=torch.bool)
    keep[[3, 200]] = False
    assert not bool(torch.isfinite(got[[3, 200]]).any())
    assert torch.equal(got[keep], clean[keep])
