"""qvit_gemm_f32_nt / qvit_gemm_f32_tn against the float64 product: exact on integers whose dropped cross terms
vanish, within (4 L + 9) 2^-24 (|A||B|) on random data, deterministic, exactly homogeneous under power-of-two scaling,
NaN / Inf confined to the row or column that contracts it, padding inert. Operands are written here as X [rows, L] and
Y [cols, L] with C = X Y^T; NT takes them as they are, TN takes their transposes (the contraction along the rows)."""
import pytest
import torch

from quantized_vit_amd import _lib

pytestmark = pytest.mark.gpu

FORMS = ["nt", "tn"]
# (L, rows, cols): one element; one tile; every alignment off (padded copies); ragged multi-tile; one tile with 16
# splits (TN) and a ragged last stage; the classifier head
SHAPES = [(1, 1, 1), (10, 48, 64), (65, 10, 100), (129, 257, 130), (1000, 48, 64), (513, 1000, 768)]


def _run(dev, form, X, Y, **kw):
    if form == "nt":
        return _lib.gemm_f32_nt(X.to(dev), Y.to(dev), **kw)
    return _lib.gemm_f32_tn(X.t().contiguous().to(dev), Y.t().contiguous().to(dev), **kw)


def _ints(shape, top, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-top, top + 1, shape, generator=gen, dtype=torch.int64).float()


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# (L, rows, cols, max |X|, max |Y|): every partial sum stays below 2^24 and every dropped cross term is zero.
# 12 x 9 bits: two non-zero bf16 terms on each side; 20 x 3 bits: three terms on one side, one on the other.
INT_CASES = [(L, r, c, 8, 127) for L, r, c in SHAPES] + [(L, 65, 130, 4095, 511) for L in (1, 2, 3, 4)] + \
            [(L, 65, 130, tx, ty) for L in (1, 2) for tx, ty in ((2 ** 20 - 1, 7), (7, 2 ** 20 - 1))]


@pytest.mark.parametrize("case", INT_CASES)
@pytest.mark.parametrize("form", FORMS)
def test_exact_on_integers(dev, form, case):
    L, rows, cols, tx, ty = case
    X, Y = _ints((rows, L), tx, 1), _ints((cols, L), ty, 2)
    got = _run(dev, form, X, Y).cpu()
    assert got.shape == (rows, cols)
    assert torch.equal(got.double(), X.double() @ Y.double().t())
    if form == "tn" and (L, rows, cols) == (1000, 48, 64):
        assert _lib.gemm_f32_tn_splits(L, rows, cols) == 16


@pytest.mark.parametrize("scale", [1.0, 1e-6, 1e4])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_random_within_fp32_gemm_bound(dev, form, shape, scale):
    L, rows, cols = shape
    X, Y = _randn((rows, L), 3) * scale, _randn((cols, L), 4)
    got = _run(dev, form, X, Y).cpu().double()
    bound = (4 * L + 9) * 2.0 ** -24 * (X.double().abs() @ Y.double().abs().t())
    err = (got - X.double() @ Y.double().t()).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"gemm_f32 {form} {shape} scale {scale:g}: max err {float(err.max()):.3e}, worst err / bound {worst:.4f}")
    assert bool((err <= bound).all()), (float(err.max()), worst)


@pytest.mark.parametrize("form", FORMS)
def test_deterministic_homogeneous_and_dirty_workspace(dev, form):
    L, rows, cols = 1000, 48, 64
    X, Y = _randn((rows, L), 5), _randn((cols, L), 6)
    a = _run(dev, form, X, Y)
    assert torch.equal(a, _run(dev, form, X, Y))
    for s in (2.0 ** -20, 2.0 ** 12):
        assert torch.equal(_run(dev, form, X * s, Y), a * s)
    if form == "tn":
        ws = torch.full((16 * 128 * 128,), float("nan"), device=dev)
        assert torch.equal(_run(dev, form, X, Y, workspace=ws), a)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("form", FORMS)
def test_nan_and_inf_stay_in_their_row_or_column(dev, form, bad):
    L, rows, cols = 129, 257, 130
    X, Y = _randn((rows, L), 7), _randn((cols, L), 8)
    clean = _run(dev, form, X, Y).cpu()
    Xb, Yb = X.clone(), Y.clone()
    Xb[200, 77], Yb[129, 128] = bad, bad
    for got, axis, at in ((_run(dev, form, Xb, Y).cpu(), 0, 200), (_run(dev, form, X, Yb).cpu(), 1, 129)):
        hit = got.select(axis, at)
        keep = torch.ones(rows if axis == 0 else cols, dtype=torch.bool)
        keep[at] = False
        assert not bool(torch.isfinite(hit).any())
        assert torch.equal(got.index_select(axis, keep.nonzero().flatten()),
                           clean.index_select(axis, keep.nonzero().flatten()))


@pytest.mark.parametrize("form", FORMS)
def test_padding_is_inert(dev, form):
    L, rows, cols = 65, 10, 100
    X, Y = _randn((rows, L), 9).to(dev), _randn((cols, L), 10).to(dev)
    fn = _lib.gemm_f32_nt if form == "nt" else _lib.gemm_f32_tn
    ops = (X, Y) if form == "nt" else (X.t().contiguous(), Y.t().contiguous())
    want = fn(*ops)

    def padded(t):   # the same rows in a 16-byte aligned buffer with NaN behind the extent: the fast path reads it
        big = torch.full((t.shape[0], t.shape[1] // 4 * 4 + 12), float("nan"), device=dev)
        big[:, :t.shape[1]] = t
        return big[:, :t.shape[1]]
    out = torch.full((rows, 112), -7.0, device=dev)
    got = fn(*(padded(t) for t in ops), out=out[:, :cols])
    assert torch.equal(got, want) and bool((out[:, cols:] == -7.0).all())

    def sliced(t):   # a column slice off a 16-byte boundary, and a base one float off: both copied by the wrapper
        big = torch.full((t.shape[0], t.shape[1] + 7), float("nan"), device=dev)
        big[:, 3:3 + t.shape[1]] = t
        return big[:, 3:3 + t.shape[1]]
    assert torch.equal(fn(sliced(ops[0]), ops[1]), want)
    flat = torch.zeros(ops[1].numel() + 1, device=dev)
    flat[1:] = ops[1].reshape(-1)
    assert torch.equal(fn(ops[0], flat[1:].view(ops[1].shape)), want)
    if form == "tn":
        zero = fn(ops[0][:0], ops[1][:0], out=torch.full((rows, cols), 5.0, device=dev))
        assert bool((zero == 0).all())
