"""TrainLoss (qvit_train_loss) on the device against tests/train_loss_ref.py in float64 under autograd.

Bars. For each kind of output the floor is the largest error of the float32 transcription against the float64 one
over CASES (_errors(_reference(..., torch.float32), _ref64(...)): computed on the CPU, without the kernel), and the
bar is 8 times the floor: room for another summation order and the device's exp and log, while a
wrong term, a missed column or a wrong scale shows at 1e-3 or worse.
  scalars (loss, ce, kd): |x - ref64| / max(1, |ref64|); floor SCALAR_FLOOR = 1.489e-6 (1 x 3 with the full objective
    at T = 5: the T^2 = 25 in front of a small KL; the other cases lie between 2e-8 and 6e-7).
  gradient: B |dlogits - ref64|, so that the bar does not depend on the batch; floor GRAD_FLOOR = 5.838e-7 (3 x 21843
    with the full objective; the others between 5e-8 and 5e-7).
correct and bad_labels are compared exactly."""
import functools

import pytest
import torch

import train_loss_ref as R
from quantized_vit_amd import TrainLoss

pytestmark = pytest.mark.gpu

SCALAR_FLOOR, GRAD_FLOOR = 1.489e-6, 5.838e-7
SCALAR_BAR, GRAD_BAR = 8 * SCALAR_FLOOR, 8 * GRAD_FLOOR

# (B, C, row stride or None); 4096 | 4097: the last register-resident row length and the first that is read twice
SHAPES = [(1, 3, None), (5, 10, None), (7, 100, None), (4, 1000, None), (3, 1001, None), (6, 1024, 1032),
          (2, 4096, None), (2, 4097, None), (3, 21843, None)]
# name: (label_smoothing, gamma of the mixup or None, T of the distillation or None)
MODES = {"hard": (0.0, None, None), "smooth": (0.1, None, None), "mix_g0": (0.1, 0.0, None),
         "mix_g0.3": (0.1, 0.3, None), "mix_g1": (0.1, 1.0, None), "full_T1": (0.1, 0.3, 1.0),
         "full_T5": (0.1, 0.3, 5.0)}
# every shape with the full objective; every mode at an aligned (4 x 1000) and an unaligned (5 x 10) shape; the
# last case scales the logits so that rows reach +-80 at T = 1
CASES = [(s, "full_T5", 1.0) for s in SHAPES] + [(s, m, 1.0) for s in (SHAPES[3], SHAPES[1]) for m in list(MODES)[:6]]
CASES += [(SHAPES[3], "full_T1", 80.0), (SHAPES[1], "full_T1", 80.0)]
IDS = [f"{s[0]}x{s[1]}{'_ld%d' % s[2] if s[2] else ''}-{m}{'-pm80' if top != 1.0 else ''}" for s, m, top in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(B, C, top):
    """Seeded CPU inputs: logits and teacher randn * 3 (or scaled to reach +-top), labels with columns 0 and C - 1
    and the row's argmax at odd rows, and a permutation with the fixed point 0."""
    g = torch.Generator().manual_seed(1000 * B + C)
    s, t = torch.randn(B, C, generator=g) * 3, torch.randn(B, C, generator=g) * 3
    if top != 1.0:
        s, t = s * (top / s.abs().max()), t * (top / t.abs().max())
    labels = torch.randint(0, C, (B,), generator=g)
    labels[1::2] = s[1::2].argmax(dim=1)
    labels[0], labels[-1] = 0, C - 1
    perm = torch.cat([torch.zeros(1, dtype=torch.int64), torch.arange(1, B).roll(1)])
    return s, t, labels, perm


def _reference(s, t, labels, perm, mode, dtype):
    """(loss, ce, kd, correct, B * dlogits) of the transcription in `dtype`, as float64 CPU tensors."""
    eps, gamma, T = MODES[mode]
    x = s.to(dtype, copy=True).requires_grad_(True)
    loss, ce, kd, correct = R.objective(x, labels, eps or None, perm if gamma is not None else None, gamma,
                                        t if T else None, 0.5 if T else 0.0, T or 1.0, dtype)
    loss.backward()
    return [v.detach().double() for v in (loss, ce, kd, correct, x.grad * s.shape[0])]


@functools.lru_cache(maxsize=None)
def _ref64(B, C, mode, top):
    return _reference(*_inputs(B, C, top), mode, torch.float64)


def _errors(got, ref):
    """(largest scalar error, largest gradient error) of (loss, ce, kd, _, B * dlogits) against the reference."""
    scalar = max((abs(g - r) / max(1.0, abs(r))).item() for g, r in zip(got[:3], ref[:3]))
    return scalar, (got[4] - ref[4]).abs().max().item()


def _on_device(x, ld, dev):
    """x [B, C] on the device, dense or as a view of NaN-padded rows of pitch ld."""
    if ld is None:
        return x.to(dev)
    buf = torch.full((x.shape[0], ld), float("nan"), device=dev)
    buf[:, :x.shape[1]] = x.to(dev)
    return buf[:, :x.shape[1]]


def _run(dev, s, t, labels, perm, mode, ld=None, grad=True, scale=1.0):
    eps, gamma, T = MODES[mode]
    crit = TrainLoss(label_smoothing=eps, kd_alpha=0.5 if T else 0.0, kd_temperature=T or 1.0)
    x = _on_device(s, ld, dev).requires_grad_(grad)
    labels = labels.to(dev)
    res = crit(x, labels, teacher_logits=_on_device(t, ld, dev) if T else None,
               mix=(labels[perm.to(dev)], gamma) if gamma is not None else None)
    if grad:
        (scale * res.loss).backward()
    return res, x.grad


@pytest.mark.parametrize("shape,mode,top", CASES, ids=IDS)
def test_matches_float64_reference(dev, shape, mode, top):
    """Fails without the feature: the package has no TrainLoss."""
    B, C, ld = shape
    ref = _ref64(B, C, mode, top)
    res, grad = _run(dev, *_inputs(B, C, top), mode, ld)
    got = [res.loss.detach().double().cpu(), res.ce.double().cpu(), res.kd.double().cpu(), None, grad.double().cpu() * B]
    scalar, gerr = _errors(got, ref)
    print(f"train_loss {B}x{C} {mode}: scalar error {scalar:.3e} (bar {SCALAR_BAR:.1e}), gradient error {gerr:.3e} "
          f"(bar {GRAD_BAR:.1e})")
    assert all(bool(torch.isfinite(v).all()) for v in (got[0], got[1], got[2], got[4]))
    assert res.correct.item() == ref[3].item() and res.bad_labels.item() == 0
    assert scalar <= SCALAR_BAR and gerr <= GRAD_BAR


@pytest.mark.parametrize("C", [10, 1000, 5000])
def test_argmax_ties_take_the_first_column(dev, C):
    s = _inputs(2, C, 1.0)[0].clone()
    s[1] = s[0]
    lo, hi = 1, C - 2
    s[:, lo] = s[:, hi] = s.max() + 1.0
    assert torch.argmax(s, dim=1).tolist() == [lo, lo]
    for labels, want in (([lo, lo], 2), ([lo, hi], 1), ([hi, hi], 0)):
        res = TrainLoss()(s.to(dev), torch.tensor(labels, device=dev))
        assert res.correct.item() == want, labels


@pytest.mark.parametrize("C,mode", [(10, "hard"), (1000, "full_T5")])
def test_labels_out_of_range_match_no_class(dev, C, mode):
    s, t, labels, perm = _inputs(5, C, 1.0)
    labels = labels.clone()
    labels[1], labels[3] = -1, C
    bad = (labels < 0) | (labels >= C)
    if MODES[mode][1] is not None:
        bad = bad | bad[perm]                     # a row is bad when either label of its pair is
    ref = _reference(s, t, labels, perm, mode, torch.float64)      # (finite: the one-hot term of those rows dropped)
    res, grad = _run(dev, s, t, labels, perm, mode)
    assert all(bool(torch.isfinite(v).all()) for v in (res.loss, res.ce, res.kd, grad))
    assert res.bad_labels.item() == bad.sum().item() and res.correct.item() == ref[3].item()
    gerr = (grad.double().cpu() * 5 - ref[4])[~bad].abs().max().item()
    assert gerr <= GRAD_BAR                       # the rows with valid labels are the reference's


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[8]], ids=["5x10", "4x1000", "3x21843"])
def test_no_grad_form_and_reruns_give_the_same_bits(dev, shape):
    args = _inputs(shape[0], shape[1], 1.0)
    res1, g1 = _run(dev, *args, "full_T5")
    res2, g2 = _run(dev, *args, "full_T5")
    res3, g3 = _run(dev, *args, "full_T5", scale=2.5)
    with torch.no_grad():
        res0, _ = _run(dev, *args, "full_T5", grad=False)
    assert torch.equal(g1, g2) and torch.equal(g3, 2.5 * g1)
    for other in (res0, res2):
        assert torch.equal(torch.stack(list(other)).detach(), torch.stack(list(res1)).detach())
    assert not res0.loss.requires_grad and res1.loss.requires_grad
