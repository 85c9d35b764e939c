"""CPU reference of qvit_quant_error and the seeded data sets its tests share.

fq comes from oracle.quant_oracle.fake_quant in fp32; the target is x (linear) or sign(x) * input_pow with input_pow the
un-rounded fp32 power of SymQuantizerNonLinear.forward (quant_layers.py:63); squares and sums are float64; nclip is an
exact count of |x| >= q_m."""
import math

import numpy as np
import torch

from oracle import quant_oracle as O

QT_NAMES = {0: O.LINEAR, 1: O.NONLINEAR}


def target(x: torch.Tensor, qtype: int, t: float) -> torch.Tensor:
    """The fp32 value the quantizer rounds: x, or sign(x) * exp(t * log|x|) as the reference's forward takes it."""
    if qtype == 0:
        return x
    tt = torch.tensor([float(t)], dtype=torch.float32)
    return torch.sign(x) * torch.exp(tt * torch.log(torch.abs(x)))


def quant_error_terms(x: torch.Tensor, qtype: int, d: float, q_m: float, t: float = 1.0) -> torch.Tensor:
    """((double)p - (double)fq)^2 per element, float64, shaped as x."""
    x = x.detach().cpu().float()
    fq = O.fake_quant(x.clone(), QT_NAMES[qtype], float(d), float(q_m), float(t))
    return (target(x, qtype, t).double() - fq.double()).square()


def quant_error(x: torch.Tensor, qtype: int, d, q_m, t: float = 1.0):
    """(err float64 [ncand], nclip int64 [ncand]) of x under the candidates (d[c], q_m[c])."""
    x = x.detach().cpu().float()
    d = torch.as_tensor(d, dtype=torch.float32).reshape(-1)
    q_m = torch.as_tensor(q_m, dtype=torch.float32).reshape(-1)
    err = torch.zeros(d.numel(), dtype=torch.float64)
    nclip = torch.zeros(d.numel(), dtype=torch.int64)
    for c in range(d.numel()):
        err[c] = quant_error_terms(x, qtype, d[c].item(), q_m[c].item(), t).sum()
        nclip[c] = (x.abs() >= q_m[c]).sum()
    return err, nclip


def power_slack(x: torch.Tensor, qtype: int, d, q_m, t: float = 1.0) -> torch.Tensor:
    """How far err[c] may move, float64 [ncand], when another correct fp32 routine evaluates exp(t log|x|) (nonlinear
    type; zeros for the linear one). Two 1-ulp routines differ by one ulp in log|x|, which the exponential turns into
    |t ln|x|| ulps of p, plus one ulp each of their own: delta_i = (2 + 2 |t ln|x_i||) ulp(p_i). A term (p - fq)^2
    then moves by at most 2 |p - fq| delta + delta^2, or, where the move carries p / d across a rounding tie and fq
    jumps by d, by (d/2 + delta)^2 - (d/2 - delta)^2 = 2 d delta with |p - fq| >= d/2 - delta. Both are below
    (4 |p - fq| + d) delta, which is summed here. Saturated and zero elements are selected by x itself, not by p."""
    x = x.detach().cpu().float()
    d = torch.as_tensor(d, dtype=torch.float32).reshape(-1)
    q_m = torch.as_tensor(q_m, dtype=torch.float32).reshape(-1)
    out = torch.zeros(d.numel(), dtype=torch.float64)
    if qtype == 0:
        return out
    p = target(x, qtype, t)
    finite = torch.isfinite(p) & (x != 0)
    ulp = torch.from_numpy(np.spacing(np.abs(p.numpy()))).double()
    lg = torch.log(x.abs().double().clamp_min(1e-300)).abs() * abs(t)
    delta = torch.where(finite, (2.0 + 2.0 * lg) * ulp, torch.zeros((), dtype=torch.float64))
    for c in range(d.numel()):
        fq = O.fake_quant(x.clone(), QT_NAMES[qtype], d[c].item(), q_m[c].item(), float(t))
        out[c] = ((4.0 * (p.double() - fq.double()).abs() + d[c].double()) * delta).sum()
    return out


def candidates(absmax: float, bits: int, t: float = 1.0, num: int = 32, min_frac: float = 0.2):
    """clip_candidates of calibrate.py restated: q_m_c = absmax (min_frac + (1 - min_frac) c / (num - 1)) and
    d_c = q_m_c^t / (2^(bits-1) - 1), as fp32 tensors (num == 1: the absmax choice alone)."""
    fr = [1.0] if num == 1 else [min_frac + (1.0 - min_frac) * c / (num - 1) for c in range(num)]
    qm = [absmax * f for f in fr]
    d = [math.exp(t * math.log(abs(q))) / (2 ** (bits - 1) - 1) for q in qm]
    return torch.tensor(qm, dtype=torch.float32), torch.tensor(d, dtype=torch.float32)


# ---- the data sets of the selection test -----------------------------------------------------------------------
# (name, bits, seed): heavy-tailed activations at 8 bits (a Student-t tail on a normal body, as a residual stream
# or a GELU output has), weight-like data at 4 bits (normal, std 0.02). tests/test_quant_error_ref_cpu.py vets every
# entry: the best and the runner-up candidate are at least 1e-6 apart, relatively. A seed that fails goes here.
SELECTION_SETS = [("heavy_tailed", 8, 11), ("heavy_tailed", 8, 12), ("weight_like", 4, 21), ("weight_like", 4, 22)]
SELECTION_SHAPE = (37, 200)
SELECTION_NUM = 32


def selection_data(kind: str, seed: int) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    n = SELECTION_SHAPE[0] * SELECTION_SHAPE[1]
    if kind == "heavy_tailed":
        v = rng.standard_normal(n) + 0.05 * rng.standard_t(2.5, n) * 8.0
    else:
        v = 0.02 * rng.standard_normal(n)
    return torch.from_numpy(v.astype(np.float32)).reshape(SELECTION_SHAPE)


def selection_case(kind: str, bits: int, seed: int, qtype: int = 0, t: float = 1.0):
    """(x, q_m, d) of one selection data set."""
    x = selection_data(kind, seed)
    q_m, d = candidates(float(x.abs().max()), bits, t, SELECTION_NUM)
    return x, q_m, d


def argmin_larger_qm(err: torch.Tensor) -> int:
    """Index of the smallest error; ties go to the larger q_m (the later candidate)."""
    e = err.detach().cpu().double()
    return int((e == e.min()).nonzero().max())
