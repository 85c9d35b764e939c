"""The training objective of the reference's train_one_epoch and evaluate (QViT_with_GETA/utils.py:197-366) on the
device: TrainLoss is one HIP call (qvit_train_loss, csrc/train_loss.hip) for the label-smoothed, mixed-up soft-target
cross-entropy (:120-154), the distillation KL against a teacher (:268-280), their blend, the correct-prediction count
(:261-262) and the gradient with respect to the logits. mixup is the input half of mixup_func (:142-154): it mixes
the images and hands the loss the label pair instead of a mixed [B, C] target.

    crit = TrainLoss(label_smoothing=0.1, kd_alpha=0.5, kd_temperature=5.0)
    images, mix = mixup(images, labels, alpha=0.2)
    res = crit(model(images), labels, teacher_logits=teacher(images), mix=mix)
    res.loss.backward()

The class count is logits.shape[1]. (The reference infers it from the largest label of the first batch,
utils.py:243-244; that quirk is not kept.) Nothing here synchronises the host.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import QvitError


class TrainLossResult(NamedTuple):
    loss: torch.Tensor         # (1 - kd_alpha) ce + kd_alpha kd, or ce alone: the scalar to call backward() on
    ce: torch.Tensor           # mean soft-target cross-entropy (detached, like the fields below)
    kd: torch.Tensor           # kl_div(..., 'batchmean') T^2; 0 without a teacher
    correct: torch.Tensor      # rows whose argmax is the hard label
    bad_labels: torch.Tensor   # rows with a label outside [0, C): they match no class


class _TrainLossFn(torch.autograd.Function):
    """One autograd node around the single call: the gradient is produced in the forward and saved."""

    @staticmethod
    def forward(ctx, logits, labels, teacher, labels_b, gamma, eps, kd_alpha, temperature):
        out, grad = _lib.train_loss(logits, labels, teacher, labels_b, gamma, eps, kd_alpha, temperature,
                                    want_grad=True)
        ctx.save_for_backward(grad)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return (grad * grad_out[0],) + (None,) * 7   # out[1:] are reports: nothing flows through them


class TrainLoss(torch.nn.Module):
    """criterion(logits, labels, teacher_logits=None, mix=None) -> TrainLossResult.

    logits: float32 [B, C] on the device, unit column stride, any row stride; labels: int64 [B] on the same device.
    teacher_logits: like logits, or None; without one, or with kd_alpha == 0, the loss is the cross-entropy alone
    (the reference's `loss = ce_loss` branch). mix: (labels[perm], gamma) from mixup(), or None. label_smoothing == 0
    and mix None is torch.nn.CrossEntropyLoss(), the form evaluate uses. Under no_grad, or for logits that need no
    gradient, the call skips the gradient pass and returns the same bits."""

    def __init__(self, label_smoothing: float = 0.0, kd_alpha: float = 0.0, kd_temperature: float = 1.0):
        super().__init__()
        for name, v in (("label_smoothing", label_smoothing), ("kd_alpha", kd_alpha)):
            if not 0.0 <= float(v) <= 1.0:
                raise QvitError(f"TrainLoss: {name} must lie in [0, 1] (got {v})")
        if not (math.isfinite(kd_temperature) and kd_temperature > 0.0):
            raise QvitError(f"TrainLoss: kd_temperature must be finite and positive (got {kd_temperature})")
        self.label_smoothing = float(label_smoothing)
        self.kd_alpha = float(kd_alpha)
        self.kd_temperature = float(kd_temperature)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor, teacher_logits: Optional[torch.Tensor] = None,
                mix: Optional[Tuple[torch.Tensor, float]] = None) -> TrainLossResult:
        labels_b, gamma = (None, 1.0) if mix is None else mix
        gamma = float(gamma)
        if not 0.0 <= gamma <= 1.0:
            raise QvitError(f"TrainLoss: the mix weight gamma must lie in [0, 1] (got {gamma})")
        teacher = None if teacher_logits is None else teacher_logits.detach()
        args = (labels, teacher, labels_b, gamma, self.label_smoothing, self.kd_alpha, self.kd_temperature)
        if torch.is_grad_enabled() and logits.requires_grad:
            out = _TrainLossFn.apply(logits, *args)
        else:
            out, _ = _lib.train_loss(logits, *args, want_grad=False)
        report = out.detach()
        return TrainLossResult(out[0], report[1], report[2], report[3], report[4])

    def extra_repr(self) -> str:
        return (f"label_smoothing={self.label_smoothing}, kd_alpha={self.kd_alpha}, "
                f"kd_temperature={self.kd_temperature}")


def mixup(images: torch.Tensor, labels: torch.Tensor, alpha: float = 0.2, gamma: Optional[float] = None,
          generator: Optional[torch.Generator] = None):
    """The reference's mixup_func (utils.py:142-154) with the target half left to TrainLoss: returns
    (gamma * images + (1 - gamma) * images[perm], (labels[perm], gamma)). gamma is a host draw from Beta(alpha, alpha)
    as in the reference (numpy's global state) unless given; the permutation comes from `generator` (a generator of
    the images' device) or torch's global state. The images are mixed on their device, out of place."""
    if not images.is_floating_point():
        raise QvitError(f"mixup: images must be a floating-point tensor (got dtype {images.dtype})")
    if labels.dim() != 1 or labels.shape[0] != images.shape[0] or labels.device != images.device:
        raise QvitError(f"mixup: labels must hold one label per image on the images' device (got shape "
                        f"{tuple(labels.shape)} on {labels.device} for {images.shape[0]} images on {images.device})")
    if gamma is None:
        gamma = float(np.random.beta(alpha, alpha))
    gamma = float(gamma)
    if not 0.0 <= gamma <= 1.0:
        raise QvitError(f"mixup: gamma must lie in [0, 1] (got {gamma})")
    perm = torch.randperm(images.shape[0], device=images.device, generator=generator)
    mixed = torch.lerp(images[perm], images, gamma)   # perm + gamma (images - perm)
    return mixed, (labels[perm], gamma)
