"""The reference's training objective in plain torch, as QViT_with_GETA/utils.py writes it: one_hot (:120-130),
mixup_func on the targets (:142-154), cross_entropy_onehot_target (:133-139), the distillation lines (:268-280) and
torch.max(pred, dim=1)[1] (:261-262). It takes a dtype, so the same code is the float64 reference and the float32
error floor of tests/test_gpu_train_loss.py, and a device, so tools/train_loss_bench.py times it.

One departure: F.one_hot refuses a label outside [0, C), so the one-hot is a comparison against the class indices,
which is F.one_hot for every valid label and a zero row (the one-hot term dropped) for an invalid one."""
import torch
import torch.nn.functional as F


def one_hot(y, num_classes, smoothing_eps=None, dtype=torch.float32):
    one_hot_y = (y[:, None] == torch.arange(num_classes, device=y.device)[None, :]).to(dtype)
    if smoothing_eps is None:
        return one_hot_y
    v1 = 1 - smoothing_eps + smoothing_eps / float(num_classes)
    v0 = smoothing_eps / float(num_classes)
    return one_hot_y * (v1 - v0) + v0


def cross_entropy_onehot_target(logit, target):
    prob_logit = F.log_softmax(logit, dim=1)
    return -(target * prob_logit).sum(dim=1).mean()


def objective(pred, labels, eps=None, perm=None, gamma=1.0, teacher=None, kd_alpha=0.0, T=1.0, dtype=torch.float64):
    """(loss, ce, kd, correct) of train_one_epoch for one batch of logits `pred`; with grad if pred requires it.
    eps None: no smoothing; perm None: no mixup (else the targets are mixed with targets[perm] at gamma)."""
    pred = pred.to(dtype)
    C = pred.shape[1]
    valid = bool(((labels >= 0) & (labels < C)).all())
    if eps is None and perm is None and valid:
        ce = F.cross_entropy(pred, labels)                       # criterion = torch.nn.CrossEntropyLoss() (:213)
    else:
        targets = one_hot(labels, C, eps, dtype)
        if perm is not None:
            targets = targets * gamma + (1 - gamma) * targets[perm]     # targets.mul_(gamma).add_(1 - gamma, ...)
        ce = cross_entropy_onehot_target(pred, targets)
    correct = torch.eq(torch.max(pred, dim=1)[1], labels).sum()
    kd = torch.zeros((), dtype=dtype, device=pred.device)
    loss = ce
    if teacher is not None and kd_alpha > 0.0:
        log_p_student = F.log_softmax(pred / T, dim=1)
        p_teacher = F.softmax(teacher.to(dtype) / T, dim=1)
        kd = F.kl_div(log_p_student, p_teacher, reduction='batchmean') * (T * T)
        loss = (1.0 - kd_alpha) * ce + kd_alpha * kd
    return loss, ce, kd, correct
