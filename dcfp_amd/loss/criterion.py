"""Criterion factory and CE(+deep supervision) loss — API of loss/criterion.py:11-74.

`CriterionDSN.forward(preds, target)` keeps the reference contract (full-resolution logits
in, {'loss': t} out).  `forward_lowres(preds_lr, target, size, align_corner)` is the fused
entry Seg_Model.forward uses: bilinear upsample + log-softmax + NLL in one HIP kernel per
head (the 637 MB/head full-resolution logits are never written).
Both go through dcfp_upsample_ce_*; a full-resolution input is the h==H special case
(source index == destination index, lambda == 0: the interpolation is exact)."""
import torch
import torch.nn as nn

from .. import ops
from .ohem import CriterionOhemDSN  # noqa: F401  (reference imports it here, criterion.py:7)


def build_criterions(loss_type, dataset, loss_para):
    if len(loss_type.split(",")) > 1:
        return CombinedCriterion(loss_type, dataset, loss_para)
    return build_criterion(loss_type, dataset, loss_para)


def build_criterion(loss_type, dataset, loss_para):
    if loss_type == "ce":
        cls = CriterionDSN
    elif loss_type == "ohem":
        cls = CriterionOhemDSN
    elif loss_type == "gsrl":
        cls = CriterionGsrlDSN
    elif loss_type == "kd":
        cls = CriterionKD
    elif loss_type == "kdpa":
        cls = CriterionKDPairwise
    elif loss_type == "lovasz":
        cls = CriterionLovasz
    else:
        raise NotImplementedError(loss_type)
    return cls(dataset=dataset, **loss_para)


def class_weighted_ce(logits, target, class_weights, size, align_corner, ignore_index, pixel_keep=None):
    """nn.CrossEntropyLoss(weight=w, ignore_index, 'mean') of the upsampled logits (criterion.py:54-60):
    sum_i w[y_i] * nll_i / sum_i w[y_i] over the valid (and kept) pixels, through the fused weighted-CE
    kernels with the per-pixel weight w[y_i]."""
    w = class_weights.to(device=logits.device, dtype=torch.float32)
    valid = target != ignore_index
    if pixel_keep is not None:
        valid = valid & (pixel_keep != 0)
    pix_w = w[target.clamp(min=0, max=w.numel() - 1)] * valid
    out = ops.upsample_weighted_ce(logits, target, pix_w, size, align_corner, ignore_index)   # [N, 2] = (sum w*ce, sum w)
    return out[:, 0].sum() / out[:, 1].sum()


class CombinedCriterion(nn.Module):
    """criterion.py:30-45: sum of the 'loss' entries of several criteria."""

    def __init__(self, loss_types, dataset=None, loss_para={}):
        super().__init__()
        self.criterions = [build_criterion(t, dataset, loss_para) for t in loss_types.split(",")]

    def attach(self, seg_model):
        """Hand the bare model to the criteria that tap it (CriterionKDPairwise)."""
        for c in self.criterions:
            if hasattr(c, "attach"):
                c.attach(seg_model)
        return self

    def forward(self, preds, labels):
        loss, total = {}, 0.0
        for c in self.criterions:
            part = c(preds, labels)
            total = total + part["loss"]
            loss.update(part)
        loss["loss"] = total
        return loss

    def forward_lowres(self, preds_lr, labels, size, align_corner):
        loss, total = {}, 0.0
        for c in self.criterions:
            part = c.forward_lowres(preds_lr, labels, size, align_corner)
            total = total + part["loss"]
            loss.update(part)
        loss["loss"] = total
        return loss


class CriterionDSN(nn.Module):
    """CE(main) + ds_weight * CE(deep supervision), ignore_index = dataset.ignore_label,
    mean over valid pixels (criterion.py:48-74)."""

    def __init__(self, dataset=None, ds_weight=0.4, balance_weight=False, **kwargs):
        super().__init__()
        self.ignore_index = dataset.ignore_label
        self.ds_weight = ds_weight
        # criterion.py:54-60: nn.CrossEntropyLoss(weight=dataset.class_weights) when balance_weight
        self.class_weights = None
        if balance_weight:
            self.class_weights = torch.as_tensor(dataset.class_weights, dtype=torch.float32)

    def _ce(self, logits, target, size, align_corner):
        if self.class_weights is not None:
            return class_weighted_ce(logits, target, self.class_weights, size, align_corner, self.ignore_index)
        return ops.upsample_cross_entropy(logits, target, size, align_corner, self.ignore_index)

    def forward_lowres(self, preds, target, size, align_corner):
        if isinstance(target, dict):
            target = target["ori"]
        loss = self._ce(preds[0], target, size, align_corner)
        if len(preds) >= 2:
            loss = loss + self._ce(preds[1], target, size, align_corner) * self.ds_weight
        return {"loss": loss}

    def forward(self, preds, target):
        if isinstance(preds, dict):
            preds, target = [preds["pred"], preds["deepsup"]], target["ori"]
        size = target.shape[-2:]
        return self.forward_lowres(list(preds), target, size, True)


class CriterionGsrlDSN(nn.Module):
    """Fine-tune loss of DCFP (criterion.py:77-101): per-pixel balance weights, dilated by a k x k
    max filter and multiplied by the calibration factor 1 + gamma*(1 - (p1 - p2)) of the main
    head's top-2 softmax margin, weight CE(main) and CE(deep supervision); each is normalised
    per image by its weight sum and averaged over the batch.
    labels: {'ori': int64 [N,H,W], 'weight': float [N,H,W]}."""

    def __init__(self, dataset=None, ds_weight=0.4, k=9, gamma=9, **kwargs):
        super().__init__()
        self.k = k
        self.gamma = gamma
        self.ignore_index = dataset.ignore_label
        self.ds_weight = ds_weight

    def _term(self, logits, ori, weight, size, align_corner):
        out = ops.upsample_weighted_ce(logits, ori, weight, size, align_corner, self.ignore_index)
        return torch.mean(out[:, 0] / (out[:, 1] + 1e-8))

    def forward_lowres(self, preds, labels, size, align_corner):
        ori = labels["ori"]
        with torch.no_grad():
            weight = ops.maxfilter2d(labels["weight"].to(torch.float32), self.k)
            margin = ops.upsample_margin(preds[0].detach(), size, align_corner)
            weight = (1 + self.gamma * (1 - margin)) * weight
            weight[ori == self.ignore_index] = 0.0
        loss = self._term(preds[0], ori, weight, size, align_corner)
        if len(preds) >= 2:
            loss = loss + self.ds_weight * self._term(preds[1], ori, weight, size, align_corner)
        return {"loss": loss}

    def forward(self, preds, labels):
        return self.forward_lowres(list(preds), labels, labels["ori"].shape[-2:], True)


class CriterionKD(nn.Module):
    """Distillation term of the fine-tune stage: kd_weight * ops.kd_loss(main-head logits, teacher logits) at the
    heads' low resolution.  The teacher's logits travel with the labels, as labels['teacher']
    (distill.Teacher makes them, tools/train.py --teacher-from puts them there); the deep-supervision head is not
    distilled.  kd_mode "pixel": KL over the classes per pixel; "channel": KL over the positions per class plane.
    Combined with a supervised loss as `--loss-type ce,kd` / `gsrl,kd`."""

    def __init__(self, dataset=None, kd_weight=1.0, kd_T=1.0, kd_mode="pixel", **kwargs):
        super().__init__()
        if kd_mode not in ops.KD_MODES:
            raise ValueError(f"CriterionKD: kd_mode {kd_mode!r} is not one of {sorted(ops.KD_MODES)}")
        if not float(kd_T) > 0.0:
            raise ValueError(f"CriterionKD: kd_T must be positive, got {kd_T}")
        self.kd_weight, self.kd_T, self.kd_mode = float(kd_weight), float(kd_T), kd_mode

    def _term(self, student, labels):
        if not isinstance(labels, dict) or "teacher" not in labels:
            raise ValueError("CriterionKD: labels must be a dict that holds the teacher's low-resolution logits under "
                             "'teacher' (distill.Teacher; tools/train.py --teacher-from)")
        teacher = labels["teacher"]
        if tuple(teacher.shape) != tuple(student.shape):
            raise ValueError(f"CriterionKD: the teacher's logits {tuple(teacher.shape)} and the student's "
                             f"{tuple(student.shape)} differ in shape")
        return {"loss": self.kd_weight * ops.kd_loss(student, teacher, self.kd_T, self.kd_mode)}

    def forward_lowres(self, preds, labels, size, align_corner):
        return self._term(preds[0], labels)

    def forward(self, preds, labels):
        if isinstance(preds, dict):
            preds = [preds["pred"]]
        return self._term(preds[0], labels)


class CriterionKDPairwise(nn.Module):
    """Pair-wise similarity distillation of the fine-tune stage: pa_weight * ops.pairwise_kd_loss(student
    feature, teacher feature, pa_pool) on the backbone's last tensor.  The student's feature does not travel with the
    predictions: attach(seg_model) puts a distill.FeatureTap on the bare model and every call pops it; the teacher's
    travels with the labels, as labels['teacher_feat'] (distill.Teacher(images, feature=True); tools/train.py
    --teacher-from).  The two may differ in channels.  Combined with a supervised loss as `--loss-type gsrl,kdpa` /
    `gsrl,kd,kdpa`; every rank takes the loss of its own batch."""

    def __init__(self, dataset=None, pa_weight=1.0, pa_pool=2, **kwargs):
        super().__init__()
        if not float(pa_weight) >= 0.0:
            raise ValueError(f"CriterionKDPairwise: pa_weight must not be negative, got {pa_weight}")
        if isinstance(pa_pool, bool) or not isinstance(pa_pool, int) or pa_pool < 1:
            raise ValueError(f"CriterionKDPairwise: pa_pool must be an int >= 1, got {pa_pool!r}")
        self.pa_weight, self.pa_pool = float(pa_weight), pa_pool
        self._tap = None

    def attach(self, seg_model):
        """Tap the backbone output of `seg_model` (the bare Seg_Model, under any wrapper)."""
        from ..distill import FeatureTap
        if self._tap is not None:
            self._tap.remove()
        self._tap = FeatureTap(seg_model)
        return self

    def _term(self, labels):
        if self._tap is None:
            raise ValueError("CriterionKDPairwise: attach(seg_model) first - the student's feature comes from a tap on "
                             "its backbone")
        if not isinstance(labels, dict) or "teacher_feat" not in labels:
            raise ValueError("CriterionKDPairwise: labels must be a dict that holds the teacher's feature under "
                             "'teacher_feat' (distill.Teacher(images, feature=True); tools/train.py --teacher-from)")
        student = self._tap.pop()
        if student is None:
            raise ValueError("CriterionKDPairwise: the tap holds no feature - the attached model made no training-mode "
                             "forward with grad enabled since the last call")
        return {"loss": self.pa_weight * ops.pairwise_kd_loss(student, labels["teacher_feat"], self.pa_pool)}

    def forward_lowres(self, preds, labels, size, align_corner):
        return self._term(labels)

    def forward(self, preds, labels):
        return self._term(labels)


class CriterionLovasz(nn.Module):
    """Lovasz-Softmax term of the fine-tune stage: lovasz_weight * ops.lovasz_softmax(main-head logits, labels), the
    convex surrogate of the per-class Jaccard index (Berman et al. 2018) over the classes present in the batch, computed
    from the low-resolution logits with `lovasz_bins` error bins in place of a sort.  Only the main head
    gets the term; every rank takes the loss of its own batch (no histogram is shared between data-parallel ranks), and
    the paper's per_image and classes='all' modes are not offered.  Combined with a supervised loss as
    `--loss-type ce,lovasz` / `gsrl,lovasz`; labels may be the tensor or the dict (labels['ori'])."""

    def __init__(self, dataset=None, lovasz_weight=1.0, lovasz_bins=1024, **kwargs):
        super().__init__()
        if isinstance(lovasz_bins, bool) or lovasz_bins not in ops.LOVASZ_BINS:
            raise ValueError(f"CriterionLovasz: lovasz_bins must be a power of two in 64 .. 4096, got {lovasz_bins!r}")
        if not float(lovasz_weight) >= 0.0:
            raise ValueError(f"CriterionLovasz: lovasz_weight must not be negative, got {lovasz_weight}")
        self.lovasz_weight, self.lovasz_bins = float(lovasz_weight), int(lovasz_bins)
        self.ignore_index = dataset.ignore_label

    def forward_lowres(self, preds, labels, size, align_corner):
        if isinstance(labels, dict):
            labels = labels["ori"]
        term = ops.lovasz_softmax(preds[0], labels, size, align_corner, self.ignore_index, self.lovasz_bins)
        return {"loss": self.lovasz_weight * term}

    def forward(self, preds, labels):
        if isinstance(preds, dict):
            preds = [preds["pred"]]
        if isinstance(labels, dict):
            labels = labels["ori"]
        return self.forward_lowres(list(preds), labels, labels.shape[-2:], True)
