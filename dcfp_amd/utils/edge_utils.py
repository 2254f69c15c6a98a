"""Boundary-IoU helpers under the names of the reference's utils/edge_utils.py:98-127, on device tensors: the
per-class erosions of the reference are one HIP kernel family over the label map here (ops.label_boundary)."""
from math import sqrt

from .. import ops


def boundary_dilation(h, w, dilation_ratio=0.02):
    """Width d of the boundary band for an h x w map: the ratio times the image diagonal, rounded as Python rounds,
    at least 1."""
    return max(1, int(round(dilation_ratio * sqrt(h * h + w * w))))


def mask_to_boundary(mask, num_classes, dilation_ratio=0.02, background=255):
    """[H,W] or [N,H,W] int32 / int64 device label map -> the same map with every pixel further than d from a class
    boundary (or the image border) set to `background`, as are pixels outside [0, num_classes)."""
    h, w = mask.shape[-2:]
    return ops.label_boundary(mask, num_classes, boundary_dilation(h, w, dilation_ratio), background)
