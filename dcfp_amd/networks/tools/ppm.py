"""Pyramid pooling module — module tree of networks/tools/ppm.py:10-38 on the HIP kernels.

Stages `stages.{k}` = (AdaptiveAvgPool2d(s), 1x1 conv, BatchNorm, ReLU) for s in `sizes`, then `bottleneck` = 3x3 conv
-> BatchNorm -> ReLU on the concat [stage 0, ..., stage 3, feats] (ppm.py:37).  The stages and the concat are ONE
autograd node, ops.PyramidPoolingFn: one sweep over feats pools every level and places feats in the concat buffer,
which is row-pitched for `bottleneck.0` in a training graph (dense for inference: conv2d_fused_infer reads dense
inputs).  The leaf modules hold parameters only."""
import torch
import torch.nn as nn

from .. import _exec
from ... import ops

BatchNorm2d = nn.BatchNorm2d


class PPMModule(nn.Module):
    def __init__(self, features, out_features=512, sizes=(1, 2, 3, 6), align_corners=True):
        super().__init__()
        self.align_corners = align_corners
        self.stages = nn.ModuleList([self._make_stage(features, out_features, size) for size in sizes])
        self.bottleneck = nn.Sequential(
            nn.Conv2d(features + len(sizes) * out_features, out_features, kernel_size=3, padding=1, dilation=1,
                      bias=False),
            BatchNorm2d(out_features),
            nn.ReLU(inplace=True))

    def _make_stage(self, features, out_features, size):
        prior = nn.AdaptiveAvgPool2d(output_size=(size, size))
        conv = nn.Conv2d(features, out_features, kernel_size=1, bias=False)
        bn = BatchNorm2d(out_features)
        act = nn.ReLU(inplace=True)
        return nn.Sequential(prior, conv, bn, act)

    def concat_pitch(self, shape):
        """Row pitch of the concat buffer of `shape`: the one `bottleneck.0` wants for its input (0: dense)."""
        return _exec._conv_pitch(self.bottleneck[0], shape)

    def forward(self, feats):
        sizes, tensors, bns = [], [], []
        for st in self.stages:
            pool, c = st[0], st[1]
            size = pool.output_size
            size = (size, size) if isinstance(size, int) else tuple(size)
            if size[0] != size[1] or size[0] is None:
                raise RuntimeError(f"dcfp_amd: unsupported pyramid stage pooling {pool}")
            if c.groups != 1 or c.bias is not None or c.kernel_size != (1, 1) or c.stride != (1, 1) \
                    or c.padding != (0, 0):
                raise RuntimeError(f"dcfp_amd: unsupported pyramid stage conv {c}")
            sizes.append(int(size[0]))
            tensors += [c.weight, st[2].weight, st[2].bias]
            bns.append(st[2])
        # row-pitched for a training graph; inference reads a dense concat (conv2d_fused_infer takes dense inputs)
        grad = torch.is_grad_enabled() and (feats.requires_grad or any(t.requires_grad for t in tensors))
        shape = (feats.shape[0], sum(int(t.shape[0]) for t in tensors[0::3]) + feats.shape[1]) + tuple(feats.shape[2:])
        cfg = {"sizes": sizes, "bn": [_exec._bn_args(b) for b in bns], "pitch": self.concat_pitch(shape) if grad else 0,
               "owner": self, "align": self.align_corners}
        cat = ops.pyramid_pooling(feats, cfg, tensors)
        return _exec.run_sequential(self.bottleneck, cat)
