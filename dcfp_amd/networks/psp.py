"""PSPNet `Seg_Model` — constructor, attributes, module names and forward contract of networks/psp.py:11-50.

The pyramid pooling module (networks/tools/ppm.py) runs its stages and concat as one autograd node,
ops.PyramidPoolingFn.  forward() follows networks/deeplabv3.py: with a criterion and labels the 8x upsample of both
heads is fused into the loss.  As in the reference there is no get_prune_params, and ignore_prune_layer comes from
backbone_para alone."""
import torch.nn as nn

from . import _exec
from .backbone import build_backbone
from .deeplabv3 import _deepsup_head, finish
from .tools.ppm import PPMModule


class Seg_Model(nn.Module):
    def __init__(self, backbone="resnet", backbone_para=None, model_para=None, num_classes=21,
                 align_corner=False, criterion=None, deepsup=False, **kwards):
        super().__init__()
        backbone_para = dict(backbone_para or {})  # the reference mutates its argument (psp.py:20)
        model_para = model_para or {}
        in_channels = model_para.get("in_channels", [1024, 2048])
        self.ignore_prune_layer = backbone_para.get("no_prune", ["backbone.layer4.2.bn3"])
        self.align_corner = align_corner
        backbone_para["out_index"] = [3, 4]
        self.backbone = build_backbone(backbone, backbone_para=backbone_para)
        self.ppm = PPMModule(in_channels[1], out_features=512, align_corners=self.align_corner)
        self.last_conv = nn.Conv2d(512, num_classes, kernel_size=1, stride=1)
        self.criterion = criterion
        self.deepsup = deepsup
        if self.deepsup:
            self.conv_deepsup = _deepsup_head(in_channels[0], num_classes)

    def lowres_logits(self, input, deepsup=False):
        """Logits of the head(s) at 1/os resolution (before the bilinear upsample)."""
        _exec.require_device(input)
        x_deepsup, x = self.backbone(input)
        lowres = [_exec.conv(self.last_conv, self.ppm(x))]
        if self.deepsup and deepsup:
            lowres.append(_exec.run_sequential(self.conv_deepsup, x_deepsup))
        return lowres

    def forward(self, input, labels=None, deepsup=False):
        return finish(self, input, self.lowres_logits(input, deepsup), labels)
