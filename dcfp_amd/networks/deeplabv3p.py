"""DeepLabv3+ `Decoder` / `Seg_Model` — constructor, attributes, module names and forward contract of
networks/deeplabv3p.py:12-94.

The decoder's concat (deeplabv3p.py:31-38) is ONE autograd node, ops.DecoderConcatFn: the bilinear resize of the ASPP
output and the 1x1 conv -> BN -> ReLU of the layer1 tap write their channel slices of one buffer, row-pitched for
`last_conv.0` (the 3x3 conv that reads it).  forward() follows networks/deeplabv3.py: with a criterion and labels the
upsample of both heads is fused into the loss (main head at 1/4 resolution, deep supervision at 1/8).
"""
import torch
import torch.nn as nn

from . import _exec
from .backbone import build_backbone
from .deeplabv3 import _deepsup_head, finish
from .tools.aspp import ASPP
from .. import ops

BatchNorm2d = nn.BatchNorm2d


class Decoder(nn.Module):
    def __init__(self, num_classes, align_corner, high_level_inplanes=512, low_level_inplanes=256):
        super().__init__()
        self.align_corner = align_corner
        self.conv1 = nn.Conv2d(low_level_inplanes, 48, 1, bias=False)
        self.bn1 = BatchNorm2d(48)
        self.relu = nn.ReLU(inplace=True)
        self.last_conv = nn.Sequential(
            nn.Conv2d(high_level_inplanes + 48, 256, kernel_size=3, stride=1, padding=1, bias=False),
            BatchNorm2d(256), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, kernel_size=3, stride=1, padding=1, bias=False),
            BatchNorm2d(256), nn.ReLU(inplace=True),
            nn.Conv2d(256, num_classes, kernel_size=1, stride=1))

    def concat_pitch(self, shape):
        """Row pitch of the concat buffer of `shape`: the one `last_conv.0` wants for its input (0: dense)."""
        return _exec._conv_pitch(self.last_conv[0], shape)

    def forward(self, x, low_level_feat):
        c = self.conv1
        if c.groups != 1 or c.bias is not None or c.kernel_size != (1, 1) or c.stride != (1, 1) or c.padding != (0, 0):
            raise RuntimeError(f"dcfp_amd: unsupported decoder conv1 {c}")
        # row-pitched for a training graph; inference reads a dense concat (conv2d_fused_infer takes dense inputs)
        grad = torch.is_grad_enabled() and (x.requires_grad or low_level_feat.requires_grad)
        shape = (x.shape[0], x.shape[1] + c.out_channels) + tuple(low_level_feat.shape[2:])
        cfg = {"bn": _exec._bn_args(self.bn1), "pitch": self.concat_pitch(shape) if grad else 0, "owner": self,
               "align": self.align_corner}
        cat = ops.decoder_concat(x, low_level_feat, cfg, c.weight, self.bn1.weight, self.bn1.bias)
        return _exec.run_sequential(self.last_conv, cat)


class Seg_Model(nn.Module):
    def __init__(self, backbone="resnet", backbone_para=None, model_para=None, num_classes=21,
                 align_corner=False, criterion=None, deepsup=False, **kwards):
        super().__init__()
        backbone_para = dict(backbone_para or {})  # the reference mutates its argument (deeplabv3p.py:66)
        model_para = model_para or {}
        output_stride = backbone_para.get("os", 8)
        in_channels = model_para.get("in_channels", [256, 1024, 2048])
        self.ignore_prune_layer = model_para.get("no_prune", ["decoder.bn1", "aspp.bn1"]) \
            + backbone_para.get("no_prune", ["backbone.layer4.2.bn3"])
        self.align_corner = align_corner
        backbone_para["out_index"] = [1, 3, 4]
        self.backbone = build_backbone(backbone, backbone_para=backbone_para)
        self.aspp = ASPP(output_stride, self.align_corner, inplanes=in_channels[2])
        self.decoder = Decoder(num_classes, self.align_corner, low_level_inplanes=in_channels[0])
        self.criterion = criterion
        self.deepsup = deepsup
        if self.deepsup:
            self.conv_deepsup = _deepsup_head(in_channels[1], num_classes)

    def lowres_logits(self, input, deepsup=False):
        """Logits of the head(s) before the bilinear upsample: the decoder's at 1/4 resolution, deep supervision at 1/8."""
        _exec.require_device(input)
        low, x_deepsup, x = self.backbone(input)
        x = self.aspp(x)
        lowres = [self.decoder(x, low)]
        if self.deepsup and deepsup:
            lowres.append(_exec.run_sequential(self.conv_deepsup, x_deepsup))
        return lowres

    def forward(self, input, labels=None, deepsup=False):
        return finish(self, input, self.lowres_logits(input, deepsup), labels)

    def get_prune_params(self):
        for name, m in self.named_modules():
            if isinstance(m, (nn.BatchNorm2d, nn.SyncBatchNorm)) and name not in self.ignore_prune_layer:
                yield m.weight
