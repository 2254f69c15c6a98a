"""The yardstick of tests/test_deploy_heads_gpu.py for the DeepLabv3+ and PSPNet engines: the eval-mode forward of the
two heads on the CPU as a pure function of a state_dict, which never touches dcfp_amd.deploy.  A plain helper module
like tests/_deploy_ref.py (whose rules it keeps): no fixtures, no tests.

The backbone loop uses oracle.model's tables (strides / dilations per output stride, block counts, multi-grid); the
layer1 tap, the ASPP, the decoder (networks/deeplabv3p.py:31-38) and the pyramid (networks/tools/ppm.py:29-38) are
restated in torch.nn.functional.  One forward, two sets of rules:

  * _Exact: conv -> F.batch_norm in the tensors' own dtype.  In fp64 this is the truth (eval_logits64).
  * _Fp16Storage: what the engine stores.  BatchNorm folded into the conv in fp64, the folded weight rounded to fp16
    once, the shift fp32; the residual added before the one rounding; every tensor the engine stores rounded to fp16 -
    the image, each conv output, the pooled maps, the stage outputs, the resized maps (and with them every concat
    input); the classifier's output is not rounded.  The convolutions, pools and interpolations run in `dtype` (fp64:
    exact sums of the rounded values; fp32: one more summation order).

yardstick(sd, x, cfg) -> (ref64, e, r) as tests/_deploy_ref.py defines it."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import model as omodel  # noqa: E402


def h16(t):
    """Round to fp16 and back (the engine's storage format)."""
    return t.to(torch.float16).to(t.dtype)


class _Exact:
    """conv -> BatchNorm (-> + residual) (-> ReLU) in the dtype of `sd`."""

    def __init__(self, sd, cfg):
        self.sd, self.cfg = sd, cfg

    def store(self, t):
        return t

    def conv_bn(self, conv, bn, x, stride=1, pad=0, dil=1, relu=True, res=None):
        sd = self.sd
        y = F.conv2d(x, sd[conv + ".weight"], None, stride, pad, dil)
        y = F.batch_norm(y, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"],
                         False, 0.0, self.cfg.eps)
        if res is not None:
            y = y + res
        return F.relu(y) if relu else y

    def classifier(self, conv, x):
        return F.conv2d(x, self.sd[conv + ".weight"], self.sd[conv + ".bias"])


class _Fp16Storage:
    """The engine's arithmetic with the sums in `dtype`; sd64: the state_dict in fp64."""

    def __init__(self, sd64, cfg, dtype):
        self.sd, self.cfg, self.dtype = sd64, cfg, dtype

    def store(self, t):
        return h16(t)

    def conv_bn(self, conv, bn, x, stride=1, pad=0, dil=1, relu=True, res=None):
        sd = self.sd
        scale = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + self.cfg.eps)
        shift = sd[bn + ".bias"] - sd[bn + ".running_mean"] * scale
        w = (sd[conv + ".weight"] * scale.view(-1, 1, 1, 1)).to(torch.float16).to(self.dtype)
        y = F.conv2d(x, w, None, stride, pad, dil) + shift.float().to(self.dtype).view(1, -1, 1, 1)
        if res is not None:
            y = y + res                     # added to the accumulator: one rounding for the sum
        return h16(F.relu(y) if relu else y)

    def classifier(self, conv, x):
        w = self.sd[conv + ".weight"].to(torch.float16).to(self.dtype)
        return F.conv2d(x, w, self.sd[conv + ".bias"].float().to(self.dtype))


def _backbone(R, sd, x, cfg):
    """{1..4: output of layer1..4} (oracle.model.backbone_forward with every layer tapped)."""
    strides, dils = omodel._OS[cfg.os]
    p = "backbone."
    x = R.conv_bn(p + "conv1.0", p + "conv1.1", x, 2, 1)
    x = R.conv_bn(p + "conv1.3", p + "conv1.4", x, 1, 1)
    x = R.conv_bn(p + "conv1.6", p + "bn1", x, 1, 1)
    x = F.max_pool2d(x, 3, 2, 1)
    feats = {}
    for li in range(1, 5):
        n = cfg.layers[li - 1] if li < 4 else len(cfg.mg_unit)
        for bi in range(n):
            d = dils[li - 1] if li < 4 else cfg.mg_unit[bi] * dils[3]
            s = strides[li - 1] if bi == 0 else 1
            b = p + f"layer{li}.{bi}"
            out = R.conv_bn(b + ".conv1", b + ".bn1", x)
            out = R.conv_bn(b + ".conv2", b + ".bn2", out, s, d, d)
            res = x
            if (b + ".downsample.0.weight") in sd:
                res = R.conv_bn(b + ".downsample.0", b + ".downsample.1", x, s, relu=False)
            x = R.conv_bn(b + ".conv3", b + ".bn3", out, res=res)
        feats[li] = x
    return feats


def _aspp(R, x, cfg):
    d = omodel._ASPP_D[cfg.os]
    xs = [R.conv_bn("aspp.aspp1.atrous_conv", "aspp.aspp1.bn", x)]
    for k in (2, 3, 4):
        xs.append(R.conv_bn(f"aspp.aspp{k}.atrous_conv", f"aspp.aspp{k}.bn", x, 1, d[k - 1], d[k - 1]))
    g = R.store(F.adaptive_avg_pool2d(x, 1))
    g = R.conv_bn("aspp.global_avg_pool.1", "aspp.global_avg_pool.2", g)
    g = F.interpolate(g, size=x.shape[2:], mode="bilinear", align_corners=cfg.align_corner)   # a broadcast: exact
    return R.conv_bn("aspp.conv1", "aspp.bn1", torch.cat(xs + [g], dim=1))


def _deeplabv3p(R, sd, x, cfg):
    feats = _backbone(R, sd, x, cfg)
    a = _aspp(R, feats[4], cfg)
    low = R.conv_bn("decoder.conv1", "decoder.bn1", feats[1])
    a = R.store(F.interpolate(a, size=low.shape[2:], mode="bilinear", align_corners=cfg.align_corner))
    y = R.conv_bn("decoder.last_conv.0", "decoder.last_conv.1", torch.cat((a, low), dim=1), 1, 1)
    y = R.conv_bn("decoder.last_conv.3", "decoder.last_conv.4", y, 1, 1)
    return R.classifier("decoder.last_conv.6", y)


def _psp(R, sd, x, cfg):
    f = _backbone(R, sd, x, cfg)[4]
    priors = []
    for k, s in enumerate(getattr(cfg, "pyramid_sizes", (1, 2, 3, 6))):
        g = R.store(F.adaptive_avg_pool2d(f, s))
        g = R.conv_bn(f"ppm.stages.{k}.1", f"ppm.stages.{k}.2", g)
        priors.append(R.store(F.interpolate(g, size=f.shape[2:], mode="bilinear", align_corners=cfg.align_corner)))
    y = R.conv_bn("ppm.bottleneck.0", "ppm.bottleneck.1", torch.cat(priors + [f], dim=1), 1, 1)
    return R.classifier("last_conv", y)


_HEADS = {"deeplabv3p": _deeplabv3p, "psp": _psp}


def _sd64(sd):
    return {k: v.detach().double() for k, v in sd.items() if v.is_floating_point()}


def eval_logits64(sd, x, cfg):
    """The fp64 eval-mode low-resolution logits of the main head (the truth)."""
    sd64 = _sd64(sd)
    with torch.no_grad():
        return _HEADS[cfg.model](_Exact(sd64, cfg), sd64, x.double(), cfg)


def fp16_storage_logits(sd, x, cfg, dtype):
    """Low-resolution logits (float64) of the fp16-storage emulation with the sums in `dtype`."""
    sd64 = _sd64(sd)
    with torch.no_grad():
        return _HEADS[cfg.model](_Fp16Storage(sd64, cfg, dtype), sd64, h16(x.to(dtype)), cfg).double()


def yardstick(sd, x, cfg):
    """(ref64, e, r): the fp64 logits, and the larger of the two emulations' max-abs / relative-L2 distances to them."""
    ref = eval_logits64(sd, x, cfg)
    e = r = 0.0
    for dt in (torch.float64, torch.float32):
        emu = fp16_storage_logits(sd, x, cfg, dt)
        e = max(e, float((emu - ref).abs().max()))
        r = max(r, float((emu - ref).norm() / ref.norm()))
    return ref, e, r
