"""The yardstick of tests/test_deploy_gpu.py: an fp16-STORAGE emulation of the eval-mode forward, on the CPU, that never
touches dcfp_amd.deploy.  It runs oracle.model.seg_forward with its `_conv` / `_bn` patched (the oracle files are
untouched): the BatchNorm is folded into the conv in fp64 and the folded weights rounded to fp16 once; every tensor
the engine stores is rounded to fp16 - after each conv + shift (+ ReLU), the downsample branch, after the residual
add + ReLU, the pooled vector - while the convolution itself runs in `dtype` (fp64: exact sums of the rounded values;
fp32: one more summation order).  A plain helper module like tests/_parity.py: no fixtures, no tests.

How the rounding points are placed with two patches only: a tensor that is stored is either rounded where `_bn`
returns it, or - the residual sum F.relu(out + res), which neither patch sees - on entry to every `_conv` that reads
it (rounding is idempotent, so rounding every conv input is the same as rounding every stored tensor once).  The bn3
output is NOT rounded: the engine adds the residual to the fp32 accumulator and rounds the sum.  The global average
pool reads the stored (rounded) tensor, so F.adaptive_avg_pool2d is patched to round its input."""
import os
import sys
from unittest import mock

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import model as omodel  # noqa: E402


def h16(t):
    """Round to fp16 and back (the engine's storage format)."""
    return t.to(torch.float16).to(t.dtype)


class _Pending:
    """A bias-free conv waiting for the BatchNorm that follows it."""

    def __init__(self, name, x, stride, pad, dil):
        self.name, self.x, self.stride, self.pad, self.dil = name, x, stride, pad, dil


def eval_logits64(sd, x, cfg):
    """The fp64 eval-mode low-resolution logits of the main head (the truth)."""
    sd64 = {k: v.detach().double() if v.is_floating_point() else v.detach().clone() for k, v in sd.items()}
    with torch.no_grad():
        return omodel.seg_forward(sd64, x.double(), cfg, training=False)[2][0]


def fp16_storage_logits(sd, x, cfg, dtype):
    """Low-resolution logits (float64) of the fp16-storage emulation with the convolutions summed in `dtype`."""
    sd64 = {k: v.detach().double() for k, v in sd.items() if v.is_floating_point()}

    def conv(sd_, name, x, stride=1, pad=0, dil=1):
        x = h16(x)
        if (name + ".bias") in sd64:          # the classifier: fp16 weights, fp32/fp64 bias, output not rounded
            w = sd64[name + ".weight"].to(torch.float16).to(dtype)
            return F.conv2d(x, w, sd64[name + ".bias"].to(dtype), stride, pad, dil)
        return _Pending(name, x, stride, pad, dil)

    def bn(sd_, name, p, cfg_, training, relu):
        assert isinstance(p, _Pending) and not training
        scale = sd64[name + ".weight"] / torch.sqrt(sd64[name + ".running_var"] + cfg_.eps)
        shift = sd64[name + ".bias"] - sd64[name + ".running_mean"] * scale
        w = (sd64[p.name + ".weight"] * scale.view(-1, 1, 1, 1)).to(torch.float16).to(dtype)
        y = F.conv2d(p.x, w, None, p.stride, p.pad, p.dil) + shift.float().to(dtype).view(1, -1, 1, 1)
        if relu:
            y = F.relu(y)
        return y if name.endswith(".bn3") else h16(y)

    real_pool = F.adaptive_avg_pool2d

    def pool(x, size):
        return real_pool(h16(x), size)

    with torch.no_grad(), mock.patch.object(omodel, "_conv", conv), mock.patch.object(omodel, "_bn", bn), \
            mock.patch.object(omodel.F, "adaptive_avg_pool2d", pool):
        low = omodel.seg_forward({k: v for k, v in sd.items()}, x.to(dtype), cfg, training=False)[2][0]
    return low.double()


def yardstick(sd, x, cfg):
    """(ref64, e, r): the fp64 logits, and the larger of the two emulations' max-abs / relative-L2 distances to them."""
    ref = eval_logits64(sd, x, cfg)
    e = r = 0.0
    for dt in (torch.float64, torch.float32):
        emu = fp16_storage_logits(sd, x, cfg, dt)
        e = max(e, float((emu - ref).abs().max()))
        r = max(r, float((emu - ref).norm() / ref.norm()))
    return ref, e, r
