"""The yardstick of tests/test_deploy_f8_*.py: an fp8-STORAGE emulation of the eval-mode forward, on the CPU, that never
touches dcfp_amd.deploy.  Like tests/_deploy_ref.py it runs oracle.model.seg_forward with `_conv` / `_bn` /
adaptive_avg_pool2d patched (the oracle files are untouched), and it quantises where the fp8 plan does, with the
scales the plan derives from the same `amax` dict ({record name: absolute maximum of that record's output}):

  * the conv that reads the image is fp16 storage (image, folded weights and output rounded to fp16); its output is
    then quantised with s = amax / 448;
  * every later conv: folded fp64 weights quantised per output channel (s_w = max|w[co]| / 448), output = conv + shift
    (+ ReLU) quantised with the output buffer's scale; the bn3 output is NOT quantised (the engine adds the residual to
    the fp32 accumulator), the block output relu(out + res) is - with conv3's scale - on entry to the convs and the
    pool that read it (quantising with one scale is idempotent);
  * the ASPP concat has ONE scale: the largest amax of its five writers;
  * the image-pool branch is fp16: mean of the quantised map rounded to fp16, fp16 weights, fp16 output, quantised with
    the concat's scale where it is broadcast;
  * the classifier: quantised weights, fp32 bias, output not rounded.

Every quantisation is clamp to [-448, 448] in fp32, then round to nearest even to e4m3fn.  The convolution itself runs
in `dtype` (fp64: exact sums of the quantised values; fp32: one more summation order).  A plain helper module: no
fixtures, no tests."""
import os
import sys
from unittest import mock

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _deploy_ref as dref  # noqa: E402
from _deploy_ref import h16, omodel  # noqa: E402

F8 = torch.float8_e4m3fn
FIRST, STEM_LAST = "backbone.conv1.0", "backbone.conv1.6"
GAP, GAP_UP = "aspp.global_avg_pool.1", "aspp.global_avg_pool.up"
CAT = tuple(f"aspp.aspp{k}.atrous_conv" for k in (1, 2, 3, 4)) + (GAP_UP,)


def to_f8(t):
    return t.float().clamp(-448.0, 448.0).to(F8)


def q8(t, s):
    """Quantise with scale s: the real values an fp8 buffer of that scale holds."""
    return to_f8(t / s).to(t.dtype) * s


def _reads_block_output(name, cfg):
    """Convs whose input is a tensor neither patch saw being made: the stem's pooled output or a block's relu(out + res)."""
    return ((".layer" in name and name.endswith(".conv1")) or name.startswith("aspp.aspp")
            or (name == "last_conv.0" and cfg.model != "deeplabv3"))


def record_amax(sd, x, cfg):
    """{record name: max|output|} of the fp64 eval-mode forward, under the engine's record names (a conv's record holds
    its BatchNorm, ReLU and residual sum): the CPU stand-in for deploy.calibrate."""
    sd64 = {k: v.detach().double() if v.is_floating_point() else v.detach().clone() for k, v in sd.items()}
    amax, st = {}, {"last": None, "pending": None}
    real_conv, real_bn, real_pool = omodel._conv, omodel._bn, F.adaptive_avg_pool2d

    def settle(x):
        if st["pending"] is not None:
            amax[st["pending"]] = float(x.abs().max())
            st["pending"] = None

    def conv(sd_, name, x, stride=1, pad=0, dil=1):
        if _reads_block_output(name, cfg):
            settle(x)
        y = real_conv(sd_, name, x, stride, pad, dil)
        st["last"] = name
        if (name + ".bias") in sd_:
            amax[name] = float(y.abs().max())
        return y

    def bn(sd_, name, x, cfg_, training, relu):
        y = real_bn(sd_, name, x, cfg_, training, relu)
        if name.endswith(".bn3"):
            st["pending"] = st["last"]
        else:
            amax[st["last"]] = float(y.abs().max())
            if st["last"] == GAP:
                amax[GAP_UP] = amax[GAP]
        return y

    def pool(x, size):
        settle(x)
        return real_pool(x, size)

    with torch.no_grad(), mock.patch.object(omodel, "_conv", conv), mock.patch.object(omodel, "_bn", bn), \
            mock.patch.object(omodel.F, "adaptive_avg_pool2d", pool):
        omodel.seg_forward(sd64, x.double(), cfg, training=False)
    return amax


def scales_of(amax):
    """{record name: scale of the buffer it writes}: amax / 448 (1 for 0); the ASPP concat's writers share one."""
    s = {k: (float(v) / 448.0 if float(v) > 0 else 1.0) for k, v in amax.items()}
    if any(k in s for k in CAT):
        top = max(float(amax[k]) for k in CAT)
        for k in CAT:
            s[k] = top / 448.0 if top > 0 else 1.0
    return s


class _Pending:
    """A bias-free conv waiting for the BatchNorm that follows it."""

    def __init__(self, name, x, stride, pad, dil):
        self.name, self.x, self.stride, self.pad, self.dil = name, x, stride, pad, dil


def quantise_weight(wf):
    """Folded fp64 weights -> the real values of their per-output-channel e4m3 quantisation (fp64)."""
    a = wf.abs().amax(dim=(1, 2, 3))
    s_w = torch.where(a > 0, a / 448.0, torch.ones_like(a)).view(-1, 1, 1, 1)
    return to_f8(wf / s_w).double() * s_w


def fp8_storage_logits(sd, x, cfg, amax, dtype):
    """Low-resolution logits (float64) of the fp8-storage emulation with the convolutions summed in `dtype`."""
    sd64 = {k: v.detach().double() for k, v in sd.items() if v.is_floating_point()}
    s = scales_of(amax)
    st = {"block": s[STEM_LAST], "pending": None}

    def block_scale():
        if st["pending"] is not None:
            st["block"], st["pending"] = st["pending"], None
        return st["block"]

    def conv(sd_, name, x, stride=1, pad=0, dil=1):
        if name == FIRST:
            return _Pending(name, h16(x), stride, pad, dil)
        if name == GAP:
            return _Pending(name, x, stride, pad, dil)          # (the pool patch rounded it to fp16)
        if _reads_block_output(name, cfg):
            x = q8(x, block_scale())
        elif name.endswith(".downsample.0"):
            x = q8(x, st["block"])                              # the block's input: conv1 of this block settled it
        if (name + ".bias") in sd64:                            # the classifier: output not rounded
            w = quantise_weight(sd64[name + ".weight"]).to(dtype)
            return F.conv2d(x, w, sd64[name + ".bias"].float().to(dtype), stride, pad, dil)
        return _Pending(name, x, stride, pad, dil)

    def bn(sd_, name, p, cfg_, training, relu):
        assert isinstance(p, _Pending) and not training
        scale = sd64[name + ".weight"] / torch.sqrt(sd64[name + ".running_var"] + cfg_.eps)
        shift = sd64[name + ".bias"] - sd64[name + ".running_mean"] * scale
        wf = sd64[p.name + ".weight"] * scale.view(-1, 1, 1, 1)
        fp16 = p.name in (FIRST, GAP)
        w = (wf.to(torch.float16) if fp16 else quantise_weight(wf)).to(dtype)
        y = F.conv2d(p.x, w, None, p.stride, p.pad, p.dil) + shift.float().to(dtype).view(1, -1, 1, 1)
        if relu:
            y = F.relu(y)
        if fp16:
            return q8(h16(y), s[GAP_UP if p.name == GAP else FIRST])
        if name.endswith(".bn3"):
            st["pending"] = s[p.name]
            return y
        return q8(y, s[p.name])

    real_pool = F.adaptive_avg_pool2d

    def pool(x, size):
        return h16(real_pool(q8(x, block_scale()), size))

    with torch.no_grad(), mock.patch.object(omodel, "_conv", conv), mock.patch.object(omodel, "_bn", bn), \
            mock.patch.object(omodel.F, "adaptive_avg_pool2d", pool):
        low = omodel.seg_forward({k: v for k, v in sd.items()}, x.to(dtype), cfg, training=False)[2][0]
    return low.double()


def distances(sd, x, cfg, amax):
    """(ref64, [(max-abs, relative L2, label disagreement) of the fp64-sum and of the fp32-sum emulation])."""
    ref = dref.eval_logits64(sd, x, cfg)
    out = []
    for dt in (torch.float64, torch.float32):
        emu = fp8_storage_logits(sd, x, cfg, amax, dt)
        out.append((float((emu - ref).abs().max()), float((emu - ref).norm() / ref.norm()),
                    float((emu.argmax(1) != ref.argmax(1)).double().mean())))
    return ref, out


def yardstick(sd, x, cfg, amax):
    """(ref64, e, r): the fp64 logits, and the larger of the two emulations' max-abs / relative-L2 distances to them."""
    ref, d = distances(sd, x, cfg, amax)
    return ref, max(v[0] for v in d), max(v[1] for v in d)
