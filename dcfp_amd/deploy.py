"""Half-precision deployment engine — the fourth stage of the reference's pipeline (totrt.py / scripts/cs/trt.sh:
freeze the fine-tuned, pruned network into an FP16 engine, save it, time it, evaluate through it).

`build_engine(model)` walks an eval-mode Seg_Model of any of the four heads - `simple`, `deeplabv3`, `deeplabv3p`, `psp`,
full width or slimmed by pruners.init_pruned_model - once and returns an `Engine`: a flat plan of layer records over
numbered activation buffers plus the packed tensors.  (`freeze(model)` is the older entry point for `deeplabv3` and
`simple` and gives the same engine for them.)  Planning and packing are plain torch on the CPU; running the plan needs
the device and goes through the kernels of csrc/conv_f16.hip and csrc/heads_f16.hip only:

  * activations NHWC fp16, channels padded to a multiple of 8 (the padding holds exact zeros);
  * weights [Cout8][kh][kw][Cin8] fp16 with the eval-mode BatchNorm scale folded in (in fp64, one rounding), the
    BatchNorm shift (and a conv bias) as an fp32 vector added in the conv's epilogue, with the residual add and ReLU;
  * the ASPP branches write their channel slice of the concat buffer (no cat), the image-pool branch is a global
    average pool, a 1x1 conv on N pixels and a broadcast; the classifier writes fp32 NCHW logits;
  * DeepLabv3+: the decoder concat [ASPP output resized, conv1(layer1)] is one buffer - a `resize` node and
    decoder.conv1 write its two slices; the layer1 output stays alive until then;
  * PSPNet: the concat [stage 0 .. 3, feats] is one buffer - the last bottleneck's conv3 writes the feats slice
    directly, one `pyramid` node pools all levels from that slice in one sweep, a 1x1 conv per level runs on the s x s
    map and a `resize` node writes each prior into its slice.

`build_engine(model, precision="fp8", amax=calibrate(fp16 engine, batches))` builds the calibrated 8-bit engine for
`simple` and `deeplabv3` (opt-in; DESIGN.md §11a, kernels in csrc/conv_f8.hip): activations NHWC e4m3 with channels
padded to 16 and ONE scale per buffer (the calibrated absolute maximum of the records writing it / 448), weights
[Cout8][kh][kw][Cin16] e4m3 quantised per output channel, the epilogue acc * mul[co] + add[co] (+ res_mul * residual).
The conv that reads the image and the image-pool branch stay fp16; a `cast` node quantises the former's output.  Such an
engine is saved as format 2; format-1 (fp16) engines load and run as before.  `Engine.trace(image)` returns what every
record wrote - the calibration and the per-record tests are built on it.

An Engine offers what evaluate.predict_whole / predict_sliding / predict_multiscale / predict_labels ask of a net:
engine(image) -> [logits], engine.lowres_logits(image) -> [lowres], engine.align_corner.

`save_flat(engine, path, mean, std)` writes an engine of either format as a flat engine file: what the
library's C runtime (dcfp_engine_* of include/dcfp_hip.h, tools/engine_run.cpp) loads and runs without Python.
`CEngine(path, device)` is that runtime behind the interface of an Engine - same kernels, same arguments, same bits -
and `CEngine.run_u8` takes uint8 HWC frames, normalised on the device through `input_table(mean, std)`.
"""
import ctypes as C
import os

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import check

FORMAT = 1                                          # fp16 engines
FORMAT_F8 = 2                                       # fp8 engines (meta["dtype"] == "float8_e4m3fn")
F8 = torch.float8_e4m3fn
F8_MAX = 448.0
_POOL_OPS = ("maxpool", "avgpool", "broadcast")
_GRAN = {"f16": 8, "f8": 16}                        # channel granule of a buffer: one 16-byte chunk
_ESIZE = {"f16": 2, "f8": 1}
PYRAMID_MAX_LEVELS, PYRAMID_MAX_SIZE = 4, 8         # what dcfp_pyramid_pool_nhwc_f16 takes


def _r8(c):
    return (int(c) + 7) // 8 * 8


def _rg(c, g):
    return (int(c) + g - 1) // g * g


def to_f8(t):
    """The engine's one conversion rule: clamp to [-448, 448] in fp32, then round to nearest even (e4m3fn keeps its
    subnormals; without the clamp torch turns 465 into NaN)."""
    return t.float().clamp(-F8_MAX, F8_MAX).to(F8)


def _f32(v):
    """A Python float formed in fp64, rounded once to fp32 (what a kernel's float argument holds)."""
    return float(torch.tensor(float(v), dtype=torch.float64).float())


def fold_bn(conv, bn):
    """(scale, shift) in fp64 of eval-mode `bn` after `conv` (bn None: the conv's own bias, scale 1)."""
    cout = conv.weight.shape[0]
    bias = conv.bias.detach().double().cpu() if conv.bias is not None else torch.zeros(cout, dtype=torch.float64)
    if bn is None:
        return torch.ones(cout, dtype=torch.float64), bias
    scale = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.detach().double().cpu() + bn.eps)
    shift = bn.bias.detach().double().cpu() + (bias - bn.running_mean.detach().double().cpu()) * scale
    return scale, shift


def pack_weight(w, scale, segments, cin8):
    """[Cout, Cin, k, k] * scale[co] (fp64) -> fp16 [Cout8, k, k, cin8]; input channel block (offset, count) of
    `segments` (in the conv's channel order) lands at columns offset .. offset + count - 1, everything else is zero."""
    cout, cin, kh, kw = w.shape
    ws = (w.detach().double().cpu() * scale.view(-1, 1, 1, 1)).to(torch.float16)
    out = torch.zeros((_r8(cout), kh, kw, cin8), dtype=torch.float16)
    s = 0
    for off, cnt in segments:
        out[:cout, :, :, off:off + cnt] = ws[:, s:s + cnt].permute(0, 2, 3, 1)
        s += cnt
    assert s == cin, (s, cin)
    return out.contiguous()


def unpack_weight(packed, cout, segments):
    """The inverse of pack_weight / pack_weight_f8: [cout, Cin, k, k] in the packed dtype."""
    parts = [packed[:cout, :, :, off:off + cnt] for off, cnt in segments]
    return torch.cat(parts, dim=3).permute(0, 3, 1, 2).contiguous()


def pack_weight_f8(wf, segments, cin16):
    """Folded fp64 weights [Cout, Cin, k, k] -> (e4m3 [Cout8, k, k, cin16], s_w fp64 [Cout]): quantised per output
    channel, q = fp8(clamp(w / s_w[co])) with s_w[co] = max|w[co]| / 448 (1 for an all-zero filter); channel placement
    and zero padding as pack_weight."""
    cout, cin, kh, kw = wf.shape
    amax = wf.abs().amax(dim=(1, 2, 3))
    s_w = torch.where(amax > 0, amax / F8_MAX, torch.ones_like(amax))
    q = to_f8(wf / s_w.view(-1, 1, 1, 1))
    out = torch.zeros((_r8(cout), kh, kw, cin16), dtype=torch.uint8).view(F8)
    s = 0
    for off, cnt in segments:
        out[:cout, :, :, off:off + cnt] = q[:, s:s + cnt].permute(0, 2, 3, 1)
        s += cnt
    assert s == cin, (s, cin)
    return out.contiguous(), s_w


class _Planner:
    """fp8 = False: every buffer and record is fp16.  fp8 = True: a new buffer is fp8 (granule 16) unless asked
    otherwise, a conv takes the format of the buffer it reads, and the fp8 records keep their folded fp64 weights until
    finalize_f8 knows every buffer's scale."""

    def __init__(self, fp8=False):
        self.records, self.tensors, self.pitch, self.segments, self.fmt = [], [], [], [], []
        self.fp8 = bool(fp8)
        self.gran = _GRAN["f8" if fp8 else "f16"]    # of the buffers the plan makes by default (concat slices)
        self.scales = None

    def buffer(self, segments, pitch=None, fmt=None):
        fmt = fmt or ("f8" if self.fp8 else "f16")
        self.pitch.append(pitch if pitch is not None else _rg(sum(c for _, c in segments), _GRAN[fmt]))
        self.segments.append(list(segments))
        self.fmt.append(fmt)
        return len(self.pitch) - 1

    def tensor(self, t):
        self.tensors.append(t)
        return len(self.tensors) - 1

    def conv(self, name, conv, bn, src, relu, dst=None, y_off=0, res=-1, f32=False):
        if not isinstance(conv, nn.Conv2d) or (bn is not None and not isinstance(bn, nn.BatchNorm2d)):
            raise NotImplementedError(f"freeze: {name}: {type(conv).__name__} / {type(bn).__name__} is not conv + BatchNorm2d")
        k, s, p, d = conv.kernel_size, conv.stride, conv.padding, conv.dilation
        if (k[0] != k[1] or k[0] not in (1, 3) or s[0] != s[1] or s[0] not in (1, 2) or p[0] != p[1] or d[0] != d[1]
                or conv.groups != 1 or conv.padding_mode != "zeros" or isinstance(p, str)):
            raise NotImplementedError(f"freeze: {name}: unsupported conv geometry {conv}")
        cout, cin = conv.weight.shape[:2]
        if cin != sum(c for _, c in self.segments[src]):
            raise ValueError(f"freeze: {name} reads {cin} channels, its input holds {self.segments[src]}")
        scale, shift = fold_bn(conv, bn)
        fmt = self.fmt[src]
        if dst is None:
            dst = -1 if f32 else self.buffer([(0, cout)], fmt=fmt)
        if fmt == "f8":
            rec = {"op": "conv", "fmt": "f8", "name": name, "src": src, "dst": dst, "res": res, "cin": int(cin),
                   "cout": int(cout), "cin8": self.pitch[src], "k": k[0], "stride": s[0], "pad": p[0], "dil": d[0],
                   "relu": bool(relu), "y_off": int(y_off), "f32": bool(f32),
                   "segments": [list(sg) for sg in self.segments[src]],
                   "_w64": conv.weight.detach().double().cpu() * scale.view(-1, 1, 1, 1), "_shift64": shift}
            if (dst >= 0 and self.fmt[dst] != "f8") or (res >= 0 and self.fmt[res] != "f8"):
                raise ValueError(f"freeze: {name}: an fp8 conv writes and adds fp8 buffers only")
        else:
            rec = self._conv_f16(name, src, dst, res, cin, cout, k, s, p, d, relu, y_off, f32, conv, scale, shift)
        if res >= 0 and [tuple(sg) for sg in self.segments[res]] != [(0, int(cout))]:
            # (the residual keeps its own pitch - the kernel takes res_pitch - but holds the conv's channels from 0)
            raise ValueError(f"freeze: {name}: residual holds {self.segments[res]}, the conv writes {cout} channels")
        self.records.append(rec)
        return dst

    def _conv_f16(self, name, src, dst, res, cin, cout, k, s, p, d, relu, y_off, f32, conv, scale, shift):
        sh = torch.zeros(_r8(cout), dtype=torch.float32)
        sh[:cout] = shift.float()
        rec = {"op": "conv", "name": name, "src": src, "dst": dst, "res": res, "cin": int(cin), "cout": int(cout),
               "cin8": self.pitch[src], "k": k[0], "stride": s[0], "pad": p[0], "dil": d[0], "relu": bool(relu),
               "y_off": int(y_off), "f32": bool(f32), "segments": [list(sg) for sg in self.segments[src]],
               "w": self.tensor(pack_weight(conv.weight, scale, self.segments[src], self.pitch[src])),
               "shift": self.tensor(sh)}
        if self.fp8:
            rec["fmt"] = "f16"
        return rec

    def finalize_f8(self, amax):
        """Buffer scales from the calibration maxima, then the fp8 records' packed tensors."""
        def need(name):
            if name not in amax:
                raise KeyError(f"build_engine: amax has no entry for the record {name!r}")
            return float(amax[name])
        top = {}
        for r in self.records:                       # the largest calibrated |output| over the records writing a buffer
            b = r["dst"]
            if b >= 0 and self.fmt[b] == "f8" and r["op"] != "maxpool":   # (a cast writes what its source record wrote)
                top[b] = max(top.get(b, 0.0), need(r["amax_of"] if r["op"] == "cast" else r["name"]))
        scales = [1.0] * len(self.pitch)
        for b, v in top.items():
            scales[b] = v / F8_MAX if v > 0 else 1.0
        for r in self.records:                       # (in plan order: the pool's input is scaled by then)
            if r["op"] == "maxpool" and self.fmt[r["dst"]] == "f8":
                scales[r["dst"]] = scales[r["src"]]
        for r in self.records:
            s_x = scales[r["src"]]
            if r["op"] == "cast" or (r["op"] == "broadcast" and r.get("fmt") == "f8"):
                r["scale"] = _f32(1.0 / scales[r["dst"]])
            elif r["op"] == "avgpool" and r.get("fmt") == "f8":
                r["scale"] = _f32(s_x)
            elif r["op"] == "conv" and r["fmt"] == "f8":
                s_y = 1.0 if r["f32"] else scales[r["dst"]]
                wf, shift = r.pop("_w64"), r.pop("_shift64")
                cout = r["cout"]
                packed, s_w = pack_weight_f8(wf, r["segments"], r["cin8"])
                mul, add = torch.zeros(_r8(cout), dtype=torch.float32), torch.zeros(_r8(cout), dtype=torch.float32)
                mul[:cout] = (s_w * s_x / s_y).float()
                add[:cout] = (shift / s_y).float()
                r["w"], r["mul"], r["add"] = self.tensor(packed), self.tensor(mul), self.tensor(add)
                r["res_mul"] = _f32(scales[r["res"]] / s_y) if r["res"] >= 0 else 0.0
        self.scales = scales

    def node(self, op, name, src, dst, y_off=0, **extra):
        self.records.append({"op": op, "name": name, "src": src, "dst": dst, "y_off": int(y_off), **extra})
        return dst


def _plan_sequential(pl, prefix, mods, x, tail_bn=None):
    """conv (-> BatchNorm2d) (-> ReLU) groups of an nn.Sequential's children; tail_bn: the BatchNorm (+ ReLU) that the
    model applies to the last conv from outside the container (the deep stem's bn1 / relu1)."""
    i = 0
    while i < len(mods):
        conv = mods[i]
        name = f"{prefix}.{i}"
        if not isinstance(conv, nn.Conv2d):
            raise NotImplementedError(f"freeze: {name}: {type(conv).__name__} in a conv stack")
        i += 1
        bn, relu = None, False
        if i < len(mods) and isinstance(mods[i], nn.BatchNorm2d):
            bn = mods[i]; i += 1
        if i < len(mods) and isinstance(mods[i], nn.ReLU):
            relu = True; i += 1
        last = i >= len(mods)
        if last and tail_bn is not None:
            bn, relu = tail_bn, True
        x = pl.conv(name, conv, bn, x, relu, f32=(last and bn is None))
        if pl.fp8 and x >= 0 and pl.fmt[x] == "f16":   # the conv that reads the image stays fp16; quantise its output
            x = pl.node("cast", name + ".cast", x, pl.buffer(pl.segments[x]), amax_of=name, fmt="f8",
                        c=sum(c for _, c in pl.segments[x]))
    return x


def _plan_backbone(pl, bb, x, tail=None):
    """{1..4: the output buffer of layer1..4}.  tail = (buffer, offset): the last block's conv3 writes that channel
    slice of a buffer the caller made (PSPNet's concat) instead of a buffer of its own."""
    from .networks.backbone.resnet import Bottleneck, ResNet
    if not isinstance(bb, ResNet):
        raise NotImplementedError(f"freeze: backbone {type(bb).__module__}.{type(bb).__name__} is not the ResNet")
    x = _plan_sequential(pl, "backbone.conv1", list(bb.conv1.children()), x, tail_bn=bb.bn1)
    mp = bb.maxpool
    if not isinstance(mp, nn.MaxPool2d) or (mp.kernel_size, mp.stride, mp.padding) != (3, 2, 1):
        raise NotImplementedError(f"freeze: backbone.maxpool {mp}")
    x = pl.node("maxpool", "backbone.maxpool", x, pl.buffer(pl.segments[x]), **({"fmt": "f8"} if pl.fp8 else {}))
    feats = {}
    for li in range(1, 5):
        layer = getattr(bb, f"layer{li}")
        for bi, blk in enumerate(layer):
            p = f"backbone.layer{li}.{bi}"
            if not isinstance(blk, Bottleneck):
                raise NotImplementedError(f"freeze: {p}: {type(blk).__name__}")
            out = pl.conv(p + ".conv1", blk.conv1, blk.bn1, x, True)
            out = pl.conv(p + ".conv2", blk.conv2, blk.bn2, out, True)
            res = x
            if blk.downsample is not None:
                ds = list(blk.downsample.children())
                if len(ds) != 2:
                    raise NotImplementedError(f"freeze: {p}.downsample {blk.downsample}")
                res = pl.conv(p + ".downsample.0", ds[0], ds[1], x, False)
            if tail is not None and li == 4 and bi == len(layer) - 1:
                x = pl.conv(p + ".conv3", blk.conv3, blk.bn3, out, True, res=res, dst=tail[0], y_off=tail[1])
            else:
                x = pl.conv(p + ".conv3", blk.conv3, blk.bn3, out, True, res=res)
        feats[li] = x
    return feats


def _plan_aspp(pl, aspp, x):
    from .networks.tools.aspp import ASPP
    if not isinstance(aspp, ASPP) or aspp.outplanes is None:
        raise NotImplementedError(f"freeze: aspp {type(aspp).__name__} (outplanes {getattr(aspp, 'outplanes', None)})")
    pool = list(aspp.global_avg_pool.children())
    if len(pool) != 4 or not isinstance(pool[0], nn.AdaptiveAvgPool2d) or pool[0].output_size not in (1, (1, 1)):
        raise NotImplementedError(f"freeze: aspp.global_avg_pool {aspp.global_avg_pool}")
    branches = [aspp.aspp1, aspp.aspp2, aspp.aspp3, aspp.aspp4]
    widths = [m.atrous_conv.weight.shape[0] for m in branches] + [pool[1].weight.shape[0]]
    offs, o = [], 0
    for c in widths:      # every slice starts at a multiple of the granule; the gaps hold the branches' zero padding
        offs.append(o); o += _rg(c, pl.gran)
    cat = pl.buffer(list(zip(offs, widths)), pitch=o)
    for i, m in enumerate(branches):
        pl.conv(f"aspp.aspp{i + 1}.atrous_conv", m.atrous_conv, m.bn, x, True, dst=cat, y_off=offs[i])
    if pl.fp8:            # the image-pool branch stays fp16: N pixels, and its input is a mean, not a quantised map
        g = pl.node("avgpool", "aspp.global_avg_pool.0", x, pl.buffer(pl.segments[x], pitch=pl.pitch[x], fmt="f16"),
                    fmt="f8")
        g = pl.conv("aspp.global_avg_pool.1", pool[1], pool[2], g, isinstance(pool[3], nn.ReLU))
        pl.node("broadcast", "aspp.global_avg_pool.up", g, cat, y_off=offs[4], fmt="f8", c=widths[4])
    else:
        g = pl.node("avgpool", "aspp.global_avg_pool.0", x, pl.buffer(pl.segments[x]))
        g = pl.conv("aspp.global_avg_pool.1", pool[1], pool[2], g, isinstance(pool[3], nn.ReLU))
        pl.node("broadcast", "aspp.global_avg_pool.up", g, cat, y_off=offs[4])
    return pl.conv("aspp.conv1", aspp.conv1, aspp.bn1, cat, True)


def _slices(widths):
    """(offsets, pitch) of a concat buffer: every slice starts at a multiple of 8; the gaps hold the zero padding."""
    offs, o = [], 0
    for c in widths:
        offs.append(o); o += _r8(c)
    return offs, o


def _is_plain_1x1(conv):
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.bias is None
            and conv.padding == (0, 0) and conv.groups == 1)


def _plan_psp(pl, model, x):
    """Backbone -> pyramid, with no cat and no copy of the features (networks/tools/ppm.py)."""
    from .networks.tools.ppm import PPMModule
    ppm = model.ppm
    if not isinstance(ppm, PPMModule):
        raise NotImplementedError(f"freeze: ppm {type(ppm).__name__} is not the PPMModule")
    if not 1 <= len(ppm.stages) <= PYRAMID_MAX_LEVELS:
        raise NotImplementedError(f"freeze: ppm.stages has {len(ppm.stages)} stages (1 .. {PYRAMID_MAX_LEVELS} are supported)")
    sizes = []
    for k, st in enumerate(ppm.stages):
        mods = list(st.children()) if isinstance(st, nn.Sequential) else []
        if len(mods) != 4 or not isinstance(mods[0], nn.AdaptiveAvgPool2d) or not isinstance(mods[2], nn.BatchNorm2d) \
                or not isinstance(mods[3], nn.ReLU):
            raise NotImplementedError(f"freeze: ppm.stages.{k} {st} is not pool, conv, BatchNorm2d, ReLU")
        size = mods[0].output_size
        size = (size, size) if isinstance(size, int) else tuple(size)
        if len(size) != 2 or size[0] != size[1] or not isinstance(size[0], int) or not 1 <= size[0] <= PYRAMID_MAX_SIZE:
            raise NotImplementedError(f"freeze: ppm.stages.{k}.0 pools to {mods[0].output_size} "
                                      f"(square sizes 1 .. {PYRAMID_MAX_SIZE} are supported)")
        if not _is_plain_1x1(mods[1]):
            raise NotImplementedError(f"freeze: ppm.stages.{k}.1 {mods[1]} is not a bias-free 1x1 conv")
        sizes.append(int(size[0]))
    c_feats = int(ppm.stages[0][1].weight.shape[1])
    widths = [int(st[1].weight.shape[0]) for st in ppm.stages] + [c_feats]
    offs, pitch = _slices(widths)
    cat = pl.buffer(list(zip(offs, widths)), pitch=pitch)          # [stage 0 .. stage 3, feats] (ppm.py:37)
    _plan_backbone(pl, model.backbone, x, tail=(cat, offs[-1]))
    pooled = [pl.buffer([(0, c_feats)]) for _ in sizes]
    pl.node("pyramid", "ppm.stages.pool", cat, pooled[0], dsts=pooled, x_off=offs[-1], c8=_r8(c_feats), sizes=sizes)
    for k, st in enumerate(ppm.stages):
        g = pl.conv(f"ppm.stages.{k}.1", st[1], st[2], pooled[k], True)
        pl.node("resize", f"ppm.stages.{k}.up", g, cat, y_off=offs[k], align=bool(ppm.align_corners))
    x = _plan_sequential(pl, "ppm.bottleneck", list(ppm.bottleneck.children()), cat)
    if x == -1 or not isinstance(model.last_conv, nn.Conv2d) or model.last_conv.bias is None:
        raise NotImplementedError(f"freeze: last_conv {model.last_conv} is not a classifier conv with a bias")
    return pl.conv("last_conv", model.last_conv, None, x, False, f32=True)


def _plan_deeplabv3p(pl, model, x):
    """Backbone (layer1 tapped) -> ASPP -> decoder, the decoder concat written in slices (deeplabv3p.py:31-38)."""
    from .networks.deeplabv3p import Decoder
    dec = model.decoder
    if not isinstance(dec, Decoder):
        raise NotImplementedError(f"freeze: decoder {type(dec).__name__} is not the Decoder")
    if not _is_plain_1x1(dec.conv1):
        raise NotImplementedError(f"freeze: decoder.conv1 {dec.conv1} is not a bias-free 1x1 conv")
    for name, _ in dec.named_children():
        if name not in ("conv1", "bn1", "relu", "last_conv"):
            raise NotImplementedError(f"freeze: module decoder.{name}")
    feats = _plan_backbone(pl, model.backbone, x)
    a = _plan_aspp(pl, model.aspp, feats[4])
    widths = [sum(c for _, c in pl.segments[a]), int(dec.conv1.weight.shape[0])]
    offs, pitch = _slices(widths)
    cat = pl.buffer(list(zip(offs, widths)), pitch=pitch)          # [ASPP output resized, conv1(layer1)]
    pl.conv("decoder.conv1", dec.conv1, dec.bn1, feats[1], True, dst=cat, y_off=offs[1])
    pl.node("resize", "decoder.up", a, cat, y_off=offs[0], align=bool(dec.align_corner))
    return _plan_sequential(pl, "decoder.last_conv", list(dec.last_conv.children()), cat)


def _freeze(model, dtype, heads, precision="fp16", amax=None):
    from . import networks
    if dtype != torch.float16:
        raise NotImplementedError(f"freeze: dtype {dtype}: the engine is fp16 only (fp8: build_engine(precision='fp8'))")
    if precision not in ("fp16", "fp8"):
        raise ValueError(f"build_engine: precision {precision!r} (fp16 and fp8 are built)")
    fp8 = precision == "fp8"
    if fp8 and amax is None:
        raise ValueError("build_engine: precision='fp8' needs amax, the {record name: absolute maximum} dict of "
                         "deploy.calibrate on an fp16 engine of the same model")
    kinds = {getattr(networks, h).Seg_Model: h for h in heads}
    if type(model) not in kinds:
        raise NotImplementedError(f"freeze: {type(model).__module__}.{type(model).__name__} is not supported "
                                  f"({' and '.join('networks.' + h for h in heads)} are" +
                                  ("; deploy.build_engine freezes every head)" if len(heads) == 2 else ")"))
    kind = kinds[type(model)]
    if fp8 and kind not in ("simple", "deeplabv3"):
        raise NotImplementedError(f"build_engine: precision='fp8' is not built for networks.{kind}: its resize"
                                  f"{' and pyramid' if kind == 'psp' else ''} nodes are fp16 (simple and deeplabv3 are)")
    if model.training:
        raise RuntimeError("freeze: the model is in training mode; call model.eval() first (BatchNorm is folded from "
                           "its running statistics)")
    own = {"simple": ("last_conv",), "deeplabv3": ("aspp", "last_conv"), "deeplabv3p": ("aspp", "decoder"),
           "psp": ("ppm", "last_conv")}[kind]
    pl = _Planner(fp8)
    with torch.no_grad():
        x = pl.buffer([(0, 3)], fmt="f16")          # buffer 0: the converted input image
        for name, _ in model.named_children():
            if name not in ("backbone", "conv_deepsup", "criterion") + own:
                raise NotImplementedError(f"freeze: module {name} of {type(model).__module__}")
        if kind == "psp":
            out = _plan_psp(pl, model, x)
        elif kind == "deeplabv3p":
            out = _plan_deeplabv3p(pl, model, x)
        else:
            x = _plan_backbone(pl, model.backbone, x)[4]
            if kind == "deeplabv3":
                x = _plan_aspp(pl, model.aspp, x)
            out = _plan_sequential(pl, "last_conv", list(model.last_conv.children()), x)
    if out != -1:
        raise NotImplementedError("freeze: last_conv does not end in a classifier conv with a bias")
    meta = {"align_corner": bool(model.align_corner), "num_classes": int(pl.records[-1]["cout"]), "in_channels": 3,
            "dtype": "float16", "model": kind}
    if not fp8:
        return Engine({"format": FORMAT, "meta": meta, "plan": pl.records, "buffers": list(pl.pitch), "tensors": pl.tensors})
    pl.finalize_f8(amax)
    meta["dtype"] = "float8_e4m3fn"
    return Engine({"format": FORMAT_F8, "meta": meta, "plan": pl.records, "buffers": list(pl.pitch),
                   "buffer_fmt": list(pl.fmt), "scales": list(pl.scales), "tensors": pl.tensors})


def freeze(model, dtype=torch.float16):
    """Freeze an eval-mode networks.deeplabv3 / networks.simple Seg_Model into an Engine (on the CPU; .to(device) or
    load_engine(state, device) puts it on the GPU).  conv_deepsup is dropped.

    This is the engine's first entry point and it keeps its contract, which includes refusing the other heads by name;
    build_engine is the entry point for all four heads and returns exactly this engine for these two."""
    return _freeze(model, dtype, ("deeplabv3", "simple"))


def build_engine(model, dtype=torch.float16, precision="fp16", amax=None):
    """Freeze an eval-mode Seg_Model of networks.simple / deeplabv3 / deeplabv3p / psp into an Engine (on the CPU;
    .to(device) or load_engine(state, device) puts it on the GPU).  conv_deepsup is dropped.  What the planner does not
    know - a pyramid size outside 1 .. 8, more than 4 stages, a stage conv that is not a bias-free 1x1 - raises
    NotImplementedError naming the module.

    precision="fp8" (networks.simple and deeplabv3; opt-in) builds the calibrated e4m3 engine: `amax`
    is the {record name: absolute maximum of that record's output} dict of deploy.calibrate(fp16 engine, batches); a
    record it lacks raises KeyError naming it.  The conv that reads the image and the image-pool branch stay fp16."""
    return _freeze(model, dtype, ("deeplabv3", "simple", "deeplabv3p", "psp"), precision, amax)


def calibrate(engine, batches):
    """{record name: absolute maximum of what that record wrote} of an fp16 engine on the device over an iterable of
    float32 [N,3,H,W] images: the `amax` of build_engine(precision="fp8").  Maxima across the batches."""
    if engine.format != FORMAT:
        raise ValueError("calibrate: the calibration run is made on an fp16 engine")
    amax = {}
    for image in batches:
        for name, t in engine.trace(image.to(engine.device)).items():
            amax[name] = max(amax.get(name, 0.0), float(t.float().abs().amax()))
    return amax


def load_engine(path_or_dict, device=None):
    """The engine saved by torch.save(engine.state_dict(), path) (or that dict itself), on `device`."""
    state = path_or_dict
    if not isinstance(state, dict):
        state = torch.load(path_or_dict, map_location="cpu", weights_only=True)
    eng = Engine(state)
    return eng.to(device) if device is not None else eng


class Engine:
    """A frozen fp16 (format 1) or fp8 (format 2) inference program.  Holds the plan, the packed tensors and, per device, a pool of activation
    slots: buffers whose lifetimes do not overlap share a slot, a slot grows to the largest tenant seen, and the
    per-input-shape launch list is built once and reused."""

    def __init__(self, state):
        if state.get("format") not in (FORMAT, FORMAT_F8):
            raise ValueError(f"engine format {state.get('format')}: this build reads formats {FORMAT} and {FORMAT_F8}")
        self.format = state["format"]
        self.meta = dict(state["meta"])
        self.plan = [dict(r) for r in state["plan"]]
        self.buffers = list(state["buffers"])
        # format 2: the storage format of every buffer ("f16" / "f8") and its scale (real value = stored value * scale)
        self.buffer_fmt = list(state["buffer_fmt"]) if self.format == FORMAT_F8 else ["f16"] * len(self.buffers)
        self.scales = list(state["scales"]) if self.format == FORMAT_F8 else [1.0] * len(self.buffers)
        self.tensors = list(state["tensors"])
        self.align_corner = self.meta["align_corner"]
        self.num_classes = self.meta["num_classes"]
        self.device = torch.device("cpu")
        self.training = False
        first, last = {0: -1}, {}
        for i, r in enumerate(self.plan):
            for b in [r["src"], r["dst"], r.get("res", -1)] + list(r.get("dsts", ())):
                if b >= 0:
                    first.setdefault(b, i)
                    last[b] = i
        self._slot_of, free, nslots = {}, [], 0     # liveness: buffer -> slot, the same for every input shape
        for i in range(-1, len(self.plan)):
            for b in sorted(k for k, v in first.items() if v == i):
                if free:
                    self._slot_of[b] = free.pop()
                else:
                    self._slot_of[b] = nslots; nslots += 1
            free += [self._slot_of[b] for b in sorted(k for k, v in last.items() if v == i)]
        self._slots = [None] * nslots
        self._generation = 0
        self._programs = {}
        self._avg_ws = None

    # ---- persistence / placement
    def state_dict(self):
        """Tensors and plain Python containers only: the plan plus the packed tensors (on the CPU)."""
        state = {"format": self.format, "meta": dict(self.meta), "plan": [dict(r) for r in self.plan],
                 "buffers": list(self.buffers), "tensors": [t.detach().cpu() for t in self.tensors]}
        if self.format == FORMAT_F8:
            state.update(buffer_fmt=list(self.buffer_fmt), scales=list(self.scales))
        return state

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.tensors = [t.to(device) for t in self.tensors]
        self.device = device
        self._slots = [None] * len(self._slots)
        self._programs, self._avg_ws = {}, None
        self._generation += 1
        return self

    def eval(self):
        return self

    # ---- running the plan
    def buffer_shapes(self, H, W):
        """{buffer id: (h, w)} of every activation buffer for an H x W input (-1: the fp32 low-resolution logits)."""
        hw = {0: (H, W)}
        for r in self.plan:
            h, w = hw[r["src"]]
            if r["op"] == "conv":
                ext = r["dil"] * (r["k"] - 1) + 1
                o = ((h + 2 * r["pad"] - ext) // r["stride"] + 1, (w + 2 * r["pad"] - ext) // r["stride"] + 1)
            elif r["op"] == "maxpool":
                o = ((h - 1) // 2 + 1, (w - 1) // 2 + 1)
            elif r["op"] == "avgpool":
                o = (1, 1)
            elif r["op"] == "pyramid":               # one s x s map per level; "dst" is the first of them
                for b, s in zip(r["dsts"], r["sizes"]):
                    if hw.setdefault(b, (s, s)) != (s, s):
                        raise RuntimeError(f"deploy.Engine: {r['name']} writes {(s, s)} into a {hw[b]} buffer")
                o = (r["sizes"][0],) * 2
            elif r["op"] == "cast":
                o = (h, w)
            elif r["op"] in ("broadcast", "resize"):   # the destination's own size
                if r["dst"] not in hw:
                    raise RuntimeError(f"deploy.Engine: {r['name']} writes a buffer of unknown size")
                o = hw[r["dst"]]
            else:
                raise RuntimeError(f"deploy.Engine: unknown op {r['op']} ({r['name']})")
            if min(o) < 1:
                raise RuntimeError(f"deploy.Engine: a {H}x{W} input is too small for {r['name']}")
            if hw.setdefault(r["dst"], o) != o:
                raise RuntimeError(f"deploy.Engine: {r['name']} writes {o} into a {hw[r['dst']]} buffer")
            r_res = r.get("res", -1)
            if r_res >= 0 and hw[r_res] != o:
                raise RuntimeError(f"deploy.Engine: {r['name']}: residual {hw[r_res]} on {o}")
        return hw

    def _program(self, N, H, W):
        key = (N, H, W)
        prog = self._programs.get(key)
        if prog is not None and prog[0] == self._generation:
            return prog
        L = _lib.lib()
        hw = self.buffer_shapes(H, W)
        need = [0] * len(self._slots)
        for b, (h, w) in hw.items():
            if b >= 0:
                s = self._slot_of[b]
                need[s] = max(need[s], N * h * w * self.buffers[b] * _ESIZE[self.buffer_fmt[b]])
        grown = False
        for s, n in enumerate(need):
            if self._slots[s] is None or self._slots[s].numel() < n:
                self._slots[s] = torch.empty(n, dtype=torch.uint8, device=self.device)
                grown = True
        # the partial sums of the average pool and of the pyramid pool (one workspace: the launches of a call run in
        # order on one stream): sized before any launch list is built and grown like a slot, so that no cached list
        # keeps a pointer into a buffer that has been given back
        ws_of = {}
        for i, r in enumerate(self.plan):
            h, w = hw[r["src"]]
            if r["op"] == "avgpool":
                ws_of[i] = int(L.dcfp_avgpool_nhwc_f16_workspace_bytes(N, self.buffers[r["src"]], h * w))
            elif r["op"] == "pyramid":
                sizes = (C.c_int * len(r["sizes"]))(*r["sizes"])
                ws_of[i] = int(L.dcfp_pyramid_pool_nhwc_f16_workspace_bytes(N, h, w, r["c8"], len(sizes), sizes))
                if ws_of[i] == 0:
                    raise RuntimeError(f"deploy.Engine: {r['name']}: pyramid {r['sizes']} on a {h}x{w} map is not supported")
        ws_need = max(list(ws_of.values()) + [0])
        if ws_need and (self._avg_ws is None or self._avg_ws.numel() < ws_need):
            self._avg_ws = torch.empty(ws_need, dtype=torch.uint8, device=self.device)
            grown = True
        if grown:
            self._generation += 1
            self._programs = {}

        def ptr(b):
            return C.c_void_p(self._slots[self._slot_of[b]].data_ptr())
        calls, descs, out_shape, out_call = [], [], None, None
        for i, r in enumerate(self.plan):
            h, w = hw[r["src"]]
            name = r["name"]
            f8 = r.get("fmt") == "f8"
            if r["op"] == "conv" and f8:
                ho, wo = hw[r["dst"]]
                f32 = r["f32"]
                d = _lib.ConvF8Desc(N, h, w, r["cin8"], self.buffers[r["src"]], r["cout"], r["k"], r["stride"], r["pad"],
                                    r["dil"], ho, wo, 0 if f32 else self.buffers[r["dst"]], r["y_off"],
                                    self.buffers[r["res"]] if r["res"] >= 0 else 0, 0, int(r["relu"]), r["res_mul"])
                descs.append(d)
                wt, mul, add = (C.c_void_p(self.tensors[r[k]].data_ptr()) for k in ("w", "mul", "add"))
                if f32:
                    out_shape = (N, r["cout"], ho, wo)
                    out_call = (name, L.dcfp_conv2d_fwd_f8_nhwc_to_f32_nchw, (C.byref(d), ptr(r["src"]), wt, mul, add))
                else:
                    calls.append((name, L.dcfp_conv2d_fwd_f8_nhwc,
                                  (C.byref(d), ptr(r["src"]), wt, mul, add,
                                   ptr(r["res"]) if r["res"] >= 0 else None, ptr(r["dst"]))))
            elif r["op"] == "cast":
                calls.append((name, L.dcfp_cast_nhwc_f16_to_f8,
                              (ptr(r["src"]), self.buffers[r["src"]], ptr(r["dst"]), self.buffers[r["dst"]], r["y_off"],
                               N * h * w, r["c"], r["scale"])))
            elif r["op"] == "maxpool" and f8:
                ho, wo = hw[r["dst"]]
                calls.append((name, L.dcfp_maxpool3x3s2_nhwc_f8,
                              (ptr(r["src"]), ptr(r["dst"]), N, h, w, self.buffers[r["src"]], self.buffers[r["src"]],
                               ho, wo, self.buffers[r["dst"]])))
            elif r["op"] == "avgpool" and f8:
                c16 = self.buffers[r["src"]]
                calls.append((name, L.dcfp_avgpool_nhwc_f8_to_f16,
                              (ptr(r["src"]), ptr(r["dst"]), N, h * w, c16, c16, self.buffers[r["dst"]], r["scale"],
                               C.c_void_p(self._avg_ws.data_ptr()), ws_of[i])))
            elif r["op"] == "broadcast" and f8:
                ho, wo = hw[r["dst"]]
                calls.append((name, L.dcfp_broadcast_nhwc_f16_to_f8,
                              (ptr(r["src"]), self.buffers[r["src"]], ptr(r["dst"]), N, ho * wo, r["c"],
                               self.buffers[r["dst"]], r["y_off"], r["scale"])))
            elif r["op"] == "conv":
                ho, wo = hw[r["dst"]]
                f32 = r["f32"]
                d = _lib.ConvF16Desc(N, h, w, r["cin8"], self.buffers[r["src"]], r["cout"] if f32 else _r8(r["cout"]),
                                     r["k"], r["stride"], r["pad"], r["dil"], ho, wo,
                                     0 if f32 else self.buffers[r["dst"]], r["y_off"],
                                     self.buffers[r["res"]] if r["res"] >= 0 else 0, 0, int(r["relu"]))
                descs.append(d)
                wt, sh = C.c_void_p(self.tensors[r["w"]].data_ptr()), C.c_void_p(self.tensors[r["shift"]].data_ptr())
                if f32:
                    out_shape = (N, r["cout"], ho, wo)
                    out_call = (name, L.dcfp_conv2d_fwd_f16_nhwc_to_f32_nchw, (C.byref(d), ptr(r["src"]), wt, sh))
                else:
                    calls.append((name, L.dcfp_conv2d_fwd_f16_nhwc,
                                  (C.byref(d), ptr(r["src"]), wt, sh, ptr(r["res"]) if r["res"] >= 0 else None,
                                   ptr(r["dst"]))))
            elif r["op"] == "maxpool":
                ho, wo = hw[r["dst"]]
                calls.append((name, L.dcfp_maxpool3x3s2_nhwc_f16,
                              (ptr(r["src"]), ptr(r["dst"]), N, h, w, self.buffers[r["src"]], self.buffers[r["src"]],
                               ho, wo, self.buffers[r["dst"]])))
            elif r["op"] == "avgpool":
                c8 = self.buffers[r["src"]]
                calls.append((name, L.dcfp_avgpool_nhwc_f16,
                              (ptr(r["src"]), ptr(r["dst"]), N, h * w, c8, c8, self.buffers[r["dst"]],
                               C.c_void_p(self._avg_ws.data_ptr()), ws_of[i])))
            elif r["op"] == "broadcast":
                ho, wo = hw[r["dst"]]
                c8 = self.buffers[r["src"]]
                calls.append((name, L.dcfp_broadcast_nhwc_f16,
                              (ptr(r["src"]), c8, ptr(r["dst"]), N, ho * wo, c8, self.buffers[r["dst"]], r["y_off"])))
            elif r["op"] == "resize":
                ho, wo = hw[r["dst"]]
                calls.append((name, L.dcfp_resize_bilinear_nhwc_f16,
                              (ptr(r["src"]), N, h, w, self.buffers[r["src"]], self.buffers[r["src"]], ptr(r["dst"]),
                               ho, wo, self.buffers[r["dst"]], r["y_off"], int(r["align"]))))
            elif r["op"] == "pyramid":
                n = len(r["sizes"])
                sizes = (C.c_int * n)(*r["sizes"])
                outs = (C.c_void_p * n)(*[ptr(b).value for b in r["dsts"]])
                pitches = (C.c_int * n)(*[self.buffers[b] for b in r["dsts"]])
                descs.append((sizes, outs, pitches))     # (kept alive with the launch list)
                calls.append((name, L.dcfp_pyramid_pool_nhwc_f16,
                              (ptr(r["src"]), N, h, w, r["c8"], self.buffers[r["src"]], r["x_off"], n, sizes, outs,
                               pitches, C.c_void_p(self._avg_ws.data_ptr()), ws_of[i])))
            else:
                raise RuntimeError(f"deploy.Engine: unknown op {r['op']} ({name})")
        if out_call is None:
            raise RuntimeError("deploy.Engine: the plan has no classifier")
        prog = (self._generation, calls, out_call, out_shape, descs, ptr(0))
        self._programs[key] = prog
        return prog

    def _check_image(self, image):
        if self.device.type != "cuda" or not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise RuntimeError("deploy.Engine runs on the MI355X HIP kernels only: engine.to('cuda') and a CUDA image "
                               "(no CPU fallback exists)")
        if image.device != self.device:
            raise RuntimeError(f"deploy.Engine: the engine is on {self.device}, the image on {image.device}")
        if image.dtype != torch.float32 or image.dim() != 4 or image.shape[1] != self.meta["in_channels"]:
            raise RuntimeError(f"deploy.Engine: image must be float32 [N,{self.meta['in_channels']},H,W]")

    @torch.no_grad()
    def lowres_logits(self, image, deepsup=False):
        """[fp32 N x classes x h x w logits at 1/os resolution] (the deep-supervision head is not part of an engine)."""
        self._check_image(image)
        image = image.contiguous()
        N, Cc, H, W = image.shape
        with torch.cuda.device(self.device):         # (the launches go to the engine's device and its current stream)
            return self._run(image, N, Cc, H, W)

    def _run(self, image, N, Cc, H, W, tap=None):
        _, calls, out_call, out_shape, _, in_ptr = self._program(N, H, W)
        L, stream = _lib.lib(), ops._stream()
        check(L.dcfp_nchw_f32_to_nhwc_f16(C.c_void_p(image.data_ptr()), in_ptr, N, Cc, H, W, self.buffers[0], stream),
              "deploy: input conversion")
        for i, (name, fn, args) in enumerate(calls):
            check(fn(*args, stream), "deploy: " + name)
            if tap is not None:
                tap(i)
        out = torch.empty(out_shape, dtype=torch.float32, device=image.device)
        name, fn, args = out_call
        check(fn(*args, C.c_void_p(out.data_ptr()), stream), "deploy: " + name)
        return [out]

    def _buffer_view(self, b, N, hw):
        """Buffer b of the current program as an [N, h, w, pitch] tensor of its storage dtype (a view of its slot)."""
        h, w = hw[b]
        fmt = self.buffer_fmt[b]
        raw = self._slots[self._slot_of[b]][:N * h * w * self.buffers[b] * _ESIZE[fmt]]
        return raw.view(F8 if fmt == "f8" else torch.float16).view(N, h, w, self.buffers[b])

    def _written(self, r, N, hw):
        """The bytes record r wrote: its channel slice of its destination buffer."""
        if r["op"] == "pyramid":
            return torch.cat([self._buffer_view(b, N, hw).reshape(-1) for b in r["dsts"]])
        y = self._buffer_view(r["dst"], N, hw)
        g = _GRAN[self.buffer_fmt[r["dst"]]]
        if r["op"] == "conv":
            return y[..., r["y_off"]:r["y_off"] + _rg(r["cout"], g)]
        if r["op"] in ("broadcast", "resize"):
            width = _rg(r["c"], g) if "c" in r else self.buffers[r["src"]]
            return y[..., r["y_off"]:r["y_off"] + width]
        return y

    def backbone_record(self):
        """Index (among the launch list) and record of the conv whose output is the backbone's last tensor: the last
        `backbone.layer4.*.conv3`, which carries the block's residual add and ReLU."""
        recs = [r for r in self.plan if not (r["op"] == "conv" and r["f32"])]
        hits = [i for i, r in enumerate(recs) if r["op"] == "conv" and r["name"].startswith("backbone.layer4.")
                and r["name"].endswith(".conv3")]
        if not hits:
            raise NotImplementedError("deploy.Engine: the plan holds no backbone.layer4.*.conv3 record")
        return hits[-1], recs[hits[-1]]

    @torch.no_grad()
    def lowres_logits_and_feature(self, image):
        """(fp32 low-resolution logits, feature, channels) of ONE run: `feature` is a contiguous fp16 NHWC clone
        [N, h, w, pitch] of what backbone_record() wrote - the stage output the head reads, for networks.psp a channel
        slice of the concat buffer - taken right after that launch; its first `channels` channels are the feature, the
        rest is the granule's padding.  An fp8 engine stores e4m3 there and is refused."""
        if self.format == FORMAT_F8:
            raise NotImplementedError("deploy.Engine: the feature of an fp8 engine is e4m3; build the teacher as fp16")
        self._check_image(image)
        image = image.contiguous()
        N, Cc, H, W = image.shape
        at, rec = self.backbone_record()
        got = []
        with torch.cuda.device(self.device):
            self._program(N, H, W)                   # (sizes the slots before any view of them is taken)
            hw = self.buffer_shapes(H, W)

            def tap(i):
                if i == at:
                    got.append(self._written(rec, N, hw).clone(memory_format=torch.contiguous_format))
            logits = self._run(image, N, Cc, H, W, tap)[0]
        return logits, got[0], rec["cout"]

    @torch.no_grad()
    def trace(self, image):
        """{record name: a clone of the bytes that record wrote} of one run, in the stored dtype (fp16 / e4m3 NHWC
        slices; the classifier's fp32 NCHW logits), plus "input": the converted image.  A debugging and testing path:
        it runs the launch list with a clone after each call."""
        self._check_image(image)
        image = image.contiguous()
        N, Cc, H, W = image.shape
        out = {}
        with torch.cuda.device(self.device):
            self._program(N, H, W)                   # (sizes the slots before any view of them is taken)
            hw = self.buffer_shapes(H, W)
            recs = [r for r in self.plan if not (r["op"] == "conv" and r["f32"])]
            last = [r for r in self.plan if r["op"] == "conv" and r["f32"]][-1]

            def tap(i):
                if i == 0:
                    out["input"] = self._buffer_view(0, N, hw).clone()
                out[recs[i]["name"]] = self._written(recs[i], N, hw).clone()
            logits = self._run(image, N, Cc, H, W, tap)[0]
        out[last["name"]] = logits
        return out

    @torch.no_grad()
    def __call__(self, image, labels=None, deepsup=False):
        """[fp32 N x classes x H x W logits]: the low-resolution logits through the bilinear upsample kernel."""
        lowres = self.lowres_logits(image)
        return [ops.upsample_bilinear(z, image.shape[2:], self.align_corner) for z in lowres]

    def conv_records(self):
        return [r for r in self.plan if r["op"] == "conv"]


# ---------------------------------------------------------------------------------------------------------------------
# The flat engine file and the C runtime: an engine as a file a C program loads and runs
# (include/dcfp_hip.h, dcfp_engine_*; csrc/engine_file.cpp parses it, csrc/engine_rt.hip runs it).

FLAT_VERSION = 1
FLAT_MAGIC = b"DCFPENG\0"
FLAT_SECTIONS = ("meta", "records", "buffers", "tensors", "strings", "weights", "input")
FLAT_HEADER_BYTES = 32 + 16 * len(FLAT_SECTIONS)
FLAT_RECORD_INTS, FLAT_RECORD_BYTES = 32, 136       # 32 int32 fields, then the floats res_mul and scale
FLAT_WEIGHT_ALIGN = 256
_FLAT_OPS = {"conv": 1, "maxpool": 2, "avgpool": 3, "broadcast": 4, "cast": 5, "resize": 6, "pyramid": 7}
_FLAT_FMT = {"f16": 0, "f8": 1}
_FLAT_DTYPE = {torch.float16: 0, torch.float32: 1, F8: 2}
_FLAT_MODELS = ("simple", "deeplabv3", "deeplabv3p", "psp")


def input_table(mean, std):
    """fp16 [3, 256]: table[c][v] = (v / 255 - mean[c]) / std[c], formed in fp64 and rounded once - what the uint8
    input kernel looks a byte up in (dcfp_image_u8_hwc_to_nhwc_f16)."""
    mean, std = torch.tensor(list(mean), dtype=torch.float64), torch.tensor(list(std), dtype=torch.float64)
    if mean.numel() != 3 or std.numel() != 3:
        raise ValueError("input_table: mean and std hold one value per colour channel")
    v = torch.arange(256, dtype=torch.float64).view(1, 256)
    return ((v / 255.0 - mean.view(3, 1)) / std.view(3, 1)).to(torch.float16)


def _f32_bits(v):
    """The 4 bytes of the float a ctypes call makes of a Python number."""
    return bytes(C.c_float(float(v)))


def _pad_to(b, align):
    return b + b"\0" * (-len(b) % align)


def flat_bytes(engine, mean=None, std=None, bgr=True):
    """The flat engine file (version FLAT_VERSION, layout in DESIGN.md §11b) of `engine`, as bytes: only what
    engine.state_dict() holds, plus - when mean / std are given - the uint8 input table and the channel order."""
    import struct
    state = engine.state_dict()
    meta, plan, fmt8 = state["meta"], state["plan"], state["format"] == FORMAT_F8
    if (mean is None) != (std is None):
        raise ValueError("save_flat: give both mean and std, or neither")
    names, name_off = b"", []
    for r in plan:
        name_off.append(len(names))
        names += r["name"].encode() + b"\0"
    records = b""
    for r, noff in zip(plan, name_off):
        f8 = r.get("fmt") == "f8"
        sizes, dsts = list(r.get("sizes", ())), list(r.get("dsts", ()))
        conv = r["op"] == "conv"
        ints = [_FLAT_OPS[r["op"]], noff, _FLAT_FMT[r.get("fmt", "f16")], r["src"], r["dst"], r.get("res", -1),
                r.get("k", 0), r.get("stride", 0), r.get("pad", 0), r.get("dil", 0), r.get("cin8", 0), r.get("cout", 0),
                r.get("y_off", 0), r.get("x_off", 0), r.get("c", 0), r.get("c8", 0), int(r.get("relu", False)),
                int(r.get("f32", False)), int(r.get("align", False)), len(sizes)]
        ints += (sizes + [0] * 4)[:4] + (dsts + [-1] * 4)[:4]
        ints += [r["w"], r["mul"] if f8 else r["shift"], r["add"] if f8 else -1] if conv else [-1, -1, -1]
        ints += [0]
        assert len(ints) == FLAT_RECORD_INTS and len(sizes) <= 4
        records += struct.pack(f"<{FLAT_RECORD_INTS}i", *ints) + _f32_bits(r.get("res_mul", 0.0)) + \
            _f32_bits(r.get("scale", 0.0))
    fmts = state["buffer_fmt"] if fmt8 else ["f16"] * len(state["buffers"])
    scales = state["scales"] if fmt8 else [1.0] * len(state["buffers"])
    buffers = b"".join(struct.pack("<ii", p, _FLAT_FMT[f]) + _f32_bits(s) + struct.pack("<i", 0)
                       for p, f, s in zip(state["buffers"], fmts, scales))
    tensors, blob = b"", bytearray()
    for t in state["tensors"]:
        raw = t.contiguous().view(torch.uint8).numpy().tobytes()
        blob += b"\0" * (-len(blob) % FLAT_WEIGHT_ALIGN)       # every tensor starts on a 256-byte boundary
        tensors += struct.pack("<iiQQ", _FLAT_DTYPE[t.dtype], 0, len(raw), len(blob))
        blob += raw
    meta_b = struct.pack("<8i", state["format"], int(meta["align_corner"]), meta["num_classes"], meta["in_channels"],
                         _FLAT_MODELS.index(meta["model"]), len(plan), len(state["buffers"]), len(state["tensors"]))
    parts = {"meta": meta_b, "records": records, "buffers": buffers, "tensors": tensors, "strings": names,
             "weights": bytes(blob), "input": b""}
    if mean is not None:
        order = [2, 1, 0] if bgr else [0, 1, 2]
        parts["input"] = input_table(mean, std).numpy().tobytes() + struct.pack("<4i", *order, 0)
    out, table = bytearray(b"\0" * FLAT_HEADER_BYTES), []
    for name in FLAT_SECTIONS:                       # the weight blob and the table behind it start on 256 bytes
        out += b"\0" * (-len(out) % (FLAT_WEIGHT_ALIGN if name in ("weights", "input") else 16))
        table.append((len(out), len(parts[name])))
        out += parts[name]
    head = FLAT_MAGIC + struct.pack("<IIQII", FLAT_VERSION, FLAT_HEADER_BYTES, len(out), len(FLAT_SECTIONS), 0)
    head += b"".join(struct.pack("<QQ", o, n) for o, n in table)
    out[:FLAT_HEADER_BYTES] = head
    return bytes(out)


def save_flat(engine, path, mean=None, std=None, bgr=True):
    """Write `engine` as a flat engine file: what dcfp_engine_open, deploy.CEngine and tools/engine_run.cpp load.
    mean / std (per RGB channel, of the 0 .. 1 image): the file also carries the uint8 input table, without which it
    cannot take uint8 input; bgr: the uint8 frames are B, G, R (the loaders' order), else R, G, B."""
    data = flat_bytes(engine, mean, std, bgr)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def flat_sections(data):
    """{section name: (offset, size)} of a flat engine file's bytes, as its header states them."""
    import struct
    return {name: struct.unpack_from("<QQ", data, 32 + 16 * i) for i, name in enumerate(FLAT_SECTIONS)}


def is_flat_file(path):
    with open(path, "rb") as f:
        return f.read(len(FLAT_MAGIC)) == FLAT_MAGIC


class CEngine:
    """A flat engine file run by the library's C runtime (dcfp_engine_*): the plan is parsed, sized and launched in C;
    this wrapper owns the torch-allocated weight and workspace tensors and offers what an Engine offers the
    evaluation drivers: engine(image) -> [logits], engine.lowres_logits(image) -> [lowres], engine.align_corner, plus
    run_u8(uint8 [N,H,W,3] image) -> [lowres] for a file that carries the input table.  Same kernels, same arguments,
    same bits as the Engine the file was written from.  Not thread-safe (one handle, one cache of launch lists)."""

    def __init__(self, path_or_bytes, device="cuda"):
        L = _lib.lib()
        self._lib = L
        self.handle = C.c_void_p()
        err = C.create_string_buffer(256)
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            data = bytes(path_or_bytes)
            st = L.dcfp_engine_open_memory(data, len(data), C.byref(self.handle), err, len(err))
        else:
            st = L.dcfp_engine_open(os.fsencode(path_or_bytes), C.byref(self.handle), err, len(err))
        if st != 0:
            self.handle = C.c_void_p()
            raise ValueError(f"deploy.CEngine: {err.value.decode(errors='replace')} (status {st})")
        info = _lib.EngineInfo()
        check(L.dcfp_engine_info(self.handle, C.byref(info)), "deploy.CEngine: info")
        self.format, self.num_classes, self.align_corner = info.format, info.num_classes, bool(info.align_corner)
        self.has_input_table = bool(info.has_input_table)
        self.meta = {"align_corner": self.align_corner, "num_classes": info.num_classes, "in_channels": info.in_channels,
                     "dtype": "float16" if info.format == FORMAT else "float8_e4m3fn", "model": _FLAT_MODELS[info.model]}
        self.n_records, self.n_buffers, self.n_slots = info.n_records, info.n_buffers, info.n_slots
        self.training = False
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("deploy.CEngine runs on the MI355X HIP kernels only (no CPU fallback exists)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.weights = torch.empty(int(L.dcfp_engine_weight_bytes(self.handle)), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            check(L.dcfp_engine_upload(self.handle, C.c_void_p(self.weights.data_ptr()), ops._stream()),
                  "deploy.CEngine: upload")
            torch.cuda.current_stream().synchronize()
        self._workspace = None

    def __del__(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self._lib.dcfp_engine_close(self.handle)
            self.handle = C.c_void_p()

    def eval(self):
        return self

    def output_shape(self, N, H, W):
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        st = self._lib.dcfp_engine_output_shape(self.handle, N, H, W, C.byref(c), C.byref(h), C.byref(w))
        if st != 0:
            raise RuntimeError(f"deploy.CEngine: a {N}x{H}x{W} input is too small for a layer or not supported "
                               f"(status {st})")
        return (N, c.value, h.value, w.value)

    def buffer_shapes(self, H, W):
        """{buffer id: (h, w)}, what Engine.buffer_shapes returns (-1: the low-resolution logits)."""
        pairs = (C.c_int * (2 * self.n_buffers))()
        st = self._lib.dcfp_engine_buffer_shapes(self.handle, H, W, pairs, self.n_buffers)
        if st != 0:
            raise RuntimeError(f"deploy.CEngine: a {H}x{W} input is too small for a layer or not supported (status {st})")
        hw = {b: (pairs[2 * b], pairs[2 * b + 1]) for b in range(self.n_buffers) if pairs[2 * b] > 0}
        hw[-1] = self.output_shape(1, H, W)[2:]
        return hw

    def workspace_bytes(self, N, H, W):
        return int(self._lib.dcfp_engine_workspace_bytes(self.handle, N, H, W))

    def workspace(self, N, H, W):
        """The workspace tensor a call of this shape runs in (grown to the largest shape seen; its bytes need no
        initialising)."""
        need = self.workspace_bytes(N, H, W)
        if need == 0:
            raise RuntimeError(f"deploy.CEngine: a {N}x{H}x{W} input is too small for a layer or not supported")
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspace

    def _check_image(self, image, dtype, what):
        if not isinstance(image, torch.Tensor) or not image.is_cuda or image.device != self.device:
            raise RuntimeError(f"deploy.CEngine: the engine is on {self.device}; the image must be a tensor there")
        if image.dtype != dtype or image.dim() != 4:
            raise RuntimeError(f"deploy.CEngine: image must be {what}")

    def _launch(self, run, image, extra, N, H, W):
        with torch.cuda.device(self.device):
            out = torch.empty(self.output_shape(N, H, W), dtype=torch.float32, device=self.device)
            ws = self.workspace(N, H, W)
            check(run(self.handle, C.c_void_p(self.weights.data_ptr()), C.c_void_p(image.data_ptr()), *extra, N, H, W,
                      C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(out.data_ptr()), ops._stream()),
                  "deploy.CEngine: run")
        return [out]

    @torch.no_grad()
    def lowres_logits(self, image, deepsup=False):
        """[fp32 N x classes x h x w logits at 1/os resolution] of a float32 [N,3,H,W] image."""
        self._check_image(image, torch.float32, f"float32 [N,{self.meta['in_channels']},H,W]")
        if image.shape[1] != self.meta["in_channels"]:
            raise RuntimeError(f"deploy.CEngine: image must be float32 [N,{self.meta['in_channels']},H,W]")
        image = image.contiguous()
        N, _, H, W = image.shape
        return self._launch(self._lib.dcfp_engine_run_f32, image, (), N, H, W)

    @torch.no_grad()
    def run_u8(self, image_u8):
        """[fp32 low-resolution logits] of a uint8 [N,H,W,3] image (the channel order the file was saved for),
        normalised on the device by the file's table.  Rows may be pitched: image_u8[:, :, :W] of a wider tensor."""
        self._check_image(image_u8, torch.uint8, "uint8 [N,H,W,3]")
        N, H, W, Cc = image_u8.shape
        if Cc != 3:
            raise RuntimeError("deploy.CEngine: image must be uint8 [N,H,W,3]")
        if not self.has_input_table:
            raise RuntimeError("deploy.CEngine: this engine file carries no input table (save_flat(mean=, std=))")
        sn, sh, sw, sc = image_u8.stride()
        if sc != 1 or sw != 3 or sh < 3 * W or (N > 1 and sn != H * sh):
            image_u8 = image_u8.contiguous()
            sh = 3 * W
        return self._launch(self._lib.dcfp_engine_run_u8, image_u8, (sh,), N, H, W)

    @torch.no_grad()
    def __call__(self, image, labels=None, deepsup=False):
        """[fp32 N x classes x H x W logits]: the low-resolution logits through the bilinear upsample kernel."""
        lowres = self.lowres_logits(image)
        return [ops.upsample_bilinear(z, image.shape[2:], self.align_corner) for z in lowres]
