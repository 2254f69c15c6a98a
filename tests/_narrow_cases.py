"""The convolutions a pruned model is left with at 1, 2 and 5 channels, and one small stand-in for every kernel they
reach.  The pruner keeps max(1, int(C * layer_keep)) channels per layer, so every slim model has layers of a handful of
channels: slim_convs() lists them from the golden prune fixtures and the model definition, classes_of() says which
forward / data-gradient / weight-gradient kernel each takes and which side of that pass is the narrow one, and NARROW
holds, per such class, the smallest shape that still routes the same way.  tests/test_narrow_routing_host_cpu.py holds
every routing written here to dcfp_conv2d_kernel_name and proves NARROW complete against slim_convs over all fixtures;
tests/test_narrow_widths_gpu.py runs the rows.  A plain helper module like tests/_wp_cases.py: no fixtures, no tests.

A case is (N, Cin, H, W, Cout, k, stride, pad, dil).  The operands carry the row pitch the network would give them
(pitch_of: ops.conv_pitch, what networks/_exec.py asks for in front of a 3x3 stride-1 conv); where that is non-zero the
kernel names below are those of the pitched descriptor."""
import glob
import math
import os

import numpy as np

FWD, DGRAD, WGRAD = 0, 1, 2
PASS_NAMES = ("fwd", "dgrad", "wgrad")
NARROW_MAX = 8
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (N, H, W) of the network input: tools/train.py's default and the full-size configuration of test_fullsize_gpu.py
GEOMETRIES = {"train": (8, 769, 769), "fullsize": (4, 1024, 2048)}
# fixture tag -> (networks module, backbone)
MODELS = {"pspr50": ("psp", "resnet50"), "simple_r50": ("simple", "resnet50"), "v3pr50": ("deeplabv3p", "resnet50"),
          "v3r101": ("deeplabv3", "resnet101"), "v3r50": ("deeplabv3", "resnet50")}
BB = {"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128, "pretrained": False}


def fixtures():
    return sorted(glob.glob(os.path.join(G, "prune_*.npz")))


def _out(size, k, s, p, d):
    return (size + 2 * p - d * (k - 1) - 1) // s + 1


_MODEL_CACHE = {}


def _model_convs(tag):
    """{conv name: (module, place)} of the model definition; place = divisor chain applied to the input size, as a
    function (H, W) -> (H, W) of the map that conv reads, or None where this module does not know the layer's place."""
    if tag in _MODEL_CACHE:
        return _MODEL_CACHE[tag]
    import torch.nn as nn
    from dcfp_amd import networks
    name, backbone = MODELS[tag]
    m = getattr(networks, name).Seg_Model(backbone=backbone, backbone_para=dict(BB), num_classes=19, align_corner=True,
                                          deepsup=True)
    steps = {}          # conv name -> list of (k, s, p, d) of everything in front of it, in execution order
    chain = []
    bb = m.backbone
    for i, mod in enumerate(bb.conv1):
        if isinstance(mod, nn.Conv2d):
            steps[f"backbone.conv1.{i}"] = list(chain)
            chain.append((mod.kernel_size[0], mod.stride[0], mod.padding[0], mod.dilation[0]))
    mp = bb.maxpool
    chain.append((mp.kernel_size, mp.stride, mp.padding, 1))
    for li in range(1, 5):
        for bi, blk in enumerate(getattr(bb, f"layer{li}")):
            pre = f"backbone.layer{li}.{bi}."
            steps[pre + "conv1"] = list(chain)
            steps[pre + "conv2"] = list(chain)
            if blk.downsample is not None:
                steps[pre + "downsample.0"] = list(chain)
            c2 = blk.conv2
            chain.append((c2.kernel_size[0], c2.stride[0], c2.padding[0], c2.dilation[0]))
            steps[pre + "conv3"] = list(chain)
    out = {}
    for cname, mod in m.named_modules():
        if not isinstance(mod, nn.Conv2d):
            continue
        if cname in steps:
            place = steps[cname]
        elif ".global_avg_pool." in cname:
            place = "1x1"                              # behind AdaptiveAvgPool2d((1, 1))
        elif cname.startswith(("aspp.", "last_conv", "conv_deepsup")):
            place = list(chain)                        # the heads read the output-stride-8 maps of layer3 / layer4
        else:
            place = None
        out[cname] = (mod, place)
    # (the fixtures also name the BatchNorms behind the convs: known names that are no conv)
    out[None] = {n for n, mod in m.named_modules() if isinstance(mod, nn.BatchNorm2d)}
    _MODEL_CACHE[tag] = out
    return out


def slim_convs(npz, geometry, named=False):
    """Every conv of the slim model of fixture `npz` (a path under tests/golden) with min(Cin, Cout) <= 8, at the
    feature-map size it has for a network input of GEOMETRIES[geometry]: (N, Cin, H, W, Cout, k, s, p, d) - with
    named=True (layer name, case)."""
    tag = os.path.basename(npz)[len("prune_"):].rsplit("_gp", 1)[0]
    g = np.load(npz)
    N, H0, W0 = GEOMETRIES[geometry]
    convs = _model_convs(tag)
    names = g["names"].tolist()
    names += sorted({k.split(":", 1)[1] for k in g.files if k.startswith(("in_n:", "out_n:"))} - set(names))
    for cname in names:
        if cname not in convs:
            # a BatchNorm of the model, or the fixture and the model definition have drifted apart: a layer that is
            # renamed must not drop out of the enumeration unnoticed
            if cname not in convs[None]:
                raise KeyError(f"{tag}: the fixture names {cname!r}, which is neither a Conv2d nor a BatchNorm2d of the model")
            continue
        mod, place = convs[cname]
        cin = int(g["in_n:" + cname][0]) if "in_n:" + cname in g.files else mod.in_channels
        cout = int(g["out_n:" + cname][0]) if "out_n:" + cname in g.files else mod.out_channels
        if min(cin, cout) > NARROW_MAX:
            continue
        if place is None:
            raise NotImplementedError(f"{tag}: {cname} is narrow ({cin} -> {cout}) and _narrow_cases does not know "
                                      "the size of the map it reads")
        if place == "1x1":
            H, W = 1, 1
        else:
            H, W = H0, W0
            for k, s, p, d in place:
                H, W = _out(H, k, s, p, d), _out(W, k, s, p, d)
        case = (N, cin, H, W, cout, mod.kernel_size[0], mod.stride[0], mod.padding[0], mod.dilation[0])
        yield (cname, case) if named else case


# ------------------------------------------------------------------ routing
def pitch_of(case):
    """The row pitch the network gives the x / dy operands of this conv (0: dense)."""
    from dcfp_amd import ops
    N, Cin, H, W, Cout, k, s, p, d = case
    return ops.conv_pitch((N, Cin, H, W), (Cout, Cin, k, k), s, p, d)


def desc_of(case):
    from dcfp_amd import ops
    N, Cin, H, W, Cout, k, s, p, d = case
    pitch = pitch_of(case)
    return ops._desc((N, Cin, H, W), (Cout, Cin, k, k), s, p, d, pitch, pitch)


def routes(case):
    """(forward, dgrad, wgrad) kernel names of the case as the network would run it."""
    from dcfp_amd import ops
    d = desc_of(case)
    return tuple(ops.conv_kernel_name(d, which) for which in (FWD, DGRAD, WGRAD))


def sides(case, which):
    """Which sides of pass `which` are narrow: "M" where its output rows are <= 8, "K" where its reduction channels
    are (forward: M = Cout, K = Cin; data gradient: M = Cin, K = Cout; weight gradient: M = Cout, the columns Cin*k*k of
    dw reduce over pixels - its narrow "K" side is a narrow Cin)."""
    N, Cin, H, W, Cout, k, s, p, d = case
    m, kk = (Cin, Cout) if which == DGRAD else (Cout, Cin)
    return [side for side, n in (("M", m), ("K", kk)) if n <= NARROW_MAX]


def classes_of(case, names=None):
    """{(pass name, kernel name, side)} of a case."""
    names = names if names is not None else routes(case)
    return {(PASS_NAMES[w], names[w], side) for w in (FWD, DGRAD, WGRAD) if names[w] is not None for side in sides(case, w)}


# ------------------------------------------------------------------ the case table
_T0, _T1, _T2, _T3, _T4, _T5 = "1,4,1,4,0", "2,4,1,4,0", "2,4,2,2,0", "2,2,2,2,0", "4,4,2,2,0", "2,4,2,2,1"


def _ig(taps, cfg):
    return f"igemm2_kernel<{taps},{cfg}>"


D8_1, D8_9, DMA1P, GEMV = "igemm2_dma8_kernel<1>", "igemm2_dma8_kernel<9>", "igemm2_dma1p_kernel", "gemv_1x1_map_kernel"
WG1, WG9 = "wgrad2_kernel<1,2,2,1,1>", "wgrad2_kernel<9,2,2,1,1>"            # the one-wave 64 x 64 tile
WIDE1, WIDE9 = "wgrad_dma_kernel<1,false,true>", "wgrad_dma_kernel<9,false,true>"

# (case, forward kernel, dgrad kernel, wgrad kernel); None = that pass is not run for the row.
#
# How the rows were shrunk (conv_igemm2.hip pick_cfg / dcfp_igemm2_use_dma8, conv_wgrad.hip make_plan):
# * M <= 32 / <= 64 rows take the 32 x 512 / 64 x 512 tile at any map size: 9 x 13 ... 13 x 18 maps, two images, more
#   than one tile only through the batch;
# * the 128 x 256 and 256 x 256 tiles need >= 192 tiles of 256 pixels and, to stay off the LDS-DMA kernels, an output width
#   that is no multiple of 4: 2 x 129 x 191 (as tests/_wp_cases.py), the wide side cut to 65 / 86 / 129 channels;
# * the LDS-DMA routes (dma8, dma1p) need >= 192 tiles and a width that is a multiple of 4: 2 x 128 x 192; the 3x3 convs of
#   dilation 1 / 2 reach them only row-pitched (NARROW_PITCH), dilation 4 dense;
# * the WIDE weight-gradient tile needs W % 16 == 0, stride 1 and more than 128 columns Cin*k*k; at 3x3 also
#   Cin*9 > 1152 and, for dilation 1 / 2, the pitched x it only has on the 2 x 128 x 192 map.
#
# The statistics epilogue: the library emits BatchNorm statistics only from tiles that are all live (Cout a multiple of the
# tile height, 32 at least), so EVERY row with a narrow Cout must decline it (st is None) - the rows in STATS, narrow on
# the reduction side, are the ones that have it.
NARROW = [
    # -- the small tiles, both orientations of each layer pair (c -> 1 with 1 -> c, c -> 2 with 2 -> c, c -> 5 with 5 -> c)
    ((2, 19, 9, 13, 1, 1, 1, 0, 1), _ig(1, _T0), _ig(1, _T0), WG1),
    ((2, 1, 9, 13, 19, 1, 1, 0, 1), _ig(1, _T0), _ig(1, _T0), WG1),                  # wgrad: Nn = 1 on the one-wave tile
    ((2, 37, 9, 13, 2, 1, 1, 0, 1), _ig(1, _T0), _ig(1, _T1), WG1),
    ((2, 2, 9, 13, 37, 1, 1, 0, 1), _ig(1, _T1), _ig(1, _T0), WG1),
    ((2, 20, 11, 15, 1, 3, 1, 1, 1), _ig(9, _T0), _ig(9, _T0), WG9),                 # layer1.0.conv2 at gp70
    ((2, 33, 11, 15, 1, 3, 1, 1, 1), _ig(9, _T0), _ig(9, _T1), WG9),                 # ... at gp50
    ((1, 1, 10, 14, 20, 3, 1, 1, 1), _ig(9, _T0), _ig(9, _T0), WG9),                 # wgrad: Nn = 9 on the one-wave tile
    ((2, 37, 11, 15, 2, 3, 1, 1, 1), _ig(9, _T0), _ig(9, _T1), WG9),
    ((2, 2, 11, 15, 37, 3, 1, 1, 1), _ig(9, _T1), _ig(9, _T0), WG9),                 # K = 18
    # -- dilation 2 and 4 at 3x3, narrow on either side (layer3.1.conv2 and its mirror)
    ((2, 23, 13, 17, 5, 3, 1, 2, 2), _ig(9, _T0), _ig(9, _T0), WG9),
    ((2, 5, 13, 17, 23, 3, 1, 2, 2), _ig(9, _T0), _ig(9, _T0), WG9),                 # K = Nn = 45
    ((2, 21, 13, 18, 5, 3, 1, 4, 4), _ig(9, _T0), _ig(9, _T0), WG9),
    ((2, 5, 13, 18, 21, 3, 1, 4, 4), _ig(9, _T0), _ig(9, _T0), WG9),
    # -- the lop-sided weight-gradient tiles through a narrow Cin: cfg 4 (32 < Nn = 45 <= 64), cfg 3 (64 < Nn = 72 <= 128)
    ((2, 5, 13, 17, 150, 3, 1, 1, 1), _ig(9, _T3), _ig(9, _T0), "wgrad2_kernel<9,4,1,2,2>"),
    ((2, 8, 13, 17, 130, 3, 1, 2, 2), _ig(9, _T3), _ig(9, _T0), "wgrad2_kernel<9,4,2,2,2>"),
    # -- stride 2: the phase data-gradient tile (cfg 5) with narrow M (layer2.0.conv2, the stem) and narrow K
    ((2, 2, 17, 19, 40, 3, 2, 1, 1), _ig(9, _T1), _ig(9, _T5), WG9),
    ((2, 40, 17, 19, 2, 3, 2, 1, 1), _ig(9, _T0), _ig(9, _T5), WG9),
    ((2, 3, 18, 22, 24, 3, 2, 1, 1), _ig(9, _T0), _ig(9, _T5), WG9),                 # conv1.0 at gp70 (Cout != 64: no stem kernel)
    ((2, 3, 18, 22, 33, 3, 2, 1, 1), _ig(9, _T1), _ig(9, _T5), WG9),                 # ... at gp50
    ((2, 2, 16, 24, 40, 1, 2, 0, 1), _ig(1, _T1), _ig(1, _T5), WG1),                 # 1x1: one live phase, zeros in three
    ((2, 40, 15, 23, 1, 1, 2, 0, 1), _ig(1, _T0), _ig(1, _T5), WG1),
    # -- the tiles only a training-sized map reaches (train geometry: 193 x 193 and 97 x 97 maps, odd widths)
    ((2, 129, 129, 191, 2, 1, 1, 0, 1), _ig(1, _T0), _ig(1, _T4), WG1),              # layer2.0.conv1: dgrad 256 x 256, K = 2
    ((2, 1, 129, 191, 129, 1, 1, 0, 1), _ig(1, _T4), _ig(1, _T0), WG1),              # layer1.0.conv3: forward 256 x 256, K = 1
    ((2, 5, 129, 191, 129, 1, 1, 0, 1), _ig(1, _T4), _ig(1, _T0), WG1),              # layer3.1.conv3: K = 5
    ((2, 86, 129, 191, 5, 3, 1, 2, 2), _ig(9, _T0), _ig(9, _T2), WG9),               # layer3.1.conv2 at gp70: dgrad 128 x 256
    ((2, 129, 129, 191, 5, 3, 1, 2, 2), _ig(9, _T0), _ig(9, _T4), WG9),              # ... at gp50: dgrad 256 x 256, K = 5
    ((2, 2, 257, 381, 65, 3, 2, 1, 1), _ig(9, _T2), _ig(9, _T5), WG9),               # layer2.0.conv2: forward 128 x 256, K = 18
    # -- the LDS-DMA routes (full-size geometry: widths that are multiples of 4)
    ((2, 1, 128, 192, 40, 1, 1, 0, 1), D8_1, D8_1, WG1),                             # layer1.0.conv3
    ((2, 40, 128, 192, 2, 1, 1, 0, 1), D8_1, D8_1, WG1),                             # layer2.0.conv1, Cin <= 128
    ((2, 133, 128, 192, 2, 1, 1, 0, 1), D8_1, D8_1, WIDE1),                          # ... as pruned: the WIDE tile, 2 live rows
    ((2, 5, 128, 192, 256, 1, 1, 0, 1), DMA1P, D8_1, WG1),                           # layer3.1.conv3 (Cout a multiple of 256)
    ((2, 130, 16, 32, 1, 1, 1, 0, 1), _ig(1, _T0), _ig(1, _T3), WIDE1),              # the WIDE tile with Cout = 1: 255 dead rows
    ((2, 20, 128, 192, 1, 3, 1, 1, 1), D8_9, D8_9, WG9),                             # layer1.0.conv2, row-pitched
    ((2, 24, 128, 192, 5, 3, 1, 2, 2), D8_9, D8_9, WG9),                             # layer3.4.conv2 at gp70, row-pitched
    ((2, 130, 128, 192, 5, 3, 1, 2, 2), D8_9, D8_9, WIDE9),                          # ... at gp50: WIDE 3x3, pitched x
    ((2, 5, 128, 192, 24, 3, 1, 2, 2), D8_9, D8_9, WG9),                             # its mirror: K = 45, row-pitched
    ((2, 24, 128, 192, 5, 3, 1, 4, 4), D8_9, D8_9, WG9),                             # dilation 4: dense operands
    ((2, 5, 128, 192, 24, 3, 1, 4, 4), D8_9, D8_9, WG9),
    # -- the 1 x 1-map gemv: the ASPP image-pool conv with 5 filters, and its mirror
    ((2, 300, 1, 1, 5, 1, 1, 0, 1), GEMV, GEMV, GEMV),
    ((3, 5, 1, 1, 300, 1, 1, 0, 1), GEMV, GEMV, GEMV),
    # -- the statistics epilogue with a narrow reduction: 32 x 512 and 64 x 512 tiles that are all live
    ((2, 1, 16, 32, 32, 1, 1, 0, 1), _ig(1, _T0), _ig(1, _T0), WG1),
    ((2, 5, 16, 32, 64, 3, 1, 1, 1), _ig(9, _T1), _ig(9, _T0), WG9),
]
# -- 3, 7, 8 and 9 channels, the two sides of the 4-float and 8-channel granules, where the narrow side is the reduction:
#    K = 27 / 63 / 72 / 81 in the forward (and Nn in the weight gradient), K = 3 / 7 / 8 / 9 in the data gradient
for _c in (3, 7, 8, 9):
    NARROW.append(((2, _c, 9, 13, 19, 3, 1, 1, 1), _ig(9, _T0), _ig(9, _T0), WG9))
    NARROW.append(((2, 19, 9, 13, _c, 1, 1, 0, 1), _ig(1, _T0), _ig(1, _T0), WG1))

# rows whose x / dy the network keeps row-pitched (pitch_of): tests/_wp_cases.py describes dense operands only, so their
# kept copies are refreshed and replayed in tests/test_narrow_widths_gpu.py instead
NARROW_PITCH = {(2, 20, 128, 192, 1, 3, 1, 1, 1): 196, (2, 24, 128, 192, 5, 3, 1, 2, 2): 196,
                (2, 130, 128, 192, 5, 3, 1, 2, 2): 196, (2, 5, 128, 192, 24, 3, 1, 2, 2): 196}
# rows whose forward has the statistics epilogue (every other row must decline it)
STATS = {(2, 5, 128, 192, 256, 1, 1, 0, 1), (2, 1, 16, 32, 32, 1, 1, 0, 1), (2, 5, 16, 32, 64, 3, 1, 1, 1)}

# Routes the issue names that a narrow width cannot reach:
# * the stem kernels (conv_stem.hip) need Cout == 64; the pruned stem conv has 24 or 33 filters;
# * the fused / three-pass Winograd kernels: no narrow fixture layer routes there at either geometry (the cost model of
#   conv_igemm.hip wino_kind pads M to 64 rows at least and K to 16; the completeness test would name the layer);
# * the masked fan-in data gradient needs Cin % 256 == 0 and the persistent 1x1 kernel (dcfp_conv2d_dgrad_fanin_supported):
#   a block behind a narrow layer takes the plain accumulate form.


def tolerance(case):
    """The forward bound of tests/test_conv_random_gpu.py (relative L2 against fp64); dgrad uses max(tol, 1e-5), the
    weight gradient 2e-5."""
    K = case[1] * case[5] * case[5]
    return 3e-6 * max(1.0, math.sqrt(K) / 8)


# ------------------------------------------------------------------ the judges
def chan_norms(t, dim):
    """Per-index L2 norms of tensor `t` along `dim`."""
    dims = [i for i in range(t.dim()) if i != dim]
    return t.pow(2).sum(dims).sqrt()


def per_channel(got, ref64, ref32, dim, bound, min_elems=1):
    """got against the fp64 result per index of `dim` (relative L2 of each channel): -> (worst err / project bound,
    worst err / the bound it is held to - the larger of the project bound and 3 x ATen's fp32 error ref32 on the SAME
    channel -, ATen's fp32 error on that channel).  min_elems: channels with fewer elements are left out (a channel of
    one element is a single sum, whose relative error is its condition number times the arithmetic's)."""
    import torch
    got = got.detach().double().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), (got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all())
    if ref64.numel() // ref64.shape[dim] < min_elems:
        return 0.0, 0.0, 0.0
    den = chan_norms(ref64, dim).clamp_min(1e-300)
    err = chan_norms(got - ref64, dim) / den
    e32 = chan_norms(ref32.double() - ref64, dim) / den
    held = torch.maximum(torch.full_like(e32, bound), 3.0 * e32)
    k = int((err / held).argmax())
    return float((err / bound).max()), float((err / held).max()), float(e32[k])


# ReLU-mask flips (an element whose mask differs from fp64's, licensed by _node_ref.masks_honest only where the
# pre-activation lies within 1e-4 rms of zero).  The share the existing node tests see: 14 of the 56 623 104 mask elements
# of tests/test_fused_nodes_gpu.py's c512 chain, 0 in its eight other cases (profiles/narrow_widths_parity.txt).  Flips are
# rare independent events, so a case with `total` mask elements that flips at that rate has a Poisson count of mean
# FLIP_RATE * total; it "stays at the share" if its count is not above the 99.9 % quantile of that distribution - 0 for
# masks under 4000 elements, 6 for 4.7 million, 16 for 26 million.  More than that is a finding.
FLIP_RATE = 14 / 56623104


def flip_allowance(total):
    lam = FLIP_RATE * total
    k, term = 0, math.exp(-lam)
    cdf = term
    while cdf < 0.999:
        k += 1
        term *= lam / k
        cdf += term
    return k
