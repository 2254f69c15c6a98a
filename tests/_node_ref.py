"""What tests/test_fused_nodes_gpu.py compares ops.BottleneckFn and ops.AsppFn with: the two module trees written as
plain ATen composites (the leaf nn.Conv2d / nn.BatchNorm2d modules called directly - F.conv2d and F.batch_norm - and a
multiplication by a ReLU mask; mean and broadcast for the image-pool branch).  Run on a `.double()` copy of the module
they are the truth, on an fp32 copy the yardstick `e32` of the bounds: the error ATen's own fp32 arithmetic makes on
the same quantity, with the same masks.

Every ReLU mask is an argument: a pre-activation within fp32 rounding of zero may fall on either side, and one such
element moves a gradient by about 1 / sqrt(numel).  The test takes the masks from the HIP run and `masks_honest`
bounds how far from zero an element may be where the kernel and fp64 disagree about its sign."""
import math

import torch
import torch.nn as nn


def rel(a, b):
    """Relative L2 distance of a from b, in fp64 on b's device."""
    b = b.detach().double()
    a = a.detach().double().to(b.device)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ------------------------------------------------------------------ module preparation
def cut_conv(conv, cout=None, cin=None):
    """Keep the first cout filters / cin input channels (what the pruner leaves behind, as test_psp_gpu cuts its stages)."""
    w = conv.weight.data
    if cout is not None:
        w = w[:cout]
    if cin is not None:
        w = w[:, :cin]
    conv.weight = nn.Parameter(w.clone())
    conv.out_channels, conv.in_channels = w.shape[0], w.shape[1]


def cut_bn(bn, n):
    bn.weight = nn.Parameter(bn.weight.data[:n].clone())
    bn.bias = nn.Parameter(bn.bias.data[:n].clone())
    bn.running_mean = bn.running_mean[:n].clone()
    bn.running_var = bn.running_var[:n].clone()
    bn.num_features = n


def cut_bottleneck(blk, c1, c2, cout):
    """conv1 -> c1 channels, conv2 -> c2, the block output (conv3, bn3 and the downsample pair) -> cout."""
    cut_conv(blk.conv1, cout=c1); cut_bn(blk.bn1, c1)
    cut_conv(blk.conv2, cout=c2, cin=c1); cut_bn(blk.bn2, c2)
    cut_conv(blk.conv3, cout=cout, cin=c2); cut_bn(blk.bn3, cout)
    if blk.downsample is not None:
        cut_conv(blk.downsample[0], cout=cout); cut_bn(blk.downsample[1], cout)


def aspp_parts(m):
    """[(conv, bn)] of the five branches in concat order."""
    pool = list(m.global_avg_pool.children())
    return [(b.atrous_conv, b.bn) for b in (m.aspp1, m.aspp2, m.aspp3, m.aspp4)] + [(pool[1], pool[2])]


def cut_aspp(m, widths):
    for (conv, bn), w in zip(aspp_parts(m), widths):
        cut_conv(conv, cout=w); cut_bn(bn, w)


def seed(mod, g):
    """Seeded non-trivial values for every conv weight (He scale: activations stay O(1) through a chain), gamma, beta,
    running mean and running var."""
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / m.weight[0].numel()))
            elif isinstance(m, nn.BatchNorm2d):
                n = m.weight.shape[0]
                m.weight.copy_(1.0 + 0.2 * torch.randn(n, generator=g))
                m.bias.copy_(0.1 * torch.randn(n, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(n, generator=g))
                m.running_var.copy_(1.0 + 0.3 * torch.rand(n, generator=g))
    return mod


# ------------------------------------------------------------------ the composites
def bottleneck_composite(blk, x, masks):
    """networks.backbone.resnet.Bottleneck on ATen, in x's dtype.  masks = (y1 > 0, y2 > 0, out > 0).
    -> (out, stage values c1 c2 c3 cd, pre-activations of the three ReLUs)."""
    m1, m2, m3 = (m.to(x.dtype) for m in masks)
    c1 = blk.conv1(x)
    p1 = blk.bn1(c1)
    c2 = blk.conv2(p1 * m1)
    p2 = blk.bn2(c2)
    c3 = blk.conv3(p2 * m2)
    if blk.downsample is not None:
        cd = blk.downsample[0](x)
        res = blk.downsample[1](cd)
    else:
        cd, res = None, x
    p3 = blk.bn3(c3) + res
    return p3 * m3, (c1, c2, c3, cd), (p1, p2, p3)


def chain_composite(blocks, x, masks):
    """Blocks whose output feeds the next.  -> (outputs of every block, stages, pre-activations), per block."""
    outs, stages, pres = [], [], []
    for blk, mk in zip(blocks, masks):
        x, st, pr = bottleneck_composite(blk, x, mk)
        outs.append(x); stages.append(st); pres.append(pr)
    return outs, stages, pres


def aspp_composite(m, x, mask):
    """networks.tools.aspp.ASPP's five branches and their concat on ATen.  mask = (cat > 0) of the HIP run.
    -> (cat, pre-activations per branch; the pool branch's is N x C x 1 x 1)."""
    N, _, H, W = x.shape
    parts = aspp_parts(m)
    outs, pres, o = [], [], 0
    for k, (conv, bn) in enumerate(parts):
        w = conv.weight.shape[0]
        mk = mask[:, o:o + w].to(x.dtype)
        if k < 4:
            p = bn(conv(x))
            outs.append(p * mk)
        else:
            p = bn(conv(x.mean(dim=(2, 3), keepdim=True)))
            outs.append((p * mk[:, :, :1, :1]).expand(N, w, H, W))
        pres.append(p)
        o += w
    return torch.cat(outs, 1), pres


def masks_honest(masks, pres):
    """The masks taken from the kernels must not hide a wrong mask: wherever one differs from fp64's own (pre > 0),
    that pre-activation lies within 1e-4 rms of zero (10x the forward bound).  -> number of such elements."""
    flipped = 0
    for i, (m, p) in enumerate(zip(masks, pres)):
        p = p.detach()
        diff = m != (p > 0)
        n = int(diff.sum())
        if n:
            rms = float(p.pow(2).mean().sqrt())
            worst = float(p[diff].abs().max())
            assert worst <= 1e-4 * rms, (i, n, worst, rms)
        flipped += n
    return flipped


# ------------------------------------------------------------------ the bounds
def bound(case, what, got, want, yard=None, floor=1e-5, widen=True):
    """got against the fp64 `want`: relative L2 <= max(floor, 3 * e32), e32 = the fp32 ATen composite's error on the
    same quantity (yard).  widen=False: the floor alone, e32 printed for the record."""
    e = rel(got, want)
    e32 = rel(yard, want) if yard is not None else 0.0
    lim = max(floor, 3.0 * e32) if widen else floor
    print(f"NODE_FIG {case} {what} hip={e:.3e} aten32={e32:.3e} bound={lim:.1e}")
    assert e <= lim, (case, what, e, e32, lim)


def param_floor(name):
    """Conv weights and gamma 1e-4, beta 1e-5 (the bounds of the DecoderConcatFn and PyramidPoolingFn tests)."""
    return 1e-5 if name.endswith(".bias") else 1e-4


def check_param_grads(case, hip, ref, ref32):
    for (name, p), (_, q), (_, r) in zip(hip.named_parameters(), ref.named_parameters(), ref32.named_parameters()):
        assert p.grad is not None and q.grad is not None, (case, name)
        bound(case, "d_" + name, p.grad, q.grad, r.grad, param_floor(name))


def check_buffers(case, hip, ref):
    for (name, b), (_, q) in zip(hip.named_buffers(), ref.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(q), (case, name, int(b), int(q))
        else:
            bound(case, name, b, q)
