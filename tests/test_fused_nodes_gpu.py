"""GPU: the two fused training nodes of DeepLabv3, ops.BottleneckFn and ops.AsppFn, each on its own against an fp64
ATen composite (tests/_node_ref.py), at the smallest shapes that still reach each of their paths.

* Bottleneck, small and ragged (direct kernels, no fan-in): identity and downsample shortcuts, stride 2 at odd sizes,
  dilation 2 and 4, distinct pruned widths; train and eval;
* Bottleneck chains at shapes where the fan-in dgrad applies - 3 x (512, 128, dilation 1) at 2x512x96x128 (row-pitched
  y1 / d_c2, fused Winograd conv2), 2 x (2048, 512, dilation 4) at 2x2048x48x64 (three-pass Winograd, fused Winograd
  weight gradient) and 2 x (2048, 512, dilation 2) at 2x2048x64x64 (the weight gradient from the kept input transform) -
  in three modes against ONE fp64 result: defaults, the fan-in epilogue's bn3 sums forced on, the materialised residual
  gradient; a second consumer of block 0's output, a non-contiguous output gradient, two forwards before two backwards;
* no input gradient wanted; gradient accumulation through the arena (tokens 1 and 2 of arena.grad_target) and through
  autograd (token 0);
* ASPP at 4x200x17x33 with widths [131, 77, 256, 19, 64] (4-byte-aligned slices, dilation 18 > H) and at 2x2048x48x64
  with widths [200, 131, 256, 77, 64] (persistent 1x1 dgrad, fused / three-pass Winograd, LDS-DMA 3x3 dgrad in its
  mixed-alignment form, gemv pool branch); no input gradient; arena accumulation;
* ops.fork, ops.dropout2d and ops.add exactly.

Bounds (relative L2 against fp64; e32 = the fp32 ATen composite's error on the same quantity, same masks): output 1e-5,
input gradient max(1e-5, 3 e32), conv-weight and gamma gradients max(1e-4, 3 e32), beta gradient max(1e-5, 3 e32),
running statistics 1e-5, num_batches_tracked equal; c1 / c2 / c3 / cd of every Bottleneck 1e-5.  Every figure is printed
("NODE_FIG ...") before it is asserted."""
import copy
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import _node_ref as nr

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the nodes on HIP
def _bottleneck_fwd(hip, xh):
    """-> (outputs per block, masks per block, (c1, c2, c3, cd) per block) - read from the node before its backward."""
    from dcfp_amd.networks import _exec
    outs, masks, stages = [], [], []
    h = xh
    for blk in hip:
        h = _exec.bottleneck(blk, h)
        assert type(h.grad_fn).__name__ == "BottleneckFnBackward"
        _, c1, y1, c2, y2, c3, out, cd = h.grad_fn.saved_tensors[:8]     # as saved in BottleneckFn.forward
        out = out if out is not None else h.detach()                     # (not saved where the 1-bit mask stands in for it)
        masks.append((y1 > 0, y2 > 0, out > 0))
        stages.append(tuple(t.clone() if t is not None else None for t in (c1, c2, c3, cd)))
        outs.append(h)
    return outs, masks, stages


def _aspp_node(m, x):
    """ops.aspp_branches with the cfg and tensors ASPP.forward builds (for an input that does not require grad)."""
    from dcfp_amd import ops
    from dcfp_amd.networks import _exec
    parts = nr.aspp_parts(m)
    tensors, bns = [], []
    for conv, bn in parts:
        tensors += [conv.weight, bn.weight, bn.bias]
        bns.append(_exec._bn_args(bn))
    cfg = {"convs": [(c.padding[0], c.dilation[0]) for c, _ in parts[:4]], "bn": bns}
    return ops.aspp_branches(x, cfg, tensors)


def _aspp_fwd(hip, xh):
    cat = hip[0](xh) if xh.requires_grad else _aspp_node(hip[0], xh)
    assert type(cat.grad_fn).__name__ == "AsppFnBackward"
    return [cat], cat.detach() > 0, None


def _chain_composite(mods, x, masks):
    outs, stages, pres = nr.chain_composite(mods, x, masks)
    return outs, stages, [p for pr in pres for p in pr], [m for mk in masks for m in mk]


def _aspp_composite(mods, x, mask):
    cat, pres = nr.aspp_composite(mods[0], x, mask)
    flat, o = [], 0
    for k, (conv, _) in enumerate(nr.aspp_parts(mods[0])):
        w = conv.weight.shape[0]
        flat.append(mask[:, o:o + w] if k < 4 else mask[:, o:o + w, :1, :1])
        o += w
    return [cat], None, pres, flat


KINDS = {"bottleneck": (_bottleneck_fwd, _chain_composite), "aspp": (_aspp_fwd, _aspp_composite)}


# ------------------------------------------------------------------ the reference
class Reference:
    """The fp64 and fp32 copies of a list of modules, and the composite run on both.  The copies' parameters collect
    the gradients (several runs accumulate, as autograd does), their buffers the running statistics."""

    def __init__(self, master, device, train, composite):
        self.m64 = [copy.deepcopy(b).double().to(device).train(train) for b in master]
        self.m32 = [copy.deepcopy(b).to(device).train(train) for b in master]
        self.device, self.composite = device, composite

    def run(self, x, grads, masks, need_dx=True, stages=None):
        """grads: [(index of the output it arrives at, gradient)].  -> (fp64 run, fp32 run): .out (the last output), .dx.
        stages: the HIP run's (c1, c2, c3, cd) per block, compared with fp64's here (<= 1e-5 each)."""
        res = []
        for dt, mods in ((torch.float64, self.m64), (torch.float32, self.m32)):
            xx = x.to(self.device, dt, copy=True).requires_grad_(need_dx)
            # (MIOpen off: fp32 takes the im2col + GEMM path fp64 takes, so the yardstick differs from the truth in precision alone)
            with torch.backends.cudnn.flags(enabled=False):
                outs, stg, pres, flat = self.composite(mods, xx, masks)
                if dt is torch.float64:
                    self.flipped = nr.masks_honest(flat, pres)
                    if stages is not None:
                        for k, (mine, want) in enumerate(zip(stages, stg)):
                            for name, a, b in zip(("c1", "c2", "c3", "cd"), mine, want):
                                assert (a is None) == (b is None)
                                if a is not None:
                                    nr.bound(f"stage.b{k}", name, a, b)
                torch.autograd.backward([outs[k] for k, _ in grads], [g.to(self.device, dt) for _, g in grads])
            res.append(SimpleNamespace(out=outs[-1].detach(), dx=xx.grad))
            del outs, stg, pres, flat
        return res


def _compare(case, hip, outs, dx, ref, r64, r32, buffers=True):
    nr.bound(case, "out", outs[-1], r64.out, r32.out, widen=False)
    if dx is not None:
        nr.bound(case, "dx", dx, r64.dx, r32.dx)
    for k, (h, a, b) in enumerate(zip(hip, ref.m64, ref.m32)):
        nr.check_param_grads(f"{case}.b{k}", h, a, b)
        if buffers:
            nr.check_buffers(f"{case}.b{k}", h, a)


def _run(case, kind, device, master, x, dy, train, need_dx=True, cached=None, extra=None, wide=False):
    """One forward and backward of the HIP node(s) against the composite.  cached: (ref, r64, r32, masks) of an earlier
    run of the same modules and input.  extra: (block index, gradient) - a second consumer of that block's output.
    wide: hand the output gradient over as a channel slice of a wider tensor."""
    from dcfp_amd import ops
    fwd, composite = KINDS[kind]
    hip = [copy.deepcopy(b).to(device).train(train) for b in master]
    before = {(k, n): b.clone() for k, h in enumerate(hip) for n, b in h.named_buffers()} if not train else None
    xh = x.to(device, copy=True).requires_grad_(need_dx)
    outs, masks, stages = fwd(hip, xh)
    grads = [(len(outs) - 1, dy)] + ([extra] if extra is not None else [])
    if cached is None:
        ref = Reference(master, device, train, composite)
        r64, r32 = ref.run(x, grads, masks, need_dx, stages)
    else:
        ref, r64, r32, masks0 = cached
        flat0 = [m for mk in masks0 for m in mk] if kind == "bottleneck" else [masks0]
        flat1 = [m for mk in masks for m in mk] if kind == "bottleneck" else [masks]
        assert all(torch.equal(a, b) for a, b in zip(flat0, flat1))       # the forward is deterministic
    dyh = dy.to(device)
    if wide:
        buf = torch.randn(dy.shape[0], dy.shape[1] + 8, *dy.shape[2:], device=device)
        buf[:, 3:3 + dy.shape[1]] = dyh
        dyh = buf[:, 3:3 + dy.shape[1]]
        assert not dyh.is_contiguous()
    ops.FANIN_RED_USED[0] = 0
    torch.autograd.backward([outs[k] for k, _ in grads], [dyh] + [g.to(device) for _, g in grads[1:]])
    torch.cuda.synchronize()
    used = ops.FANIN_RED_USED[0]
    _compare(case, hip, outs, xh.grad if need_dx else None, ref, r64, r32)
    if not train:                    # eval: running statistics and counters are constants
        for k, h in enumerate(hip):
            for n, b in h.named_buffers():
                assert torch.equal(b, before[(k, n)]), (k, n)
    return SimpleNamespace(ref=ref, r64=r64, r32=r32, masks=masks, used=used, hip=hip)


def _inputs(seed, xshape, yshape):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(xshape, generator=g)), torch.randn(yshape, generator=g)


# ------------------------------------------------------------------ routing (host side)
def _names(xs, ws, stride, pad, dil, xp=0, dp=0):
    from dcfp_amd import _lib, ops
    d = ops._desc(tuple(xs), tuple(ws), stride, pad, dil, xp, dp)
    return [ops.conv_kernel_name(d, k) for k in (_lib.CONV_FWD, _lib.CONV_DGRAD, _lib.CONV_WGRAD)]


def _block_routing(blk, xshape):
    """What a Bottleneck reaches on an input of xshape: y1's row pitch, the kernels of conv1 / conv2, the size of conv2's
    kept Winograd input transform (0: its weight gradient transforms for itself), whether conv1's dgrad has the fan-in
    form and its bn3-sum slots."""
    import ctypes
    from dcfp_amd import _lib, ops
    N, _, H, W = xshape
    w1, w2 = blk.conv1.weight, blk.conv2.weight
    stride, dil = blk.conv2.stride[0], blk.conv2.dilation[0]
    y1 = (N, w1.shape[0], H, W)
    pitch = ops.conv_pitch(y1, tuple(w2.shape), stride, dil, dil)
    d2 = ops._desc(y1, tuple(w2.shape), stride, dil, dil, pitch, 0)
    return SimpleNamespace(pitch=pitch, conv1=_names(xshape, w1.shape, 1, 0, 1),
                           xform=int(_lib.lib().dcfp_conv2d_xform_bytes(ctypes.byref(d2))),
                           conv2=_names(y1, w2.shape, stride, dil, dil, pitch, pitch),
                           fanin=ops.conv2d_dgrad_fanin_ok(None, w1, tuple(xshape)),
                           slots=ops.conv2d_dgrad_fanin_red_slots(w1, tuple(xshape)))


def _direct(names):
    return all(n.startswith(("igemm2_kernel<", "wgrad2_kernel<")) for n in names)


# ------------------------------------------------------------------ Bottleneck: small and ragged
def _block(inplanes, planes, stride=1, dil=1, ds=False, cut=None, seed=0):
    from dcfp_amd.networks.backbone.resnet import Bottleneck
    down = None
    if ds:
        down = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False),
                             nn.BatchNorm2d(planes * 4))
    blk = Bottleneck(inplanes, planes, stride, dil, down)
    if cut is not None:
        nr.cut_bottleneck(blk, *cut)
    return nr.seed(blk, torch.Generator().manual_seed(100 + seed))


# name: (N, inplanes, planes, H, W, stride, dil, downsample, pruned widths (conv1, conv2, block output))
SMALL = {
    "identity": (2, 148, 37, 17, 23, 1, 1, False, None),      # accumulate-dgrad into the residual gradient
    "downsample": (2, 96, 37, 17, 23, 1, 1, True, None),
    "stride2_odd": (2, 150, 45, 33, 41, 2, 1, True, None),    # odd sizes under stride 2: phase dgrad
    "dilation2": (3, 200, 50, 19, 21, 1, 2, True, None),
    "dilation4": (2, 148, 37, 19, 21, 1, 4, False, None),
    "pruned_widths": (2, 148, 45, 17, 23, 1, 1, False, (37, 45, 148)),
}


def _small(name):
    N, cin, planes, H, W, stride, dil, ds, cut = SMALL[name]
    blk = _block(cin, planes, stride, dil, ds, cut, seed=sorted(SMALL).index(name))
    cout = blk.conv3.weight.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    return blk, (N, cin, H, W), (N, cout, Ho, Wo)


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("name", list(SMALL))
def test_bottleneck_small_vs_fp64_composite(cuda, name, train):
    blk, xs, ys = _small(name)
    rt = _block_routing(blk, xs)
    # the ragged direct kernels, dense operands, no fan-in: conv1's dgrad accumulates into the residual gradient
    assert rt.pitch == 0 and not rt.fanin and _direct(rt.conv1 + rt.conv2), rt
    if name == "pruned_widths":
        assert [blk.conv1.weight.shape[0], blk.conv2.weight.shape[0], blk.conv3.weight.shape[0]] == [37, 45, 148]
    x, dy = _inputs(11, xs, ys)
    _run(f"{name}.{'train' if train else 'eval'}", "bottleneck", cuda, [blk], x, dy, train)


# ------------------------------------------------------------------ Bottleneck: the fan-in shapes
# name: (blocks, inplanes, planes, dilation, input shape)
CHAINS = {"c512": (3, 512, 128, 1, (2, 512, 96, 128)), "c2048": (2, 2048, 512, 4, (2, 2048, 48, 64)),
          "c2048_kept": (2, 2048, 512, 2, (2, 2048, 64, 64))}
_FUSED, _THREE_PASS = "winograd_f2x2_3x3 fused", "winograd_f2x2_3x3 (igemm2_dma1p_kernel<false,true>)"
_WG_FUSED, _WG_KEPT = "winograd_f2x2_3x3 wgrad fused", "winograd_f2x2_3x3 wgrad (wgrad_dma_kernel<"
# name: (row pitch of y1 / d_c2, conv2's forward, dgrad and wgrad kernels, weight gradient from the kept input transform)
CHAIN_ROUTING = {"c512": (132, (_FUSED, _FUSED, _WG_FUSED), False), "c2048": (0, (_THREE_PASS, _THREE_PASS, _WG_FUSED), False),
                 "c2048_kept": (0, (_THREE_PASS, _THREE_PASS, _WG_KEPT), True)}
_CHAIN_CACHE = {}


@functools.lru_cache(maxsize=None)
def _chain(name):
    """(seeded CPU blocks, input, output gradient): only ever copied"""
    n, cin, planes, dil, xs = CHAINS[name]
    master = [_block(cin, planes, 1, dil, seed=10 * len(name) + k) for k in range(n)]
    x, dy = _inputs(21, xs, xs)
    return master, x, dy


def _chain_routing(name):
    """Asserts what the chain relies on (before a test switches anything off)."""
    master, x, _ = _chain(name)
    N, _, H, W = x.shape
    rt = _block_routing(master[0], tuple(x.shape))
    pitch, conv2, kept = CHAIN_ROUTING[name]
    assert rt.fanin and rt.conv1[1] == "igemm2_dma1p_kernel", rt               # persistent 1x1 dgrad with the fan-in forms
    assert rt.slots == N * H * W // 128 and rt.pitch == pitch, rt
    assert all(n.startswith(want) for n, want in zip(rt.conv2, conv2)), rt
    assert (rt.xform > 0) == kept, rt
    return rt


def _run_chain(name, cuda, mode, **kw):
    """The chain against its one fp64 result (computed by whichever test comes first)."""
    master, x, dy = _chain(name)
    cached = _CHAIN_CACHE.get(name)
    r = _run(f"{name}.{mode}", "bottleneck", cuda, master, x, dy, True, cached=cached, **kw)
    if cached is None:
        _CHAIN_CACHE[name] = (r.ref, r.r64, r.r32, r.masks)
    return r


@pytest.mark.parametrize("mode", ["default", "bn3_sums", "materialised"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_bottleneck_chain_vs_fp64_composite(cuda, monkeypatch, name, mode):
    from dcfp_amd import ops
    _chain_routing(name)
    blocks = CHAINS[name][0]
    if mode == "bn3_sums":
        monkeypatch.setattr(ops, "FANIN_BN_SUMS_ALWAYS", True)
    elif mode == "materialised":
        monkeypatch.setattr(ops, "MASKED_FANIN", False)      # d_res written, conv1's dgrad accumulates at the large tile
    kept = []
    real = ops.conv2d_wgrad
    monkeypatch.setattr(ops, "conv2d_wgrad", lambda *a, **k: (kept.append(k.get("xform") is not None), real(*a, **k))[1])
    r = _run_chain(name, cuda, mode)
    assert sum(kept) == (blocks if CHAIN_ROUTING[name][2] else 0), kept      # conv2's weight gradient took the kept transform
    # default: the fused BatchNorm backward makes the epilogue sums unnecessary; forced on, every block but the last
    # takes bn3's sums from the next block's fan-in
    assert r.used == (blocks - 1 if mode == "bn3_sums" else 0), r.used


def test_chain_second_consumer_sends_bn3_back_to_its_own_reduce(cuda, monkeypatch):
    """Block 0's output feeds block 1 AND a second term of the loss: autograd sums the two gradients, the partial sums
    block 1's fan-in left are of something else, and block 0 must reduce for itself."""
    from dcfp_amd import ops
    _chain_routing("c512")
    monkeypatch.setattr(ops, "FANIN_BN_SUMS_ALWAYS", True)
    master, x, dy = _chain("c512")
    r = torch.randn(x.shape, generator=torch.Generator().manual_seed(22))
    res = _run("c512.second_consumer", "bottleneck", cuda, master, x, dy, True, extra=(0, r))
    assert res.used == CHAINS["c512"][0] - 2, res.used       # one lower than the plain chain


def test_chain_noncontiguous_output_gradient(cuda):
    """The output gradient as a channel-slice view of a wider tensor: the last block takes no fan-in."""
    _chain_routing("c512")
    _run_chain("c512", cuda, "noncontiguous_dout", wide=True)


def test_chain_two_forwards_then_two_backwards(cuda, monkeypatch):
    """A second forward of the same blocks while the first graph is alive gets fresh pitched buffers; both backwards
    must then be right (the first graph's y1 may not have been overwritten)."""
    from dcfp_amd import ops
    _chain_routing("c512")
    master, xa, dya = _chain("c512")
    xb, dyb = _inputs(23, xa.shape, xa.shape)
    hip = [copy.deepcopy(b).to(cuda).train() for b in master]
    calls = []
    real = ops.new_pitched
    monkeypatch.setattr(ops, "new_pitched", lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1])
    runs = []
    for x in (xa, xb):
        xh = x.to(cuda, copy=True).requires_grad_(True)
        runs.append((xh,) + _bottleneck_fwd(hip, xh))
    assert len(calls) == 2 * len(hip), calls                  # every block: its persistent buffer, then a fresh one
    for tag, x, dy, (xh, outs, masks, stages) in (("a", xa, dya, runs[0]), ("b", xb, dyb, runs[1])):
        for h in hip:
            for p in h.parameters():
                p.grad = None
        outs[-1].backward(dy.to(cuda))
        torch.cuda.synchronize()
        ref = Reference(master, cuda, True, _chain_composite)
        r64, r32 = ref.run(x, [(len(outs) - 1, dy)], masks, True, stages)
        # (the blocks' running statistics have seen two batches, each reference one: not compared here)
        _compare(f"c512.two_forwards.{tag}", hip, outs, xh.grad, ref, r64, r32, buffers=False)


# name: (block, input shape)
def _single(name):
    if name == "small_identity":
        return _small("identity")[:2]
    if name == "small_downsample":
        return _small("downsample")[:2]
    ds = name == "fanin_downsample"
    return _block(512, 128, 1, 1, ds=ds, seed=40 + ds), (2, 512, 96, 128)


@pytest.mark.parametrize("name", ["small_identity", "small_downsample", "fanin_identity", "fanin_downsample"])
def test_bottleneck_without_input_gradient(cuda, name):
    blk, xs = _single(name)
    if name.startswith("fanin"):
        rt = _block_routing(blk, xs)
        assert rt.fanin and rt.pitch == 132, rt
    x, dy = _inputs(31, xs, (xs[0], blk.conv3.weight.shape[0]) + tuple(xs[2:]))
    _run(f"no_dx.{name}", "bottleneck", cuda, [blk], x, dy, True, need_dx=False)


def _accumulate(case, kind, cuda, monkeypatch, master, xs, ys, use_arena):
    """Forward and backward twice on different inputs without zeroing, against the fp64 sum of both passes; then the
    same again after an in-place zero.  With an arena the first pass writes the gradient views (token 1 of
    arena.grad_target), every later one a temporary that add_into adds (token 2); without, autograd accumulates (0)."""
    from dcfp_amd import arena
    fwd, composite = KINDS[kind]
    hip = [copy.deepcopy(b).to(cuda).train() for b in master]
    params = [p for h in hip for p in h.parameters()]
    ar = arena.ParamArena.of(params) if use_arena else None
    tokens = []
    real = arena.grad_target
    monkeypatch.setattr(arena, "grad_target", lambda p: (lambda r: (tokens.append(r[1]), r)[1])(real(p)))
    ref = Reference(master, cuda, True, composite)
    inputs = [_inputs(41 + k, xs, ys) for k in range(2)]
    seen = []
    for rnd in range(2):
        for k, (x, dy) in enumerate(inputs):
            del tokens[:]
            xh = x.to(cuda, copy=True).requires_grad_(True)
            outs, masks, stages = fwd(hip, xh)
            outs[-1].backward(dy.to(cuda))
            torch.cuda.synchronize()
            want = ({0} if not use_arena else {1} if (rnd == 0 and k == 0) else {2})
            assert set(tokens) == want and len(tokens) >= len(params), (rnd, k, sorted(set(tokens)), len(tokens))
            if rnd == 0:
                r64, r32 = ref.run(x, [(len(outs) - 1, dy)], masks, True, stages)
                seen.append((r64, r32, masks))
            r64, r32, masks0 = seen[k]
            nr.bound(f"{case}.round{rnd}.pass{k}", "out", outs[-1], r64.out, r32.out, widen=False)
            nr.bound(f"{case}.round{rnd}.pass{k}", "dx", xh.grad, r64.dx, r32.dx)
        # the sum of both passes (the references' .grad accumulated the same two)
        for j, (h, a, b) in enumerate(zip(hip, ref.m64, ref.m32)):
            nr.check_param_grads(f"{case}.round{rnd}.sum.b{j}", h, a, b)
            if rnd == 0:
                nr.check_buffers(f"{case}.b{j}", h, a)
        if use_arena:
            ar.zero_grad(set_to_none=False)                    # one fill; the views stay attached: token 2 from now on
            assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in params)
        else:
            for p in params:
                p.grad.zero_()


@pytest.mark.parametrize("use_arena", [True, False], ids=["arena", "autograd"])
@pytest.mark.parametrize("name", ["small_identity", "fanin_identity"])
def test_bottleneck_gradient_accumulation(cuda, monkeypatch, name, use_arena):
    blk, xs = _single(name)
    _accumulate(f"accumulate.{name}.{'arena' if use_arena else 'autograd'}", "bottleneck", cuda, monkeypatch, [blk], xs, xs,
                use_arena)


# ------------------------------------------------------------------ ASPP
# name: (input shape, widths of the five branches)
ASPP_CASES = {"ragged": ((4, 200, 17, 33), [131, 77, 256, 19, 64]), "large": ((2, 2048, 48, 64), [200, 131, 256, 77, 64])}
DILATIONS = (1, 6, 12, 18)


@functools.lru_cache(maxsize=None)
def _aspp(name):
    from dcfp_amd.networks.tools.aspp import ASPP
    xs, widths = ASPP_CASES[name]
    m = ASPP(16, True, inplanes=xs[1], outplanes=None)
    nr.cut_aspp(m, widths)
    assert [c.dilation[0] for c, _ in nr.aspp_parts(m)[:4]] == list(DILATIONS)
    return nr.seed(m, torch.Generator().manual_seed(7 + len(name))), xs, (xs[0], sum(widths)) + tuple(xs[2:])


def _aspp_routing(name):
    from dcfp_amd import _lib, ops
    xs, widths = ASPP_CASES[name]
    N, cin, H, W = xs
    br = [_names(xs, (widths[0], cin, 1, 1), 1, 0, 1)]
    br += [_names(xs, (widths[k], cin, 3, 3), 1, DILATIONS[k], DILATIONS[k]) for k in (1, 2, 3)]
    pool = _names((N, cin, 1, 1), (widths[4], cin, 1, 1), 1, 0, 1)
    assert all(n == "gemv_1x1_map_kernel" for n in pool), pool
    if name == "ragged":
        assert all(_direct(b) for b in br), br
        assert all((sum(widths[:k]) * H * W) % 4 for k in (1, 4, 5)), widths     # slice bases (and images) at odd float offsets
        assert DILATIONS[3] > H and DILATIONS[3] < W                           # dead kernel rows, live columns
    else:
        assert br[0][1] == "igemm2_dma1p_kernel", br[0]                        # persistent 1x1 dgrad
        for k in (1, 2):
            assert br[k][0].startswith("winograd_f2x2_3x3 fused"), br[k]
            assert br[k][1] == "winograd_f2x2_3x3 (igemm2_dma1p_kernel<false,true>)", br[k]
            assert br[k][2].startswith("winograd_f2x2_3x3 wgrad fused"), br[k]
            d = ops._desc(xs, (widths[k], cin, 3, 3), 1, DILATIONS[k], DILATIONS[k])
            assert abs(ops.conv_executed_fraction(d, _lib.CONV_FWD) - 0.5) < 1e-6  # dead kernel rows skipped
        assert br[3][0].startswith("igemm2_kernel<9") and br[3][1] == "igemm2_dma_kernel<9,true>", br[3]
        assert br[3][2].startswith("winograd_f2x2_3x3 wgrad fused"), br[3]
    return br


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("name", list(ASPP_CASES))
def test_aspp_vs_fp64_composite(cuda, name, train):
    """(with N = 2 the pool branch's BatchNorm backward is ill-conditioned: the e32 term of the bounds is for that)"""
    _aspp_routing(name)
    m, xs, ys = _aspp(name)
    x, dy = _inputs(51, xs, ys)
    _run(f"aspp.{name}.{'train' if train else 'eval'}", "aspp", cuda, [m], x, dy, train)


def test_aspp_without_input_gradient(cuda):
    m, xs, ys = _aspp("ragged")
    x, dy = _inputs(52, xs, ys)
    _run("aspp.ragged.no_dx", "aspp", cuda, [m], x, dy, True, need_dx=False)


def test_aspp_gradient_accumulation_through_the_arena(cuda, monkeypatch):
    m, xs, ys = _aspp("ragged")
    _accumulate("aspp.ragged.accumulate", "aspp", cuda, monkeypatch, [m], xs, ys, True)


# ------------------------------------------------------------------ the small exact ops of these graphs
def test_fork_sums_two_gradients_and_passes_one_through(cuda, monkeypatch):
    from dcfp_amd import ops
    g = torch.Generator().manual_seed(61)
    adds = []
    real = ops.add
    monkeypatch.setattr(ops, "add", lambda a, b: (adds.append(1), real(a, b))[1])
    ga, gb = torch.randn(2, 5, 7, 9, generator=g).to(cuda), torch.randn(2, 5, 7, 9, generator=g).to(cuda)
    x = torch.randn(2, 5, 7, 9, generator=g).to(cuda).requires_grad_(True)
    a, b = ops.fork(x)
    assert torch.equal(a, x) and torch.equal(b, x)
    torch.autograd.backward([a, b], [ga, gb])
    assert torch.equal(x.grad, ga + gb) and len(adds) == 1
    for side in (0, 1):                                        # one tap unused: its None is not materialised, no add
        x1 = x.detach().clone().requires_grad_(True)
        ops.fork(x1)[side].backward(ga)
        assert torch.equal(x1.grad, ga)
    assert len(adds) == 1
    y = x.detach()
    assert all(t is y for t in ops.fork(y))                    # nothing to fork without grad


@pytest.mark.parametrize("shape", [(2, 19, 5, 7), (2, 256, 33, 65)])
def test_dropout2d_fixed_mask_exact(cuda, shape):
    from dcfp_amd import ops
    g = torch.Generator().manual_seed(62)
    p = 0.25
    x = torch.randn(shape, generator=g).to(cuda).requires_grad_(True)
    dy = torch.randn(shape, generator=g).to(cuda)
    mask = (torch.rand(shape[:2], generator=g) >= p).float() / (1.0 - p)
    assert 0 < int((mask == 0).sum()) < mask.numel()
    y = ops.dropout2d(x, p, True, fixed_mask=mask)
    y.backward(dy)
    m = mask.to(cuda)[:, :, None, None]
    assert torch.equal(y.detach(), x.detach() * m)
    assert torch.equal(x.grad, dy * m)
    assert ops.dropout2d(x, 0.0, True, fixed_mask=mask) is x
    assert ops.dropout2d(x, p, False, fixed_mask=mask) is x


@pytest.mark.parametrize("shape", [(3, 5, 7, 11), (1, 1, 1, 1), (2, 3, 33, 65)])
def test_add_exact_at_sizes_off_the_vector_width(cuda, shape):
    from dcfp_amd import ops
    g = torch.Generator().manual_seed(63)
    a, b = torch.randn(shape, generator=g).to(cuda), torch.randn(shape, generator=g).to(cuda)
    assert a.numel() % 4 != 0
    assert torch.equal(ops.add(a, b), a + b)
