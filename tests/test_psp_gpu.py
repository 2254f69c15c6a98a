"""GPU: PSPNet (networks.psp) and the pyramid pooling kernels of csrc/ppm.hip on the MI355X.

* pool + place against fp64 F.adaptive_avg_pool2d at sizes (1, 2, 3, 6): overlapping windows (9x9, 17x33), s > H
  (5x5) and the config-3 feats shape; the copy into a pitched channel slice bit-exact, the other channels and the pitch
  tails untouched;
* the pool adjoint and the small-grid bilinear adjoint against fp64 autograd, both align_corners values, dense and
  pitched gradients, two runs bit-identical;
* run_sequential on AdaptiveAvgPool2d(3) (an s x s map, not a global mean);
* ops.PyramidPoolingFn against an fp64 ATen composite of ppm.py at full and ragged (pruned) widths, train and eval;
* the whole model against the reference's record (tests/golden/model_psp_r50_2x65x65.npz): loss, both heads' logits,
  per-tensor gradients (tests/_parity.py, unchanged rules), running statistics;
* the slim model of the reference's global_percent 0.5 pruning against its logits;
* the data-parallel path at world size 1 bit-identical to the plain step;
* tools/train.py -> score.pth -> tools/prune.py with --model psp."""
import copy
import sys

import pytest
import torch
import torch.nn.functional as F

import _model_cases as mc       # (run as a script - the data-parallel child - this file's directory is on sys.path)

pytestmark = pytest.mark.gpu
TAG = "psp_r50_2x65x65"
SIZES = (1, 2, 3, 6)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _pitch(W):
    return W + 4 + (-(W + 4)) % 4


@pytest.mark.parametrize("shape", [(2, 5, 9, 9), (2, 3, 17, 33), (2, 4, 5, 5), (4, 2048, 128, 256)])
def test_pool_and_place_vs_fp64(cuda, shape):
    from dcfp_amd import ops
    N, Cc, H, W = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randn(shape, generator=g).to(cuda)
    lo, Ctot = 3, Cc + 5
    buf = ops.new_pitched((N, Ctot, H, W), _pitch(W), cuda)
    buf.fill_(7.25)                                           # sentinels in every live float
    full = buf.as_strided((N, Ctot, H, buf.stride(2)), buf.stride())
    outs = ops.ppm_pool(x, [(s, s) for s in SIZES], True, dst=buf[:, lo:lo + Cc])
    sums = ops.ppm_pool(x, [(s, s) for s in SIZES], False)
    torch.cuda.synchronize()
    assert torch.equal(buf[:, lo:lo + Cc], x)                 # the copy is bit-exact
    assert bool((buf[:, :lo] == 7.25).all()) and bool((buf[:, lo + Cc:] == 7.25).all())
    assert float(full[..., W:].abs().max()) == 0.0            # the pitch tail was not written
    x64 = x.double()
    for s, o, sm in zip(SIZES, outs, sums):
        ref = F.adaptive_avg_pool2d(x64, s)
        assert tuple(o.shape) == (N, Cc, s, s)
        err = (o.double() - ref).abs().max().item()
        assert err <= 2e-6 * max(1.0, ref.abs().max().item()), (s, err)
        rows = [-(-(i + 1) * H // s) - i * H // s for i in range(s)]        # PyTorch's window heights / widths
        cols = [-(-(j + 1) * W // s) - j * W // s for j in range(s)]
        area = torch.tensor([[a * b for b in cols] for a in rows], dtype=torch.float64, device=cuda)
        assert ((sm.double() - ref * area).abs().max() / (ref * area).abs().max().clamp_min(1.0)).item() <= 2e-6
    again = ops.ppm_pool(x, [(s, s) for s in SIZES], True)
    assert all(torch.equal(a, b) for a, b in zip(outs, again))


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("HW", [(9, 9), (17, 33), (5, 5), (64, 128)])
def test_adjoints_vs_fp64_autograd(cuda, align, HW, pitched):
    from dcfp_amd import ops
    H, W = HW
    N, Cf, widths = 2, 6, [5, 3, 4, 7]
    levels = [(s, s) for s in SIZES]
    g = torch.Generator().manual_seed(2)
    Ct = sum(widths) + Cf
    dense = torch.randn(N, Ct + 2, H, W, generator=g).to(cuda)
    if pitched:
        gcat = ops.new_pitched((N, Ct + 2, H, W), _pitch(W), cuda)
        gcat.copy_(dense)
    else:
        gcat = dense
    gcat = gcat[:, 1:1 + Ct]                                   # (a channel slice: read in place)
    # the small-grid adjoint of every stage's resize, one launch
    priors = [torch.randn(N, c, s, s, generator=g, dtype=torch.float64).to(cuda).requires_grad_(True)
              for c, s in zip(widths, SIZES)]
    up = torch.cat([F.interpolate(p, size=HW, mode="bilinear", align_corners=align) for p in priors], 1)
    up.backward(gcat[:, :sum(widths)].double())
    dps = ops.ppm_resize_adjoint(gcat[:, :sum(widths)], widths, levels, align)
    for p, d in zip(priors, dps):
        assert _rel(d, p.grad) <= 1e-6, _rel(d, p.grad)
    dps2 = ops.ppm_resize_adjoint(gcat[:, :sum(widths)].contiguous(), widths, levels, align)
    assert all(torch.equal(a, b) for a, b in zip(dps, dps2))  # fixed order; dense and pitched read the same values
    # the pool adjoint: dx = g + sum over levels of the pooled gradients spread back over their windows
    x64 = torch.randn(N, Cf, H, W, generator=g, dtype=torch.float64).to(cuda).requires_grad_(True)
    dp = torch.randn(sum(N * Cf * s * s for s in SIZES), generator=g).to(cuda)
    views = [v.view(N, Cf, s, s) for v, s in zip(torch.split(dp, [N * Cf * s * s for s in SIZES]), SIZES)]
    gfe = gcat[:, sum(widths):]
    want = sum((F.adaptive_avg_pool2d(x64, s) * v.double()).sum() for s, v in zip(SIZES, views)) + \
        (x64 * gfe.double()).sum()
    want.backward()
    dx = ops.ppm_pool_adjoint(dp, levels, (N, Cf, H, W), g=gfe)
    assert _rel(dx, x64.grad) <= 1e-6, _rel(dx, x64.grad)
    assert torch.equal(dx, ops.ppm_pool_adjoint(dp, levels, (N, Cf, H, W), g=gfe.contiguous()))
    # g absent counts as zero
    x0 = x64.detach().clone().requires_grad_(True)
    sum((F.adaptive_avg_pool2d(x0, s) * v.double()).sum() for s, v in zip(SIZES, views)).backward()
    assert _rel(ops.ppm_pool_adjoint(dp, levels, (N, Cf, H, W)), x0.grad) <= 1e-6


def test_small_grid_adjoint_at_config3_matches_the_generic_kernel(cuda):
    from dcfp_amd import ops
    N, H, W, widths = 4, 128, 256, [512] * 4
    g = torch.Generator().manual_seed(4)
    dy = torch.randn(N, sum(widths), H, W, generator=g).to(cuda)
    dps = ops.ppm_resize_adjoint(dy, widths, [(s, s) for s in SIZES], True)
    for k, s in enumerate(SIZES):
        base = ops.resize_bilinear_adjoint(dy[:, 512 * k:512 * (k + 1)], (s, s), True)
        assert _rel(dps[k], base) <= 1e-5                      # (two fp32 summation orders)


def test_run_sequential_adaptive_pool(cuda):
    from dcfp_amd.networks import _exec
    g = torch.Generator().manual_seed(3)
    x64 = torch.randn(2, 7, 17, 33, generator=g, dtype=torch.float64).to(cuda).requires_grad_(True)
    x = x64.detach().float().requires_grad_(True)
    for size in (3, (2, 6)):
        seq = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(size))
        y = _exec.run_sequential(seq, x)
        ref = F.adaptive_avg_pool2d(x64, size)
        assert tuple(y.shape) == tuple(ref.shape)
        assert _rel(y.detach(), ref.detach()) <= 1e-6
        dy = torch.randn(ref.shape, generator=g).to(cuda)
        x.grad = None; x64.grad = None
        y.backward(dy); ref.backward(dy.double())
        assert _rel(x.grad, x64.grad) <= 1e-6
    # (1, 1) keeps the global mean kernel
    from dcfp_amd import ops
    one = _exec.run_sequential(torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(1)), x.detach())
    assert torch.equal(one, ops.global_avg_pool(x.detach()))


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("widths,HW", [(None, (9, 9)), ([319, 318, 318, 324], (17, 33)), (None, (64, 128))])
def test_pyramid_pooling_vs_fp64_composite(cuda, train, widths, HW):
    from dcfp_amd import ops
    from dcfp_amd.networks import _exec
    from dcfp_amd.networks.tools.ppm import PPMModule
    N, Cf = 2, 2048
    g = torch.Generator().manual_seed(5)
    mod = PPMModule(Cf, 512, align_corners=True)
    if widths is not None:                                     # ragged (pruned) stage widths
        for st, w in zip(mod.stages, widths):
            st[1].weight = torch.nn.Parameter(st[1].weight.data[:w].clone())
            st[2].weight = torch.nn.Parameter(st[2].weight.data[:w].clone())
            st[2].bias = torch.nn.Parameter(st[2].bias.data[:w].clone())
            st[2].running_mean = st[2].running_mean[:w].clone(); st[2].running_var = st[2].running_var[:w].clone()
            st[2].num_features = w
        b0 = mod.bottleneck[0]
        b0.weight = torch.nn.Parameter(b0.weight.data[:, :sum(widths) + Cf].clone())
        b0.in_channels = sum(widths) + Cf
    with torch.no_grad():
        for st in mod.stages:
            c, bn = st[1], st[2]
            C = c.weight.shape[0]
            c.weight.copy_(torch.randn(c.weight.shape, generator=g) * 0.03)
            bn.weight.copy_(1.0 + 0.2 * torch.randn(C, generator=g))
            bn.bias.copy_(0.1 * torch.randn(C, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(C, generator=g))
            bn.running_var.copy_(1.0 + 0.3 * torch.rand(C, generator=g))
    ref = copy.deepcopy(mod).double().to(cuda).train(train)
    ref32 = copy.deepcopy(mod).to(cuda).train(train)            # ATen fp32: the bound's yardstick
    mod2 = copy.deepcopy(mod).to(cuda).train(train)
    mod = mod.to(cuda).train(train)
    wid = [st[1].weight.shape[0] for st in mod.stages]
    f64 = torch.relu(torch.randn(N, Cf, *HW, generator=g, dtype=torch.float64)).to(cuda).requires_grad_(True)
    f = f64.detach().float().requires_grad_(True)
    dcat = torch.randn(N, sum(wid) + Cf, *HW, generator=g).to(cuda)

    def node(m, x, pitch=None):
        tensors = [t for st in m.stages for t in (st[1].weight, st[2].weight, st[2].bias)]
        shape = (N, sum(wid) + Cf) + tuple(HW)
        if pitch is None:
            pitch = m.concat_pitch(shape) if torch.is_grad_enabled() else 0
        cfg = {"sizes": list(SIZES), "bn": [_exec._bn_args(st[2]) for st in m.stages], "pitch": pitch, "owner": m,
               "align": True}
        return ops.pyramid_pooling(x, cfg, tensors), pitch
    # (at 64 x 128 the concat is row-pitched whatever the conv library picks for bottleneck.0 at this shape)
    cat, pitch = node(mod, f, _pitch(HW[1]) if HW == (64, 128) else None)
    assert ops._pitch_of(cat) == pitch
    cat.backward(dcat)
    # the composite of ppm.py: pool -> 1x1 conv -> BN -> ReLU -> interpolate, then cat with feats; in fp64, and in fp32
    # for the bound (a training BatchNorm over the N = 2 values of the 1x1 stage is ill-conditioned in its backward)
    def composite(m, x):
        return torch.cat([F.interpolate(torch.relu(st[2](st[1](F.adaptive_avg_pool2d(x, s)))), size=HW,
                                        mode="bilinear", align_corners=True) for st, s in zip(m.stages, SIZES)] + [x], 1)
    want = composite(ref, f64)
    want.backward(dcat.double())
    f32 = f.detach().clone().requires_grad_(True)
    composite(ref32, f32).backward(dcat)
    torch.cuda.synchronize()
    assert _rel(cat.detach(), want.detach()) <= 1e-5
    assert torch.equal(cat.detach()[:, sum(wid):], f.detach())
    assert _rel(f.grad, f64.grad) <= max(1e-5, 3 * _rel(f32.grad, f64.grad))
    for st, rs, r32 in zip(mod.stages, ref.stages, ref32.stages):
        for a, b, c, floor in ((st[1].weight, rs[1].weight, r32[1].weight, 1e-4),
                               (st[2].weight, rs[2].weight, r32[2].weight, 1e-4),
                               (st[2].bias, rs[2].bias, r32[2].bias, 1e-5)):
            assert _rel(a.grad, b.grad) <= max(floor, 3 * _rel(c.grad, b.grad))
        assert _rel(st[2].running_mean, rs[2].running_mean) <= 1e-5
        assert _rel(st[2].running_var, rs[2].running_var) <= 1e-5
        assert int(st[2].num_batches_tracked) == int(rs[2].num_batches_tracked)
    with torch.no_grad():                                      # a dense concat for the inference conv, same values
        cat2, p2 = node(mod2, f.detach())
    assert p2 == 0 and _rel(cat2, want.detach()) <= 1e-5
    # the whole module (bottleneck included) runs and keeps its shape
    out = mod(f.detach().requires_grad_(True))
    assert tuple(out.shape) == (N, 512) + tuple(HW)


def test_forward_backward_vs_reference_golden(cuda, capsys):
    mc.forward_backward_vs_golden(TAG, cuda, capsys)


def test_slim_model_matches_reference(cuda, tmp_path):
    """(at 2x3x33x33 feats is 5x5: the 6x6 stage pools with s > H)"""
    def ragged_width(slim):
        assert slim.ppm.bottleneck[0].weight.shape[1] == 3327
    mc.slim_model_logits_check("psp", "pspr50", cuda, tmp_path, ragged_width)


def test_data_parallel_bit_identical_to_plain(cuda):
    mc.data_parallel_bit_identical(__file__)


def test_train_then_prune_tools(cuda, tmp_path):
    mc.train_then_prune(TAG, ("ppm.bottleneck.0", "ppm.stages.3.1"), tmp_path)


if __name__ == "__main__" and "--ddp-child" in sys.argv:
    mc.ddp_child("psp", 29547, lambda m: m.ppm.stages[0][2])
