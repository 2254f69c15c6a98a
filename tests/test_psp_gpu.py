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
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:         # (also run as a script: the data-parallel child)
    sys.path.insert(0, ROOT)

from oracle import fill  # noqa: E402
from oracle.make_scores import synthetic_scores  # noqa: E402
from _parity import check_per_tensor, check_rankwise  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
BB = {"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128, "pretrained": False}
SIZES = (1, 2, 3, 6)


class _DS:
    ignore_label = 255
    num_classes = 19
    class_weights = None


def build(device, criterion=True, deepsup=True):
    from dcfp_amd import networks
    from dcfp_amd.loss.criterion import build_criterions
    crit = build_criterions("ce", _DS(), {"ds_weight": 0.4}) if criterion else None
    m = networks.psp.Seg_Model(backbone="resnet50", backbone_para=dict(BB), num_classes=19, align_corner=True,
                               criterion=crit, deepsup=deepsup)
    m.load_state_dict(fill.closed_form_state(m.state_dict()))
    if deepsup:
        m.conv_deepsup[3].p = 0.0
    return m.to(device).train()


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
    g = np.load(os.path.join(G, "model_psp_r50_2x65x65.npz"))
    N, H, W, align = [int(v) for v in g["meta"]]
    s = int(g["logit_step"])
    m = build(cuda)
    x = fill.closed_form_input(N, H, W).to(cuda)
    lab = fill.closed_form_labels(N, H, W).to(cuda)
    loss = m(x, lab, deepsup=True)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    ref64 = float(g["loss64"]); ref32 = float(g["loss32"])
    assert abs(loss.item() - ref64) <= max(1e-5 * abs(ref64), 3 * abs(ref32 - ref64)), (loss.item(), ref32, ref64)

    m2 = build(cuda)
    with torch.no_grad():
        outs = m2(x, None, deepsup=True)
    assert tuple(outs[0].shape) == (N, 19, H, W) and tuple(outs[1].shape) == (N, 19, H, W)
    for o, key, dkey in ((outs[0], "logits32", "logits_d64m32"), (outs[1], "logits_ds32", "logits_ds_d64m32")):
        l64 = g[key].astype(np.float64) + g[dkey]
        err = np.abs(o[:, :, ::s, ::s].double().cpu().numpy() - l64).max()
        ref_err = np.abs(g[dkey]).max()
        assert err <= max(1e-3, 3 * ref_err), (key, err, ref_err)

    names = g["bn_names"].tolist()
    mods = dict(m.named_modules())
    for what, attr in (("bn_wgrad", "weight"), ("bn_bgrad", "bias")):
        mine = torch.cat([getattr(mods[n], attr).grad.reshape(-1) for n in names]).double().cpu().numpy()
        r32 = g[what + "32"].astype(np.float64)
        r64 = r32 + g[what + "d64m32"]
        rel = np.linalg.norm(mine - r64) / np.linalg.norm(r64)
        ref_rel = np.linalg.norm(r32 - r64) / np.linalg.norm(r64)
        assert rel <= max(1e-3, 3 * ref_rel), (what, rel, ref_rel)

    pn = g["param_names"].tolist()
    params = dict(m.named_parameters())
    mine = np.array([float(params[k].grad.double().norm()) for k in pn])
    l64 = g["grad_l2:64"]
    rel = np.abs(mine - l64) / (np.abs(l64) + 1e-12)
    variants = [str(v) for v in g["fp32_variants"]]
    ref_rel = np.max([np.abs(g["grad_l2:" + v] - l64) for v in variants], axis=0) / (np.abs(l64) + 1e-12)
    check_per_tensor(rel, ref_rel, pn, "psp_r50_2x65x65 gradient norms", capsys)
    proj = np.array([float((params[k].grad.double().reshape(-1) *
                            torch.cos(0.37 * torch.arange(params[k].numel(), dtype=torch.float64, device=cuda))).sum())
                     for k in pn])
    p64 = g["grad_proj:64"]
    perr = np.abs(proj - p64) / (np.abs(l64) + 1e-12)
    pref = np.max([np.abs(g["grad_proj:" + v] - p64) for v in variants], axis=0) / (np.abs(l64) + 1e-12)
    check_rankwise(perr, pref, pn, "psp_r50_2x65x65 gradient projections", capsys)
    for key in ("backbone.conv1.0", "backbone.layer1.0.conv1", "last_conv"):
        a = params[key + ".weight"].grad.double().cpu().numpy()
        b32 = g[f"wgrad:{key}:32"].astype(np.float64)
        b = b32 + g[f"wgrad:{key}:d64m32"]
        rel = np.linalg.norm(a - b) / np.linalg.norm(b)
        ref_rel = np.linalg.norm(b32 - b) / np.linalg.norm(b)
        assert rel <= max(1e-3, 3 * ref_rel), (key, rel, ref_rel)
    sd = m.state_dict()
    for bn in ("backbone.bn1", "ppm.stages.0.2", "ppm.bottleneck.1"):
        for what in ("rm", "rv"):
            key = "running_mean" if what == "rm" else "running_var"
            mine, r32, r64 = sd[f"{bn}.{key}"].double().cpu().numpy(), g[f"{what}:{bn}:32"], g[f"{what}:{bn}:64"]
            assert np.abs(mine - r64).max() <= max(1e-5, 3 * np.abs(r32 - r64).max()), (bn, what)


def test_slim_model_matches_reference(cuda, tmp_path):
    """init_pruned_model from the reference-identical channel_cfg (tests/test_psp_host_cpu.py holds it to the golden
    bit for bit), the pruned weights loaded, eval mode at 2x3x33x33 (feats 5x5: the 6x6 stage pools with s > H)."""
    g = np.load(os.path.join(G, "prune_pspr50_gp50.npz"))
    from dcfp_amd import pruners
    from dcfp_amd.pruners.dcfp_pruner import DCFPPruner
    m = build(torch.device("cpu"), criterion=False)
    torch.save({"eic": synthetic_scores(m)}, str(tmp_path / "score.pth"))
    pruner = DCFPPruner(global_percent=0.5, layer_keep=0.02, score_file=str(tmp_path / "score.pth"))
    pruned, cfg = pruner.prune_model(copy.deepcopy(m), except_start_keys=["conv_deepsup"])
    assert list(cfg.keys()) == g["names"].tolist()
    slim = build(torch.device("cpu"), criterion=False)
    pruners.init_pruned_model(slim, cfg)
    slim.load_state_dict(pruned.state_dict())
    assert slim.ppm.bottleneck[0].weight.shape[1] == 3327
    slim = slim.to(cuda).eval()
    with torch.no_grad():
        y = slim(fill.closed_form_input(2, 33, 33).to(cuda), None, deepsup=True)
    err = np.abs(y[0].double().cpu().numpy() - g["slim_logits"]).max()
    assert err <= 1e-3, err


def _ddp_child():
    import argparse
    import torch.distributed as dist
    from dcfp_amd import networks, pruners, optimizer as opt
    from dcfp_amd.engine import Engine, DataParallel
    from dcfp_amd.loss.criterion import build_criterions

    class A:
        no_decay = "bn"; optim = "sgd"; momentum = 0.9; learning_rate = 1e-3; weight_decay = 5e-4
    dev = torch.device("cuda:0")
    x = fill.closed_form_input(2, 129, 129).to(dev)
    lab = fill.closed_form_labels(2, 129, 129).to(dev)

    def run(ddp):
        torch.manual_seed(12345)
        m = networks.psp.Seg_Model(backbone="resnet50", backbone_para=dict(BB), num_classes=19, align_corner=True,
                                   criterion=build_criterions("ce", _DS(), {"ds_weight": 0.4}), deepsup=True)
        m.load_state_dict(fill.closed_form_state(m.state_dict()))
        m.conv_deepsup[3].p = 0.0
        m = m.to(dev).train()
        optimizer = opt.build_optimizer(A, m)
        optimizer.zero_grad()
        tp = pruners.dcfp_pruning(m, 0.999)
        if ddp:
            sys.argv = ["x"]
            eng = Engine(custom_parser=argparse.ArgumentParser())
            eng.distributed = True
            model = eng.data_parallel(m)
            assert isinstance(model, DataParallel)
            assert isinstance(m.ppm.stages[0][2], torch.nn.SyncBatchNorm)
        else:
            model = m
        loss = model(x, lab, deepsup=True)["loss"]
        lv = (eng.all_reduce_tensor(loss) if ddp else loss).item()
        loss.backward()
        tp.step(m)
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
        eic = torch.cat([tp.get_eic()["eic"][n].reshape(-1) for n in tp._names]).clone()
        optimizer.step()
        torch.cuda.synchronize()
        bufs = {k: v.detach().clone() for k, v in m.state_dict().items()}
        return lv, grads, eic, bufs

    plain = run(False)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", DCFP_FORCE_SYNCBN="1")
    dist.init_process_group("nccl", rank=0, world_size=1)
    ddp = run(True)
    dist.destroy_process_group()
    out = {"loss": [plain[0], ddp[0]], "grad_diff": [k for k in plain[1] if not torch.equal(plain[1][k], ddp[1][k])],
           "eic_equal": bool(torch.equal(plain[2], ddp[2])),
           "state_diff": [k for k in plain[3] if not torch.equal(plain[3][k], ddp[3][k])], "n_params": len(plain[1])}
    print("DDP_RESULT " + json.dumps(out))


def test_data_parallel_bit_identical_to_plain(cuda):
    env = dict(os.environ, DCFP_FANIN_BN_SUMS="2")
    env.pop("DCFP_FORCE_SYNCBN", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ddp-child"], env=env, capture_output=True,
                       text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("DDP_RESULT ")][-1][len("DDP_RESULT "):])
    assert rec["loss"][0] == rec["loss"][1], rec["loss"]
    assert rec["grad_diff"] == [], rec["grad_diff"][:8]
    assert rec["eic_equal"]
    assert rec["state_diff"] == [], rec["state_diff"][:8]
    assert rec["n_params"] > 150


def test_train_then_prune_tools(cuda, tmp_path):
    g = np.load(os.path.join(G, "model_psp_r50_2x65x65.npz"))
    snap = str(tmp_path / "snap")
    bb = json.dumps({"pretrained": False})
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--model", "psp", "--ddp", "False",
           "--prune-type", "dcfp", "--input-size", "129,129", "--batch-size", "2", "--num-steps", "3",
           "--snapshot-dir", snap, "--backbone-para", bb, "--learning-rate", "1e-3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    losses = [float(l.split("loss=")[1]) for l in r.stdout.splitlines() if "loss=" in l]
    assert len(losses) == 3 and all(np.isfinite(losses)), r.stdout[-2000:]
    score = torch.load(os.path.join(snap, "score.pth"), weights_only=False)
    ign = set(g["ignore_prune_layer"].tolist())
    assert list(score["eic"].keys()) == [n for n in g["bn_names"].tolist() if n not in ign]
    ckpt = os.path.join(snap, "CS_scenes_3.pth")
    out = str(tmp_path / "pruned")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "prune.py"), "--model", "psp", "--model-path", ckpt,
           "--score-path", os.path.join(snap, "score.pth"), "--save-path", out, "--backbone-para", bb]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    cfg = torch.load(os.path.join(out, "channel_cfg.pth"), weights_only=False)
    assert "ppm.bottleneck.0" in cfg and "ppm.stages.3.1" in cfg


if __name__ == "__main__" and "--ddp-child" in sys.argv:
    _ddp_child()
