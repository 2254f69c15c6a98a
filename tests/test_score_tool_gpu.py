"""GPU: the baseline criteria on a whole model and through the tools, networks.simple R50 at 19 classes with
random weights.  tools/train.py, tools/score.py and tools/prune.py are loaded with importlib and run by main(argv).

  - weight_scores for every criterion: the keys of dcfp_pruning's score, the BN widths, and equal to a per-layer fp64
    computation from build_graph(model).norm_conv_links by the rule of tests/_kd_ref.py (norm-relative per layer, at
    most max(CE_FLOOR, 3 x the distance of the same formula in fp32 on the CPU from fp64));
  - train.py --prune-type taylor / taylor_w: the score file, and the gate score against the numpy float32 restatement
    from the gamma, beta and gradients captured in front of every scoring step;
  - train.py --slim-lambda: gamma after one step against the run without it;
  - score.py --criterion fpgm, then prune.py --score-norm l2: the pruned model loads, the masks are those of
    compute_thresholds / compute_out_masks on the normalised device scores."""
import copy
import importlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import _kd_ref as kr  # noqa: E402

from dcfp_amd import networks, pruners  # noqa: E402
from dcfp_amd.pruners.channel_pruner import build_graph  # noqa: E402
from dcfp_amd.utils.pyt_utils import load_model  # noqa: E402

pytestmark = pytest.mark.gpu

BB = '{"pretrained": false}'
MODEL = ["--model", "simple", "--backbone", "resnet50", "--backbone-para", BB]
TRAIN = MODEL + ["--input-size", "65,65", "--batch-size", "2"]


def build(deepsup=True):
    return networks.simple.Seg_Model(backbone="resnet50", backbone_para={"pretrained": False}, num_classes=19,
                                     align_corner=True, criterion=None, deepsup=deepsup)


@pytest.fixture(scope="module")
def random_model(tmp_path_factory):
    """(CPU model, path of its checkpoint): seeded random weights, BN weights and biases drawn too (the default
    initialisation has gamma = 1 and beta = 0 everywhere, which says nothing about a criterion)."""
    torch.manual_seed(31)
    m = build()
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
    path = str(tmp_path_factory.mktemp("ckpt") / "random.pth")
    torch.save(m.state_dict(), path)
    return m, path


def formula(criterion, gamma, w, dtype):
    w = w.to(dtype).reshape(w.shape[0], -1)
    if criterion == "slimming":
        return gamma.to(dtype).abs()
    if criterion == "l1":
        return w.abs().sum(1)
    if criterion == "l2":
        return (w * w).sum(1).sqrt()
    return torch.cdist(w, w, compute_mode="donot_use_mm_for_euclid_dist").sum(1)


@pytest.mark.parametrize("criterion", ["slimming", "l1", "l2", "fpgm"])
def test_weight_scores_on_the_whole_model(cuda, random_model, criterion):
    m, _ = random_model
    keys = list(pruners.dcfp_pruning(m).state_dict["eic"])
    links = build_graph(m).norm_conv_links
    dm = copy.deepcopy(m).to(cuda)
    got = pruners.weight_scores(dm, criterion)
    again = pruners.weight_scores(dm, criterion)
    assert list(got) == keys
    mods = dict(m.named_modules())
    def yardstick(bn, ref64):
        return kr.nrel(formula(criterion, mods[bn].weight.detach(), mods[links[bn]].weight.detach(), torch.float32), ref64)
    worst = (-1.0, None, None)
    for bn in keys:
        gamma, w = mods[bn].weight.detach(), mods[links[bn]].weight.detach()
        s = got[bn].cpu()
        assert s.dtype == torch.float32 and tuple(s.shape) == (gamma.numel(),) == (w.shape[0],)
        assert torch.equal(s, again[bn].cpu()), bn
        ref64 = formula(criterion, gamma, w, torch.float64)
        err = kr.nrel(s, ref64)
        if not err <= kr.CE_FLOOR:             # under the floor the bound holds whatever the yardstick: it is not computed
            kr.held("weight_scores", criterion, bn, err, yardstick(bn, ref64), kr.CE_FLOOR)
        if err > worst[0]:
            worst = (err, bn, ref64)
    err, bn, ref64 = worst
    kr.held("weight_scores", criterion, f"worst layer {bn}", err, yardstick(bn, ref64), kr.CE_FLOOR)


def load_tool(name):
    return importlib.import_module(name)


def test_train_tool_taylor_gate_score_against_the_restatement(cuda, tmp_path, monkeypatch):
    train = load_tool("train")
    captured = []
    real_step = pruners.taylor_pruning.step

    def step(self, model):                      # what the scorer sees: parameters and gradients right after backward
        mods = dict(model.named_modules())
        captured.append({n: tuple(t.detach().cpu().numpy().copy() for t in
                                  (mods[n].weight, mods[n].bias, mods[n].weight.grad, mods[n].bias.grad))
                         for n in self._names})
        return real_step(self, model)

    monkeypatch.setattr(pruners.taylor_pruning, "step", step)
    d = str(tmp_path / "gate")
    train.main(TRAIN + ["--num-steps", "2", "--prune-type", "taylor", "--snapshot-dir", d])
    f = torch.load(d + "/score.pth")
    assert f["criterion"] == "taylor" and f["steps"] == 2 and len(captured) == 2
    keys = list(pruners.dcfp_pruning(build()).state_dict["eic"])
    assert list(f["eic"]) == keys
    nonzero = 0
    for bn in keys:
        total = None
        for cap in captured:
            ga, be, gg, bg = cap[bn]
            a = ga * gg                              # float32 arrays: one rounding per operation
            b = be * bg
            t = a + b
            tt = t * t
            total = tt if total is None else total + tt          # (the first step adds to +0)
        want = total / np.float32(2)
        s = f["eic"][bn]
        assert s.dtype == torch.float32 and bool(torch.isfinite(s).all()) and float(s.min()) >= 0.0
        assert np.array_equal(s.numpy().view(np.int32), want.view(np.int32)), bn
        nonzero += int((s > 0).sum())
    assert nonzero > 0
    assert pruners.DCFPPruner(global_percent=0.5, layer_keep=0.02, score_file=d + "/score.pth").eic.keys() == f["eic"].keys()


def test_train_tool_taylor_weight_score(cuda, tmp_path, monkeypatch):
    train = load_tool("train")
    probes = ["backbone.bn1", "backbone.layer2.0.bn3", "last_conv.1"]      # K = 27 (the stem), a 1x1, the head's 3x3
    captured = []
    real_step = pruners.taylor_pruning.step

    def step(self, model):
        mods = dict(model.named_modules())
        captured.append({bn: (mods[self._convs[bn]].weight.detach().cpu().clone(),
                              mods[self._convs[bn]].weight.grad.detach().cpu().clone()) for bn in probes})
        return real_step(self, model)

    monkeypatch.setattr(pruners.taylor_pruning, "step", step)
    d = str(tmp_path / "weight")
    train.main(TRAIN + ["--num-steps", "2", "--prune-type", "taylor_w", "--snapshot-dir", d])
    f = torch.load(d + "/score.pth")
    assert f["criterion"] == "taylor_w" and f["steps"] == 2 and len(captured) == 2
    m = build()
    assert list(f["eic"]) == list(pruners.dcfp_pruning(m).state_dict["eic"])
    mods = dict(m.named_modules())
    for bn, s in f["eic"].items():
        assert s.dtype == torch.float32 and tuple(s.shape) == (mods[bn].weight.numel(),)
        assert bool(torch.isfinite(s).all()) and float(s.min()) >= 0.0, bn
    assert sum(int((s > 0).sum()) for s in f["eic"].values()) > 0

    def mean_sq_dot(bn, dtype):
        return sum((w.to(dtype).flatten(1) * g.to(dtype).flatten(1)).sum(1) ** 2
                   for w, g in (cap[bn] for cap in captured)) / 2
    for bn in probes:
        ref64 = mean_sq_dot(bn, torch.float64)
        kr.held("taylor_w", bn, "score", kr.nrel(f["eic"][bn], ref64), kr.nrel(mean_sq_dot(bn, torch.float32), ref64),
                kr.CE_FLOOR)


def test_train_tool_slim_lambda_moves_gamma_by_lr_lambda_sign(cuda, tmp_path):
    """One SGD step (momentum buffer = g + wd p on the first step, p -= lr buf) with and without the L1 term, from one
    checkpoint whose gammas have both signs and zeros.  p_plain - p_slim = lr (buf_slim - buf_plain) up to one rounding
    per operation: of the two final parameters (half an ulp of p each: eps |p| together, eps = 2^-23), and, times lr, of
    g + lambda sign and of the two buffers (half an ulp each of values no larger than |buf| + lambda (+ wd |p| for g)),
    and of lr and lambda themselves as floats (eps lr lambda): eps |p| + 2 eps (lr |buf| + lr lambda) with room left in
    the 2, where lr |buf| is read off the plain run as |p0 - p_plain|.  What that reading and wd |p| add is below a
    hundredth of eps |p| (lr wd = 5e-6): the 1.01."""
    train = load_tool("train")
    torch.manual_seed(41)
    m = build()
    names = list(pruners.dcfp_pruning(m).state_dict["eic"])
    g = torch.Generator().manual_seed(42)
    mods = dict(m.named_modules())
    with torch.no_grad():
        for n in names:
            w = mods[n].weight
            w.mul_(torch.where(torch.rand(w.shape, generator=g) < 0.5, -1.0, 1.0))
            w[::7] = 0.0
    ck = str(tmp_path / "start.pth")
    torch.save(m.state_dict(), ck)
    lr, lam = 1e-2, 1e-4
    common = TRAIN + ["--num-steps", "1", "--resume", ck, "--learning-rate", str(lr)]
    train.main(common + ["--snapshot-dir", str(tmp_path / "plain")])
    train.main(common + ["--snapshot-dir", str(tmp_path / "slim"), "--slim-lambda", str(lam)])
    plain = torch.load(str(tmp_path / "plain" / "CS_scenes_1.pth"), map_location="cpu")
    slim = torch.load(str(tmp_path / "slim" / "CS_scenes_1.pth"), map_location="cpu")
    eps = 2.0 ** -23
    moved = 0
    for n in names:
        p0 = mods[n].weight.detach().double()
        a, b = plain[n + ".weight"].double(), slim[n + ".weight"].double()
        want = lr * lam * torch.sign(p0)
        big = torch.maximum(torch.maximum(a.abs(), b.abs()), p0.abs())
        bound = 1.01 * eps * big + 2 * eps * ((p0 - a).abs() + lr * lam)
        err = ((a - b) - want).abs()
        assert bool((err <= bound).all()), (n, float((err / bound).max()))
        zero = p0 == 0
        assert torch.equal(plain[n + ".weight"][zero], slim[n + ".weight"][zero])     # sign(0) = 0: the same bits
        moved += int(((a - b) != 0).sum())
    assert moved > 0
    for k in plain:                                       # nothing else is touched: the other parameters keep their bits
        if k.endswith(".weight") and k[:-7] in names:
            continue
        if not any(k.startswith(n + ".") for n in names):
            assert torch.equal(plain[k], slim[k]), k


def test_score_tool_fpgm_then_prune_tool_with_l2_norm(cuda, tmp_path, random_model):
    m, ck = random_model
    score, prune = load_tool("score"), load_tool("prune")
    sp, out = str(tmp_path / "fpgm" / "score.pth"), str(tmp_path / "pruned")
    ms = score.main(MODEL + ["--criterion", "fpgm", "--dataset", "CS", "--model-path", ck, "--out", sp])
    assert ms > 0
    f = torch.load(sp)
    assert f["criterion"] == "fpgm" and list(f["eic"]) == list(pruners.dcfp_pruning(m).state_dict["eic"])
    gp = prune.main(MODEL + ["--dataset", "CS", "--model-path", ck, "--score-path", sp, "--score-norm", "l2",
                             "--prune-ratio", "0.3", "--save-path", out])
    assert 0.5 <= gp < 1.0
    cfg = torch.load(out + "/channel_cfg.pth", weights_only=False)
    slim = build(deepsup=False)
    pruners.init_pruned_model(slim, cfg)
    load_model(slim, out + "/pruned.pth")
    sd = torch.load(out + "/pruned.pth")
    assert all(tuple(v.shape) == tuple(sd[k].shape) and torch.equal(v, sd[k]) for k, v in slim.state_dict().items()
               if k in sd)
    assert sum(p.numel() for p in slim.parameters()) < sum(p.numel() for p in build(deepsup=False).parameters())
    # the masks: DCFPPruner's thresholds (compute_thresholds / compute_out_masks) on the normalised DEVICE scores
    dev_scores = {k: v.cpu() for k, v in pruners.weight_scores(copy.deepcopy(m).to(cuda), "fpgm").items()}
    p = pruners.DCFPPruner(global_percent=gp, layer_keep=0.02, score_file=sp)
    p.eic = pruners.normalize_scores(dev_scores, "l2")
    _, want = p.prune_model(copy.deepcopy(m), except_start_keys=["conv_deepsup"])
    assert set(want) == set(cfg)
    for name in want:
        for key in ("out_mask", "in_mask"):
            if key in want[name]:
                assert np.array_equal(want[name][key], cfg[name][key]), (name, key)
    assert any(c["out_channels"] < c["raw_out_channels"] for c in cfg.values() if "out_channels" in c)
