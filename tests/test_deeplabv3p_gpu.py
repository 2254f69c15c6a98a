"""GPU: DeepLabv3+ (networks.deeplabv3p) on the MI355X.

* ops.DecoderConcatFn against an fp64 ATen composite (1x1 conv + BatchNorm + ReLU, interpolate, cat) at a ragged
  layer1 width (175, a pruned one) and on a row-pitched concat, in train and eval mode;
* the whole model against the reference's record (tests/golden/model_v3p_r50_2x65x65.npz): loss, both heads' logits,
  per-tensor gradients (tests/_parity.py, unchanged rules);
* the slim model of the reference's global_percent 0.5 pruning (ragged widths 175 / 146 / 147) against its logits;
* the data-parallel path at world size 1 bit-identical to the plain step (SyncBN through the node);
* tools/train.py -> score.pth -> tools/prune.py with --model deeplabv3p;
* the decoder's first 3x3 conv on the Winograd kernels at BASELINE config 3 shapes."""
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


class _DS:
    ignore_label = 255
    num_classes = 19
    class_weights = None


def build(device, criterion=True, deepsup=True):
    from dcfp_amd import networks
    from dcfp_amd.loss.criterion import build_criterions
    crit = build_criterions("ce", _DS(), {"ds_weight": 0.4}) if criterion else None
    m = networks.deeplabv3p.Seg_Model(backbone="resnet50", backbone_para=dict(BB), num_classes=19, align_corner=True,
                                      criterion=crit, deepsup=deepsup)
    m.load_state_dict(fill.closed_form_state(m.state_dict()))
    if deepsup:
        m.conv_deepsup[3].p = 0.0
    return m.to(device).train()


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("Cl,hw,HW", [(175, (17, 33), (33, 65)), (256, (64, 128), (128, 256))])
def test_decoder_concat_vs_fp64_composite(cuda, train, Cl, hw, HW):
    from dcfp_amd import ops
    from dcfp_amd.networks import _exec
    from dcfp_amd.networks.deeplabv3p import Decoder
    N, Cx = 2, 512
    g = torch.Generator().manual_seed(5)
    dec = Decoder(19, True, low_level_inplanes=Cl)
    with torch.no_grad():
        dec.conv1.weight.copy_(torch.randn(dec.conv1.weight.shape, generator=g) * 0.05)
        dec.bn1.weight.copy_(1.0 + 0.2 * torch.randn(48, generator=g))
        dec.bn1.bias.copy_(0.1 * torch.randn(48, generator=g))
        dec.bn1.running_mean.copy_(0.1 * torch.randn(48, generator=g))
        dec.bn1.running_var.copy_(1.0 + 0.3 * torch.rand(48, generator=g))
    ref = copy.deepcopy(dec).double()
    dec2 = copy.deepcopy(dec).to(cuda).train(train)          # (for the no_grad call below)
    dec = dec.to(cuda).train(train)
    ref = ref.to(cuda).train(train)
    x64 = torch.randn(N, Cx, *hw, generator=g, dtype=torch.float64).to(cuda).requires_grad_(True)
    low64 = torch.relu(torch.randn(N, Cl, *HW, generator=g, dtype=torch.float64)).to(cuda).requires_grad_(True)
    dcat = torch.randn(N, Cx + 48, *HW, generator=g).to(cuda)
    x = x64.detach().float().requires_grad_(True)
    low = low64.detach().float().requires_grad_(True)

    pitch = dec.concat_pitch((N, Cx + 48) + tuple(HW))
    cfg = {"bn": _exec._bn_args(dec.bn1), "pitch": pitch, "owner": dec, "align": True}
    cat = ops.decoder_concat(x, low, cfg, dec.conv1.weight, dec.bn1.weight, dec.bn1.bias)
    assert ops._pitch_of(cat) == pitch                      # (0 at 33 x 65: the 3x3 conv reads that shape dense)
    if HW == (128, 256):
        assert pitch >= HW[1] + 4                           # the row-pitched concat of the training graph
    cat.backward(dcat)

    a = F.interpolate(x64, size=HW, mode="bilinear", align_corners=True)
    # the ReLU with the kernel's mask: a pre-activation within fp32 rounding of 0 may take either side (one such element
    # moves d low by ~1e-3 relative at 2 x 48 x 128 x 256), which is not what this test is about
    b = ref.bn1(ref.conv1(low64)) * (cat.detach()[:, Cx:] > 0).double()
    want = torch.cat((a, b), 1)
    want.backward(dcat.double())
    torch.cuda.synchronize()
    assert _rel(cat.detach(), want.detach()) <= 1e-5
    assert _rel(x.grad, x64.grad) <= 1e-5
    assert _rel(low.grad, low64.grad) <= 1e-4
    assert _rel(dec.conv1.weight.grad, ref.conv1.weight.grad) <= 1e-4
    assert _rel(dec.bn1.weight.grad, ref.bn1.weight.grad) <= 1e-4
    assert _rel(dec.bn1.bias.grad, ref.bn1.bias.grad) <= 1e-5
    assert _rel(dec.bn1.running_mean, ref.bn1.running_mean) <= 1e-5
    assert _rel(dec.bn1.running_var, ref.bn1.running_var) <= 1e-5
    assert int(dec.bn1.num_batches_tracked) == int(ref.bn1.num_batches_tracked)
    # no_grad: the same values (a dense concat for the inference conv)
    with torch.no_grad():
        cfg2 = {"bn": _exec._bn_args(dec2.bn1), "pitch": 0, "owner": dec2, "align": True}
        cat2 = ops.decoder_concat(x.detach(), low.detach(), cfg2, dec2.conv1.weight, dec2.bn1.weight, dec2.bn1.bias)
    assert _rel(cat2, want.detach()) <= 1e-5


def test_forward_backward_vs_reference_golden(cuda, capsys):
    g = np.load(os.path.join(G, "model_v3p_r50_2x65x65.npz"))
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
    check_per_tensor(rel, ref_rel, pn, "v3p_r50_2x65x65 gradient norms", capsys)
    proj = np.array([float((params[k].grad.double().reshape(-1) *
                            torch.cos(0.37 * torch.arange(params[k].numel(), dtype=torch.float64, device=cuda))).sum())
                     for k in pn])
    p64 = g["grad_proj:64"]
    perr = np.abs(proj - p64) / (np.abs(l64) + 1e-12)
    pref = np.max([np.abs(g["grad_proj:" + v] - p64) for v in variants], axis=0) / (np.abs(l64) + 1e-12)
    check_rankwise(perr, pref, pn, "v3p_r50_2x65x65 gradient projections", capsys)
    for key in ("backbone.conv1.0", "backbone.layer1.0.conv1", "decoder.conv1", "decoder.last_conv.6"):
        a = params[key + ".weight"].grad.double().cpu().numpy()
        b32 = g[f"wgrad:{key}:32"].astype(np.float64)
        b = b32 + g[f"wgrad:{key}:d64m32"]
        rel = np.linalg.norm(a - b) / np.linalg.norm(b)
        ref_rel = np.linalg.norm(b32 - b) / np.linalg.norm(b)
        assert rel <= max(1e-3, 3 * ref_rel), (key, rel, ref_rel)
    sd = m.state_dict()
    for bn in ("backbone.bn1", "decoder.bn1"):
        assert np.abs(sd[bn + ".running_mean"].cpu().numpy() - g[f"rm:{bn}:64"]).max() < 1e-5
        assert np.abs(sd[bn + ".running_var"].cpu().numpy() - g[f"rv:{bn}:64"]).max() < 1e-5


def test_slim_model_matches_reference(cuda, tmp_path):
    """init_pruned_model from the reference-identical channel_cfg (tests/test_deeplabv3p_host_cpu.py holds it to the
    golden bit for bit), the pruned weights loaded, eval mode at 2x3x33x33: the reference's slim logits."""
    g = np.load(os.path.join(G, "prune_v3pr50_gp50.npz"))
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
    assert slim.decoder.conv1.weight.shape[1] == 175
    assert slim.decoder.last_conv[0].weight.shape[0] == 146 and slim.decoder.last_conv[3].weight.shape[0] == 147
    slim = slim.to(cuda).eval()
    with torch.no_grad():
        y = slim(fill.closed_form_input(2, 33, 33).to(cuda), None, deepsup=True)
    err = np.abs(y[0].double().cpu().numpy() - g["slim_logits"]).max()
    assert err <= 1e-3, err


def test_decoder_first_conv_on_winograd_at_config3(cuda):
    """BASELINE config 3 (4x3x1024x2048): the concat is 4 x 560 x 256 x 512, row-pitched for decoder.last_conv.0, whose
    three passes run on the Winograd kernels (the weight gradient and the data gradient on the fused ones)."""
    from dcfp_amd import _lib, ops
    from dcfp_amd.networks.deeplabv3p import Decoder
    dec = Decoder(19, True)
    shape = (4, 560, 256, 512)
    pitch = dec.concat_pitch(shape)
    assert pitch >= 512 + 4
    d = ops._desc(shape, tuple(dec.last_conv[0].weight.shape), 1, 1, 1, pitch, pitch)
    names = [ops.conv_kernel_name(d, k) for k in (_lib.CONV_FWD, _lib.CONV_DGRAD, _lib.CONV_WGRAD)]
    assert all(n.startswith("winograd_f2x2_3x3") for n in names), names
    assert "fused" in names[2], names
    assert bool(_lib.lib().dcfp_conv2d_pitch_supported(ctypes_byref(d)))


def ctypes_byref(d):
    import ctypes
    return ctypes.byref(d)


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
        m = networks.deeplabv3p.Seg_Model(backbone="resnet50", backbone_para=dict(BB), num_classes=19, align_corner=True,
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
            assert isinstance(m.decoder.bn1, torch.nn.SyncBatchNorm)
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
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29543", DCFP_FORCE_SYNCBN="1")
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
    g = np.load(os.path.join(G, "model_v3p_r50_2x65x65.npz"))
    snap = str(tmp_path / "snap")
    bb = json.dumps({"pretrained": False})
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--model", "deeplabv3p", "--ddp", "False",
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
    cmd = [sys.executable, os.path.join(ROOT, "tools", "prune.py"), "--model", "deeplabv3p", "--model-path", ckpt,
           "--score-path", os.path.join(snap, "score.pth"), "--save-path", out, "--backbone-para", bb]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    cfg = torch.load(os.path.join(out, "channel_cfg.pth"), weights_only=False)
    assert "decoder.last_conv.0" in cfg and "decoder.conv1" in cfg


if __name__ == "__main__" and "--ddp-child" in sys.argv:
    _ddp_child()
