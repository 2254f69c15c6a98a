"""Generate the PSPNet fixtures of tests/golden/ by importing the real reference on CPU, through
oracle/make_golden.py's helpers (imported, not changed).

Development machine only (the reference does not travel with the tree, so no test imports this file).  Run:
    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python /path/to/repo/tools/make_golden_psp.py
Writes model_psp_r50_2x65x65.npz, prune_pspr50_gp50.npz and flops_psp.npz.

make_golden.whole_model names the classifier `last_conv.6`; PSPNet's is the bare conv `last_conv`, so the whole-model
record is produced by `whole_model_psp` below: the arrays of tools/make_golden_v3p.py, plus the running statistics of
the first pyramid stage's BatchNorm (N values per channel) and of the bottleneck's."""
import copy
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from oracle import make_golden as mg  # noqa: E402  (puts the reference on sys.path and patches its pruner)
from oracle import fill  # noqa: E402
from oracle.make_scores import synthetic_scores  # noqa: E402

TAG, MODEL, BACKBONE = "psp_r50_2x65x65", "psp", "resnet50"
CLS = "last_conv"
STEP = 4           # logits stored at every 4th pixel of each axis (fixture size)
RUNNING = ("backbone.bn1", "ppm.stages.0.2", "ppm.bottleneck.1")


def _grad_summaries(m, grads, res, sfx):
    pnames = [k for k, _ in m.named_parameters()]
    res["grad_l2:" + sfx] = np.array([float(grads[k].double().norm()) for k in pnames])
    res["grad_proj:" + sfx] = np.array([
        float((grads[k].double().reshape(-1) * torch.cos(0.37 * torch.arange(grads[k].numel(), dtype=torch.float64))).sum())
        for k in pnames])
    return pnames


def whole_model_psp(tag, model, backbone, N, H, W, align):
    res = {}
    l32 = None
    for dtype, sfx in ((torch.float32, "32"), (torch.float64, "64")):
        torch.manual_seed(0)
        m = mg.build_ref(model, backbone, align, dtype)
        m.train()
        x = fill.closed_form_input(N, H, W, dtype)
        lab = fill.closed_form_labels(N, H, W)
        loss = m(x, lab, deepsup=True)["loss"]
        loss.backward()
        grads = {k: p.grad.detach() for k, p in m.named_parameters()}
        bn_names = [n for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)]
        res["loss" + sfx] = np.array(loss.item(), dtype=np.float64)
        # (fp64 arrays kept as float32 differences to the fp32 run, and four small weight gradients: the file stays < 1 MiB;
        #  a test rebuilds fp64 as fp32 + difference)
        flat = {"bn_wgrad": torch.cat([grads[n + ".weight"].reshape(-1) for n in bn_names]),
                "bn_bgrad": torch.cat([grads[n + ".bias"].reshape(-1) for n in bn_names])}
        for cname in ("backbone.conv1.0", "backbone.layer1.0.conv1", CLS):
            flat["wgrad:" + cname + ":"] = grads[cname + ".weight"]
        flat["bgrad:" + CLS + ":"] = grads[CLS + ".bias"]
        for k, v in flat.items():
            if sfx == "32":
                res[k + "32"] = v.numpy()
            else:
                res[k + "d64m32"] = (v - torch.from_numpy(res[k + "32"]).double()).float().numpy()
        pnames = _grad_summaries(m, grads, res, sfx)
        if sfx == "32":
            res["param_names"] = np.array(pnames)
        sd = m.state_dict()
        for bn in RUNNING:
            res[f"rm:{bn}:" + sfx] = sd[bn + ".running_mean"].numpy()
            res[f"rv:{bn}:" + sfx] = sd[bn + ".running_var"].numpy()
        m2 = mg.build_ref(model, backbone, align, dtype)
        m2.train()
        with torch.no_grad():
            outs = m2(x, None, deepsup=True)
        if sfx == "32":
            l32 = [o[:, :, ::STEP, ::STEP].clone() for o in outs]
            res["logits32"] = l32[0].numpy()
            res["logits_ds32"] = l32[1].numpy()
            res["bn_names"] = np.array(bn_names)
            res["state_keys"] = np.array(list(sd.keys()))
            res["state_shapes"] = np.array([str(tuple(v.shape)) for v in sd.values()])
            res["ignore_prune_layer"] = np.array(m.ignore_prune_layer)
        else:
            res["logits_d64m32"] = (outs[0][:, :, ::STEP, ::STEP] - l32[0].double()).float().numpy()
            res["logits_ds_d64m32"] = (outs[1][:, :, ::STEP, ::STEP] - l32[1].double()).float().numpy()
    # the same fp32 code in four more summation orders (tests/_parity.py takes a tensor's reference error as the largest)
    variants = (("32t1", 1, True), ("32t2", 2, True), ("32t4", 4, True), ("32nodnn", 8, False))
    for sfx, threads, dnn in variants:
        torch.set_num_threads(threads)
        torch.backends.mkldnn.enabled = dnn
        torch.manual_seed(0)
        m = mg.build_ref(model, backbone, align, torch.float32)
        m.train()
        m(fill.closed_form_input(N, H, W, torch.float32), fill.closed_form_labels(N, H, W), deepsup=True)["loss"].backward()
        _grad_summaries(m, {k: p.grad.detach() for k, p in m.named_parameters()}, res, sfx)
    torch.set_num_threads(8)
    torch.backends.mkldnn.enabled = True
    res["fp32_variants"] = np.array(["32"] + [v[0] for v in variants])
    res["meta"] = np.array([N, H, W, int(align)])
    res["logit_step"] = np.array(STEP)
    np.savez_compressed(os.path.join(mg.OUT, f"model_{tag}.npz"), **res)
    print("wrote", tag, "loss32", res["loss32"], "loss64", res["loss64"])


def flops_psp():
    """The reference's get_model_complexity_info on the full and the global_percent 0.5 PSPNet R50 at (3, 257, 257)."""
    from utils.flops_counter import get_model_complexity_info
    rec = {}
    m = mg.networks.psp.Seg_Model(backbone=BACKBONE, backbone_para=dict(mg.BB_PARA), model_para={}, num_classes=19,
                                         align_corner=True, criterion=None, deepsup=False)
    f, p = get_model_complexity_info(m, (3, 257, 257), print_per_layer_stat=False, as_strings=False)
    fs, ps = get_model_complexity_info(m, (3, 257, 257), print_per_layer_stat=False)
    rec["flops:psp_r50"] = np.array(float(f)); rec["params:psp_r50"] = np.array(float(p))
    rec["str:psp_r50"] = np.array([fs, ps])
    m = mg.build_ref(MODEL, BACKBONE, True, torch.float32)
    m.criterion = None
    torch.save({"eic": synthetic_scores(m)}, "/tmp/_golden_score_psp.pth")
    pruner = mg.dp.DCFPPruner(global_percent=0.5, layer_keep=0.02, score_file="/tmp/_golden_score_psp.pth")
    _, channel_cfg = pruner.prune_model(copy.deepcopy(m), except_start_keys=["conv_deepsup"])
    slim = mg.networks.psp.Seg_Model(backbone=BACKBONE, backbone_para=dict(mg.BB_PARA), model_para={},
                                            num_classes=19, align_corner=True, criterion=None, deepsup=False)
    mg.pruners.init_pruned_model(slim, channel_cfg)
    f, p = get_model_complexity_info(slim, (3, 257, 257), print_per_layer_stat=False, as_strings=False)
    rec["flops:psp_r50_gp50"] = np.array(float(f)); rec["params:psp_r50_gp50"] = np.array(float(p))
    np.savez_compressed(os.path.join(mg.OUT, "flops_psp.npz"), **rec)
    print("wrote flops_psp", {k: v.tolist() for k, v in rec.items()})


if __name__ == "__main__":
    torch.set_num_threads(8)
    which = sys.argv[1:] or ["model", "prune", "flops"]
    if "model" in which:
        whole_model_psp(TAG, MODEL, BACKBONE, 2, 65, 65, True)
    if "prune" in which:
        mg.PRUNE_CASES = [("pspr50", MODEL, BACKBONE, True, 0.5)]
        mg.masks_and_surgery()
    if "flops" in which:
        flops_psp()
