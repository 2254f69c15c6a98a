"""The Lovasz-Softmax term inside a training step: DeepLabv3-R50 at 2 x 3 x 65 x 65, 19 classes, criterion
`ce,lovasz` with lovasz_weight 0.5, and tools/train.py with --loss-type ce,lovasz.

The lovasz share of the loss and of the classifier-bias gradient is compared with the fp64 restatement of
tests/_lovasz_ref.py evaluated on the very logits the student's lowres_logits returned in that step (a criterion wrapper
records them); the ce share comes from a ce-only step of the same model on the same batch.  The reference bins its own
fp64 probabilities: an error within fp32 rounding of a bin edge may fall on the other side on the device, which moves
the loss by less than 2^-20 and the gradient of that one pixel between two neighbouring bins' weights - inside the
bounds below, which are those of tests/test_kd_train_gpu.py (3e-6 relative for the loss, 3e-5 norm-relative for the
gradient) widened by the restatement's own fp32 - fp64 distance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lovasz_ref as lr  # noqa: E402
import _model_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

WEIGHT, BINS = 0.5, 1024
BIAS = "last_conv.6.bias"
CE_FLOOR, CE_GFLOOR = 3e-6, 3e-5           # tests/test_loss_eval_kernels_gpu.py


class _DS:
    ignore_label = 255
    num_classes = 19
    class_weights = None


class _Tap(torch.nn.Module):
    """A criterion that records the main head's low-resolution logits it is handed, then defers."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, None

    def forward_lowres(self, preds, labels, size, align_corner):
        self.seen = preds[0].detach().clone()
        return self.inner.forward_lowres(preds, labels, size, align_corner)


@pytest.fixture(scope="module")
def step(cuda):
    """One batch through a ce-only step and a ce,lovasz step of the same network; what the tests look at, on the CPU."""
    from dcfp_amd import networks
    from dcfp_amd.loss.criterion import build_criterions
    g = torch.Generator().manual_seed(99)
    x = torch.randn(2, 3, 65, 65, generator=g).to(cuda)
    lab = torch.randint(0, 19, (2, 65, 65), generator=g)
    lab[torch.rand(2, 65, 65, generator=g) < 0.05] = 255
    torch.manual_seed(1)
    model = networks.deeplabv3.Seg_Model(backbone="resnet50", backbone_para=dict(mc.BB), model_para={}, num_classes=19,
                                         align_corner=True, criterion=None, deepsup=True)
    model.conv_deepsup[3].p = 0.0            # (no dropout draw: both steps see the same network)
    model = model.to(cuda).train()
    para = {"ds_weight": 0.4, "lovasz_weight": WEIGHT, "lovasz_bins": BINS}
    bias = dict(model.named_parameters())[BIAS]
    rec = {"labels": lab}
    for key, labels in (("ce", lab.to(cuda)), ("ce,lovasz", {"ori": lab.to(cuda)})):
        crit = _Tap(build_criterions(key, _DS(), para))
        model.zero_grad()
        model.criterion = crit
        loss = model(x, labels, deepsup=True)["loss"]
        loss.backward()
        rec[key] = (loss.detach().cpu(), bias.grad.detach().cpu().clone(), crit.seen.cpu())
    return rec


def _refs(rec):
    if "refs" not in rec:
        s = rec["ce,lovasz"][2]
        rec["refs"] = tuple(lr.binned(s, rec["labels"], (65, 65), True, 255, BINS, dt)
                            for dt in (torch.float64, torch.float32))
    return rec["refs"]


def test_loss_is_ce_plus_weighted_lovasz(step):
    loss_ce, _, s_ce = step["ce"]
    loss, _, s = step["ce,lovasz"]
    assert torch.equal(s, s_ce) and s.shape == (2, 19, 9, 9)            # the same logits in both steps
    ref64, ref32 = _refs(step)
    want = float(loss_ce) + WEIGHT * float(ref64[0])
    err = abs(float(loss) - want) / max(1.0, abs(want))
    yard = WEIGHT * abs(float(ref32[0]) - float(ref64[0])) / max(1.0, abs(want))
    bound = max(CE_FLOOR, 3.0 * yard)
    print(f"PARITY lovasz_train loss: kernel {err:.3e} fp32-yardstick {yard:.3e} bound {bound:.3e}")
    assert err <= bound
    assert float(ref64[0]) > 1e-2 and float(loss) > float(loss_ce)      # (the term is there at all)


def test_bias_gradient_is_ce_plus_weighted_lovasz(step):
    _, g_ce, _ = step["ce"]
    _, g, _ = step["ce,lovasz"]
    ref64, ref32 = _refs(step)
    want = g_ce.double() + WEIGHT * ref64[1].sum(dim=(0, 2, 3))
    err = lr.nrel(g, want)
    yard = WEIGHT * float((ref32[1].double() - ref64[1]).sum(dim=(0, 2, 3)).norm()) / float(want.norm())
    bound = max(CE_GFLOOR, 3.0 * yard)
    print(f"PARITY lovasz_train classifier-bias gradient: kernel {err:.3e} fp32-yardstick {yard:.3e} bound {bound:.3e}")
    assert err <= bound
    assert float((g - g_ce).norm()) > 1e-3 * float(g_ce.norm())


def test_driver_runs_with_the_lovasz_term(tmp_path):
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.join(ROOT, "tools", "train.py"), "--ddp", "False",
           "--loss-type", "ce,lovasz", "--loss-para", '{"lovasz_weight": 0.5, "lovasz_bins": 256}', "--num-steps", "3",
           "--input-size", "65,65", "--batch-size", "2", "--snapshot-dir", str(tmp_path / "snap"),
           "--learning-rate", "1e-3", "--backbone-para", json.dumps(mc.BB)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    losses = [float(l.split("loss=")[1]) for l in r.stdout.splitlines() if "loss=" in l]
    assert len(losses) == 3 and all(np.isfinite(losses)), r.stdout[-2000:]
