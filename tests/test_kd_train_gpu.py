"""The distillation term inside a training step: DeepLabv3-R50 at 2 x 3 x 65 x 65, 19 classes, criterion
`ce,kd` with kd_weight 0.5 and T = 2, a frozen teacher with other weights than the student's (closed-form against a seeded
initialisation) - as an fp32 Seg_Model and as an fp16 engine - and tools/train.py with --teacher-from.

The kd share of the loss and of the classifier-bias gradient is compared with the fp64 reference of tests/_kd_ref.py
evaluated on the very logits the student's lowres_logits and the Teacher returned in that step (a criterion wrapper
records them), under the rule of tests/test_loss_eval_kernels_gpu.py; the ce share comes from a ce-only step of the same
model on the same batch."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kd_ref as kr  # noqa: E402
import _model_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

KD_WEIGHT, KD_T = 0.5, 2.0
BIAS = "last_conv.6.bias"


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


def _student(seed):
    """Default-initialised (seeded) DeepLabv3-R50 at the widths of the suite's whole-model cases."""
    from dcfp_amd import networks
    torch.manual_seed(seed)
    m = networks.deeplabv3.Seg_Model(backbone="resnet50", backbone_para=dict(mc.BB), model_para={}, num_classes=19,
                                     align_corner=True, criterion=None, deepsup=True)
    m.conv_deepsup[3].p = 0.0            # (no dropout draw: the ce-only step and the ce,kd step see the same network)
    return m


def _dense():
    """The teacher: the same architecture with the suite's closed-form weights - other weights than the student's, and
    with running statistics an eval-mode forward (fp32 or fp16 engine) can use, which a fresh initialisation lacks."""
    return mc.build_model("deeplabv3", "resnet50", True, torch.device("cpu"), criterion=False).eval()


@pytest.fixture(scope="module")
def step(cuda):
    """One batch through: a ce-only step, a ce,kd step with a Seg_Model teacher, one with an engine teacher (gradients
    only), then one FusedSGD update.  Everything the tests below look at, on the CPU."""
    from dcfp_amd import deploy
    from dcfp_amd.distill import Teacher
    from dcfp_amd.loss.criterion import build_criterions
    from dcfp_amd.optimizer import FusedSGD
    g = torch.Generator().manual_seed(99)
    x = torch.randn(2, 3, 65, 65, generator=g).to(cuda)
    lab = torch.randint(0, 19, (2, 65, 65), generator=g)
    lab[torch.rand(2, 65, 65, generator=g) < 0.05] = 255
    lab = lab.to(cuda)
    student = _student(1).to(cuda).train()
    dense = _dense()
    dense_state = copy.deepcopy(dense.state_dict())
    para = {"ds_weight": 0.4, "kd_weight": KD_WEIGHT, "kd_T": KD_T}
    ce, cekd = _Tap(build_criterions("ce", _DS(), para)), _Tap(build_criterions("ce,kd", _DS(), para))
    opt = FusedSGD([p for p in student.parameters() if p.requires_grad], lr=1e-3, momentum=0.9, weight_decay=5e-4)
    bias = dict(student.named_parameters())[BIAS]
    rec = {"dense_state": dense_state}

    def run(crit, labels):
        opt.zero_grad()
        student.criterion = crit
        loss = student(x, labels, deepsup=True)["loss"]
        loss.backward()
        return loss.detach().cpu(), bias.grad.detach().cpu().clone(), crit.seen.cpu()

    rec["ce"] = run(ce, lab)
    teacher = Teacher(dense.to(cuda))
    t_model = teacher(x)
    assert not t_model.requires_grad
    rec["kd_model"] = run(cekd, {"ori": lab, "teacher": t_model}) + (t_model.cpu(),)
    engine_teacher = Teacher(deploy.build_engine(_dense())).to(cuda)
    t_engine = engine_teacher(x)
    again = engine_teacher(x)                                    # the first result is the caller's: a second call leaves it
    rec["engine_owns_result"] = t_engine.data_ptr() != again.data_ptr() and torch.equal(t_engine, again)
    rec["engine_parameters"] = engine_teacher.parameters()
    rec["kd_engine"] = run(cekd, {"ori": lab, "teacher": t_engine}) + (t_engine.cpu(),)
    before = {k: v.detach().clone() for k, v in dense.state_dict().items()}
    w0 = bias.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    rec["student_moved"] = not torch.equal(w0, bias.detach())
    rec["teacher_unchanged"] = [k for k, v in dense.state_dict().items() if not torch.equal(v, before[k])]
    rec["teacher_grads"] = [k for k, p in dense.named_parameters() if p.grad is not None or p.requires_grad]
    arena = opt.arena()
    lo, hi = arena.flat_param.data_ptr(), arena.flat_param.data_ptr() + 4 * arena.flat_param.numel()
    rec["teacher_in_arena"] = [k for k, p in dense.named_parameters()
                               if getattr(p, "_dcfp_slot", None) is not None or lo <= p.data_ptr() < hi
                               or any(p is q for q in arena.params)]
    rec["arena_size"] = len(arena.params)
    rec["n_student"] = len(list(student.parameters()))
    return rec


def _kd_share(rec, key, what):
    loss_ce, g_ce, s_ce = rec["ce"]
    loss, g, s, t = rec[key]
    assert torch.equal(s, s_ce)                                   # the same student logits in both steps
    assert s.shape == (2, 19, 9, 9) and t.shape == s.shape and t.dtype == torch.float32
    ref64, ref32 = (kr.kd_ref(s, t, KD_T, "pixel", dt) for dt in (torch.float64, torch.float32))
    if what == "loss":
        want = float(loss_ce) + KD_WEIGHT * float(ref64[0])
        yard = KD_WEIGHT * abs(float(ref32[0]) - float(ref64[0])) / max(1.0, abs(want))
        kr.held("kd_train", key, "loss", kr.rel1(loss, want), yard, kr.CE_FLOOR)
        assert float(ref64[0]) > 1e-3 and float(loss) > float(loss_ce)        # (the term is there at all)
    else:
        want = g_ce.double() + KD_WEIGHT * ref64[1].sum(dim=(0, 2, 3))
        yard = KD_WEIGHT * float((ref32[1].double() - ref64[1]).sum(dim=(0, 2, 3)).norm()) / float(want.norm())
        kr.held("kd_train", key, "classifier-bias gradient", kr.nrel(g, want), yard, kr.CE_GFLOOR)
        assert float((g - g_ce).norm()) > 1e-3 * float(g_ce.norm())


def test_loss_is_ce_plus_weighted_kd(step):
    _kd_share(step, "kd_model", "loss")


def test_bias_gradient_is_ce_plus_weighted_kd(step):
    _kd_share(step, "kd_model", "grad")


def test_teacher_parameters_stay_out_of_the_step(step):
    assert step["student_moved"]
    assert step["teacher_unchanged"] == []
    assert step["teacher_grads"] == []
    assert step["teacher_in_arena"] == []
    assert step["arena_size"] == step["n_student"]


def test_engine_teacher(step):
    _kd_share(step, "kd_engine", "loss")
    _kd_share(step, "kd_engine", "grad")
    assert step["engine_owns_result"] and step["engine_parameters"] == []
    # the fp16 engine's logits are the fp32 teacher's up to fp16 rounding: the same teacher, not the same numbers
    t32, t16 = step["kd_model"][3], step["kd_engine"][3]
    # (fp16 rounds at 2^-11 = 4.9e-4 per stored value; through ~55 convs that is a few 1e-3 of the norm)
    assert not torch.equal(t32, t16)
    assert kr.nrel(t16, t32) <= 2e-2


@pytest.mark.parametrize("engine", ["True"])
def test_driver_runs_with_a_teacher(step, tmp_path, engine):
    ckpt = str(tmp_path / "dense.pth")
    torch.save(step["dense_state"], ckpt)
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.join(ROOT, "tools", "train.py"), "--ddp", "False",
           "--loss-type", "ce,kd", "--loss-para", '{"kd_weight": 0.5, "kd_T": 2.0}', "--teacher-from", ckpt,
           "--teacher-engine", engine, "--num-steps", "3", "--input-size", "65,65", "--batch-size", "2",
           "--snapshot-dir", str(tmp_path / "snap"), "--learning-rate", "1e-3", "--backbone-para", json.dumps(mc.BB)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    losses = [float(l.split("loss=")[1]) for l in r.stdout.splitlines() if "loss=" in l]
    assert len(losses) == 3 and all(np.isfinite(losses)), r.stdout[-2000:]
