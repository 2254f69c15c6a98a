"""The pair-wise similarity term inside a training step: DeepLabv3-R50 at 2 x 3 x 65 x 65, criterion
`ce,kdpa` with pa_weight 0.5 and pa_pool 2 - the backbone's last tensor is 2 x 2048 x 9 x 9, so 25 nodes per image - and
a frozen teacher with other weights than the student's, as an fp32 Seg_Model and as an fp16 engine; the engine's feature
tap against Engine.trace; tools/train.py with `ce,kdpa`; one step of PSPNet, where the tapped tensor feeds the pyramid.

The term's share of the loss is compared with the fp64 reference of tests/_pa_ref.py on the very features of that step (a
hook of the test keeps the student's, with retain_grad), the ce share comes from a ce-only step of the same model on the
same batch.  The term's share of the gradient ARRIVING at the tapped tensor - autograd adds it to the head's - is the
difference of that tensor's .grad between the two steps; its bound is measured, not fixed: the kernel test's bound for
this shape (max(3e-5, 3 x the fp32 formula's distance), norm-relative), plus the run-to-run difference of the ce-only
gradient (two ce steps), plus 4 * 2^-24 * |grad| for autograd's one addition."""
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
import _pa_ref as pr  # noqa: E402
import _model_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

PA_WEIGHT, PA_POOL = 0.5, 2
PARA = {"ds_weight": 0.4, "pa_weight": PA_WEIGHT, "pa_pool": PA_POOL}


class _DS:
    ignore_label = 255
    num_classes = 19
    class_weights = None


def _student(name, seed):
    """Default-initialised (seeded) R50 model at the widths of the suite's whole-model cases."""
    from dcfp_amd import networks
    torch.manual_seed(seed)
    m = getattr(networks, name).Seg_Model(backbone="resnet50", backbone_para=dict(mc.BB), model_para={}, num_classes=19,
                                          align_corner=True, criterion=None, deepsup=True)
    m.conv_deepsup[3].p = 0.0            # (no dropout draw: the ce-only step and the ce,kdpa step see the same network)
    return m


def _dense(name="deeplabv3"):
    """The teacher: the same architecture with the suite's closed-form weights and usable running statistics."""
    return mc.build_model(name, "resnet50", True, torch.device("cpu"), criterion=False).eval()


def _batch(cuda):
    g = torch.Generator().manual_seed(99)
    x = torch.randn(2, 3, 65, 65, generator=g).to(cuda)
    lab = torch.randint(0, 19, (2, 65, 65), generator=g)
    lab[torch.rand(2, 65, 65, generator=g) < 0.05] = 255
    return x, lab.to(cuda)


class _Stepper:
    """Runs steps of one student under several criteria and keeps the tapped tensor (retain_grad) of each."""

    def __init__(self, student, lr=1e-3):
        from dcfp_amd.optimizer import FusedSGD
        self.student, self.feat = student, None
        self.opt = FusedSGD([p for p in student.parameters() if p.requires_grad], lr=lr, momentum=0.9, weight_decay=5e-4)
        student.backbone.register_forward_hook(self._keep)

    def _keep(self, module, args, out):
        self.feat = out[-1]
        if self.feat.requires_grad:
            self.feat.retain_grad()

    def run(self, crit, x, labels):
        self.opt.zero_grad()
        self.student.criterion = crit
        loss = self.student(x, labels, deepsup=True)["loss"]
        loss.backward()
        feat, self.feat = self.feat, None
        return loss.detach().cpu(), feat.detach().cpu(), feat.grad.detach().cpu().clone()


@pytest.fixture(scope="module")
def step(cuda):
    """One batch through DeepLabv3: two ce-only steps, a ce,kdpa step with a Seg_Model teacher, one with an engine teacher
    (gradients only), then one FusedSGD update.  Everything the tests below look at, on the CPU."""
    from dcfp_amd import deploy
    from dcfp_amd.distill import Teacher
    from dcfp_amd.loss.criterion import build_criterions
    x, lab = _batch(cuda)
    student = _student("deeplabv3", 1).to(cuda).train()
    dense = _dense()
    rec = {"dense_state": copy.deepcopy(dense.state_dict())}
    ce, cepa = build_criterions("ce", _DS(), PARA), build_criterions("ce,kdpa", _DS(), PARA)
    cepa.attach(student)
    st = _Stepper(student)
    rec["ce"], rec["ce_again"] = st.run(ce, x, lab), st.run(ce, x, lab)
    teacher = Teacher(dense.to(cuda))
    logits, t_model = teacher(x, feature=True)
    assert not t_model.requires_grad and torch.equal(logits, teacher(x))
    rec["pa_model"] = st.run(cepa, x, {"ori": lab, "teacher_feat": t_model}) + (t_model.cpu(),)
    rec["tap_empty_after_step"] = cepa.criterions[1]._tap.pop() is None
    engine_teacher = Teacher(deploy.build_engine(_dense())).to(cuda)
    logits16, t_engine = engine_teacher(x, feature=True)
    rec["engine_logits_equal"] = torch.equal(logits16, engine_teacher(x))
    rec["engine_parameters"] = engine_teacher.parameters()
    rec["pa_engine"] = st.run(cepa, x, {"ori": lab, "teacher_feat": t_engine}) + (t_engine.cpu(),)
    before = {k: v.detach().clone() for k, v in dense.state_dict().items()}
    bias = dict(student.named_parameters())["last_conv.6.bias"]
    w0 = bias.detach().clone()
    st.opt.step()
    torch.cuda.synchronize()
    rec["student_moved"] = not torch.equal(w0, bias.detach())
    rec["teacher_unchanged"] = [k for k, v in dense.state_dict().items() if not torch.equal(v, before[k])]
    rec["teacher_grads"] = [k for k, p in dense.named_parameters() if p.grad is not None or p.requires_grad]
    arena = st.opt.arena()
    lo, hi = arena.flat_param.data_ptr(), arena.flat_param.data_ptr() + 4 * arena.flat_param.numel()
    rec["teacher_in_arena"] = [k for k, p in dense.named_parameters()
                               if getattr(p, "_dcfp_slot", None) is not None or lo <= p.data_ptr() < hi
                               or any(p is q for q in arena.params)]
    rec["arena_size"], rec["n_student"] = len(arena.params), len(list(student.parameters()))
    # with no_grad / eval forwards nothing is kept, and nothing of the term runs
    with torch.no_grad():
        student(x, None, deepsup=True)
    rec["tap_empty_after_no_grad"] = cepa.criterions[1]._tap._kept is None
    return rec


def _share(rec, key, what):
    loss_ce, f_ce, g_ce = rec["ce"]
    loss, f, g, t = rec[key]
    assert torch.equal(f, f_ce) and f.shape == (2, 2048, 9, 9) and float(f.min()) >= 0.0     # the same post-ReLU feature
    ref64, ref32 = (pr.pa_ref(f, t, PA_POOL, dt) for dt in (torch.float64, torch.float32))
    assert float(ref64[0]) > 1e-4                                                           # (the term is there at all)
    if what == "loss":
        want = float(loss_ce) + PA_WEIGHT * float(ref64[0])
        yard = PA_WEIGHT * abs(float(ref32[0]) - float(ref64[0])) / max(1.0, abs(want))
        pr.held("pairwise_train", key, "loss", pr.rel1(loss, want), yard, pr.CE_FLOOR)
        assert float(loss) > float(loss_ce)
    else:
        want = PA_WEIGHT * ref64[1]
        delta = float((rec["ce_again"][2].double() - g_ce.double()).norm())
        kernel_bound = max(pr.CE_GFLOOR, 3.0 * pr.nrel(ref32[1], ref64[1])) * float(want.norm())
        bound = kernel_bound + delta + 4.0 * 2.0 ** -24 * float(g.double().norm())
        err = float(((g.double() - g_ce.double()) - want).norm())
        print(f"PARITY pairwise_train {key} gradient at the tap: err {err:.3e} bound {bound:.3e} (kernel {kernel_bound:.3e} "
              f"run-to-run {delta:.3e} |term| {float(want.norm()):.3e} |grad| {float(g.double().norm()):.3e})")
        assert err <= bound
        assert float(want.norm()) > 10.0 * bound                            # (the bound resolves the term)


def test_loss_is_ce_plus_weighted_term(step):
    _share(step, "pa_model", "loss")


def test_gradient_at_the_tap_is_the_heads_plus_the_weighted_term(step):
    _share(step, "pa_model", "grad")


def test_engine_teacher(step):
    _share(step, "pa_engine", "loss")
    _share(step, "pa_engine", "grad")
    assert step["engine_logits_equal"] and step["engine_parameters"] == []
    t32, t16 = step["pa_model"][3], step["pa_engine"][3]
    assert t16.dtype == torch.float16 and tuple(t16.shape) == (2, 9, 9, 2048) and tuple(t32.shape) == (2, 2048, 9, 9)
    # the fp16 engine's feature is the fp32 teacher's up to fp16 rounding through ~50 convs: the same teacher
    assert pr.nrel(t16.float().permute(0, 3, 1, 2), t32) <= 2e-2


def test_tap_holds_nothing_between_steps(step):
    assert step["tap_empty_after_step"] and step["tap_empty_after_no_grad"]


def test_teacher_parameters_stay_out_of_the_step(step):
    assert step["student_moved"]
    assert step["teacher_unchanged"] == []
    assert step["teacher_grads"] == []
    assert step["teacher_in_arena"] == []
    assert step["arena_size"] == step["n_student"]


@pytest.mark.parametrize("name", ["deeplabv3", "psp"])
def test_engine_tap_has_the_bytes_of_the_trace(cuda, name):
    from dcfp_amd import deploy
    x, _ = _batch(cuda)
    engine = deploy.build_engine(_dense(name)).to(cuda)
    at, rec = engine.backbone_record()
    assert rec["name"] == "backbone.layer4.2.conv3" and rec["cout"] == 2048
    logits, feat, channels = engine.lowres_logits_and_feature(x)
    trace = engine.trace(x)
    want = trace[rec["name"]]
    assert channels == 2048 and feat.is_contiguous() and feat.dtype == torch.float16
    assert tuple(feat.shape) == tuple(want.shape) and torch.equal(feat.view(torch.int16), want.view(torch.int16))
    assert torch.equal(logits, engine.lowres_logits(x)[0])
    if name == "psp":                                          # the record is a channel slice of the concat buffer
        assert engine.buffers[rec["dst"]] > feat.shape[3]
    with pytest.raises(NotImplementedError, match="fp8"):
        fp8 = deploy.Engine.__new__(deploy.Engine)
        fp8.format = deploy.FORMAT_F8
        fp8.lowres_logits_and_feature(x)


def test_driver_runs_with_the_term(step, tmp_path):
    ckpt = str(tmp_path / "dense.pth")
    torch.save(step["dense_state"], ckpt)
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.join(ROOT, "tools", "train.py"), "--ddp", "False",
           "--loss-type", "ce,kdpa", "--loss-para", json.dumps({"pa_weight": PA_WEIGHT, "pa_pool": PA_POOL}),
           "--teacher-from", ckpt, "--num-steps", "3", "--input-size", "65,65", "--batch-size", "2",
           "--snapshot-dir", str(tmp_path / "snap"), "--learning-rate", "1e-3", "--backbone-para", json.dumps(mc.BB)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    losses = [float(l.split("loss=")[1]) for l in r.stdout.splitlines() if "loss=" in l]
    assert len(losses) == 3 and all(np.isfinite(losses)), r.stdout[-2000:]


def test_second_consumer_is_safe_on_pspnet(cuda):
    """the tapped tensor feeds the pyramid pooling node and the concat: one ce step, one ce,kdpa step, same identities"""
    from dcfp_amd.distill import Teacher
    from dcfp_amd.loss.criterion import build_criterions
    x, lab = _batch(cuda)
    student = _student("psp", 2).to(cuda).train()
    ce, cepa = build_criterions("ce", _DS(), PARA), build_criterions("ce,kdpa", _DS(), PARA)
    cepa.attach(student)
    st = _Stepper(student)
    rec = {"ce": st.run(ce, x, lab), "ce_again": st.run(ce, x, lab)}
    _, t = Teacher(_dense("psp").to(cuda))(x, feature=True)
    rec["pa_psp"] = st.run(cepa, x, {"ori": lab, "teacher_feat": t}) + (t.cpu(),)
    _share(rec, "pa_psp", "loss")
    _share(rec, "pa_psp", "grad")
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in student.parameters())
