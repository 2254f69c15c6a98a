"""Host side of the pair-wise similarity distillation, no GPU: the reference of tests/_pa_ref.py against an
independent statement and against fp64 autograd, its dead-node rule, the `kdpa` criterion's errors, distill.FeatureTap,
the C-ABI's argument checks and workspace sizes, and the driver's flag check."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pa_ref as pr  # noqa: E402

# (N, Cs, Ct, h, w, pool): windows clipped at both edges, pool > h, one node, Cs != Ct both ways
SHAPES = [(2, 5, 5, 7, 9, 2), (1, 3, 8, 5, 5, 3), (2, 8, 3, 4, 6, 1), (1, 4, 4, 2, 3, 4), (3, 2, 2, 1, 1, 1),
          (1, 64, 32, 9, 9, 2)]


class _DS:
    ignore_label = 255
    num_classes = 19
    class_weights = None


def _sid(shape):
    return "x".join(map(str, shape))


def _pair(shape, seed=5, dead=()):
    N, Cs, Ct, h, w, _ = shape
    # (+ 0.05: no node of these inputs is anywhere near the dead-node threshold)
    s, t = pr.features((N, Cs, h, w), (N, Ct, h, w), seed, dead=())
    s, t = s + 0.05, t + 0.05
    for n, y, x in dead:
        s[n, :, y, x] = 0.0
    return s, t


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_reference_agrees_with_an_independent_statement_and_with_autograd(shape):
    s, t = _pair(shape)
    pool = shape[5]
    loss, grad = pr.pa_ref(s, t, pool, torch.float64)
    want, gwant = pr.pa_autograd(s, t, pool, torch.float64)
    assert abs(float(loss) - float(want)) <= 1e-13 * max(1.0, abs(float(want)))
    assert float((grad - gwant).norm()) <= 1e-13 * float(gwant.norm()) + 1e-15      # (one node: a gradient of rounding size)
    if shape[3] * shape[4] > 1 and -(-shape[3] // pool) * -(-shape[4] // pool) > 1:
        assert float(loss) > 0 and float(grad.abs().max()) > 0


def test_reference_takes_both_teacher_layouts():
    N, Cs, Ct, h, w, pool = 2, 5, 6, 5, 7, 2
    s, t = _pair((N, Cs, Ct, h, w, pool))
    t16 = t.half()
    wide = torch.full((N, h, w, Ct + 5), float("nan"), dtype=torch.float16)
    wide[..., 2:2 + Ct] = t16.permute(0, 2, 3, 1)
    a = pr.pa_ref(s, t16.float(), pool, torch.float64)
    b = pr.pa_ref(s, wide[..., 2:], pool, torch.float64, teacher_channels=Ct)
    c = pr.pa_ref(s, wide[..., 2:2 + Ct], pool, torch.float64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_dead_nodes_get_no_gradient_and_no_similarity():
    shape = (2, 6, 4, 6, 7, 2)
    dead = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1),          # the whole window of node 0 of image 0
            (1, 4, 6), (1, 5, 6)]                                # ... and the clipped last node of image 1
    s, t = _pair(shape, dead=dead)
    assert pr.assert_nodes_clear_of_threshold(s, 2) == 2
    loss, grad = pr.pa_ref(s, t, 2, torch.float64)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    for n, y, x in dead:
        assert float(grad[n, :, y, x].abs().max()) == 0.0
    assert float(grad[0, :, 2:, :].abs().max()) > 0
    # the live nodes see the dead one as a zero row and column: the smooth variant with a tiny eps agrees on them
    want, gwant = pr.pa_autograd(s, t, 2, torch.float64, eps=1e-30)
    assert abs(float(loss) - float(want)) <= 1e-13
    live = torch.ones_like(grad, dtype=torch.bool)
    for n, y, x in dead:
        live[n, :, y, x] = False
    assert float((grad - gwant)[live].norm()) <= 1e-13 * float(gwant.norm())
    # a node below the threshold but not zero is dead as well: 1/r never reaches the gradient
    tiny = s.clone()
    tiny[0, :, :2, :2] = 1e-8
    loss2, grad2 = pr.pa_ref(tiny, t, 2, torch.float64)
    assert float(grad2[0, :, :2, :2].abs().max()) == 0.0 and abs(float(loss2) - float(loss)) == 0.0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_same_tensor_gives_exactly_zero(dtype):
    s, _ = _pair((2, 7, 7, 6, 5, 2), dead=[(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1)])
    loss, grad = pr.pa_ref(s, s, 2, dtype)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the criterion
def test_criterion_builds_and_refuses():
    from dcfp_amd.loss.criterion import CombinedCriterion, CriterionGsrlDSN, CriterionKD, CriterionKDPairwise, \
        build_criterions
    crit = build_criterions("gsrl,kd,kdpa", _DS(), {"pa_weight": 0.5, "pa_pool": 3, "kd_T": 2.0})
    assert isinstance(crit, CombinedCriterion)
    assert [type(c) for c in crit.criterions] == [CriterionGsrlDSN, CriterionKD, CriterionKDPairwise]
    pa = crit.criterions[2]
    assert (pa.pa_weight, pa.pa_pool) == (0.5, 3)
    alone = build_criterions("kdpa", _DS(), {})
    assert isinstance(alone, CriterionKDPairwise) and (alone.pa_weight, alone.pa_pool) == (1.0, 2)
    with pytest.raises(ValueError, match="pa_weight"):
        build_criterions("kdpa", _DS(), {"pa_weight": -0.1})
    for pool in (0, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="pa_pool"):
            build_criterions("kdpa", _DS(), {"pa_pool": pool})
    z = torch.zeros(2, 19, 9, 9)
    lab = torch.zeros(2, 65, 65, dtype=torch.int64)
    feat = {"ori": lab, "teacher_feat": torch.zeros(2, 8, 9, 9)}
    for call in (lambda l: alone.forward_lowres([z], l, (65, 65), True), lambda l: alone([z], l)):
        with pytest.raises(ValueError, match="attach"):
            call(feat)
    model = _Model()
    assert alone.attach(model) is alone
    for call in (lambda l: alone.forward_lowres([z], l, (65, 65), True), lambda l: alone([z], l)):
        for labels in (lab, {"ori": lab}, {"ori": lab, "teacher": z}):
            with pytest.raises(ValueError, match="teacher_feat"):
                call(labels)
        with pytest.raises(ValueError, match="tap holds no feature"):
            call(feat)
    # attach reaches the criteria of a combination, and a second attach moves the tap
    crit.attach(model)
    assert crit.criterions[2]._tap is not None and not hasattr(crit.criterions[0], "_tap")
    other = _Model()
    alone.attach(other)
    model.train()(torch.zeros(1, 3, 4, 4, requires_grad=True))
    assert alone._tap.pop() is None
    other.train()(torch.zeros(1, 3, 4, 4, requires_grad=True))
    assert alone._tap.pop() is not None


def test_pairwise_kd_loss_has_no_cpu_path_and_checks_pool_first():
    from dcfp_amd import ops
    s, t = _pair((1, 3, 3, 2, 2, 1))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.pairwise_kd_loss(s, t)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.pairwise_kd_loss(s.requires_grad_(True), t.half().permute(0, 2, 3, 1).contiguous(), pool=1)
    assert "kdpa" not in ops.KD_MODES and sorted(ops.KD_MODES) == ["channel", "pixel"]


# ------------------------------------------------------------------------------------------------ the tap
class _Backbone(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 4, 1)

    def forward(self, x):
        y = self.conv(x)
        return y + 1.0, y * 2.0


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = _Backbone()

    def forward(self, x):
        return self.backbone(x)[1].sum()


def test_feature_tap_keeps_the_last_output_of_a_training_forward_only():
    from dcfp_amd.distill import FeatureTap
    model = _Model().train()
    tap = FeatureTap(model)
    x = torch.randn(2, 3, 5, 5)
    assert tap.pop() is None
    out = model(x)
    kept = tap.pop()
    assert kept is not None and kept.requires_grad and tuple(kept.shape) == (2, 4, 5, 5)
    assert torch.equal(kept.detach(), model.backbone.conv(x).detach() * 2.0)       # the LAST element, the graph tensor
    (out + kept.sum()).backward()
    assert tap.pop() is None and tap._kept is None                                  # pop() dropped the reference
    with torch.no_grad():
        model(x)
    assert tap.pop() is None
    model.eval()
    model(x)
    assert tap.pop() is None
    model.train()
    model(x)
    model.eval()
    model(x)                                                                        # a later eval forward clears it
    assert tap.pop() is None
    tap.remove()
    model.train()
    model(x)
    assert tap.pop() is None and len(model.backbone._forward_hooks) == 0
    with pytest.raises(TypeError, match="backbone"):
        FeatureTap(torch.nn.Linear(2, 2))


# ------------------------------------------------------------------------------------------------ the C-ABI
def _ru(v, m):
    return (v + m - 1) // m * m


def _want_bytes(N, Cs, Ct, h, w, pool, grad):
    """the layout include/dcfp_hip.h and DESIGN §19 state: P padded to 128, channels to 32, 256-byte segments; forward:
    both node matrices and scales, the chunk partials (64 channels per chunk) and the loss partials; a gradient adds D,
    and the transposed gradient GEMM result only where it cannot take the teacher's node matrix (Ct narrower than Cs)"""
    P = -(-h // pool) * -(-w // pool)
    Pp, cs, ct = _ru(P, 128), _ru(Cs, 32), _ru(Ct, 32)
    nt = Pp // 128
    segs = [N * cs * Pp, N * Pp, N * ct * Pp, N * Pp, N * max(-(-cs // 64), -(-ct // 64)) * Pp, N * nt * (nt + 1) // 2]
    if grad:
        segs += [N * Pp * Pp] + ([N * cs * Pp] if ct < cs else [])
    return sum(_ru(4 * v, 256) for v in segs)


def test_abi_argument_errors_and_workspace_sizes_need_no_gpu():
    from dcfp_amd import _lib
    L = _lib.lib()
    BAD, WS, UNS = _lib.E_BADDESC, _lib.E_WORKSPACE, _lib.E_UNSUPPORTED
    p = C.c_void_p(4096)                     # never dereferenced: every call below returns before any HIP call

    def fwd(s=p, t=p, layout=0, pitch=0, N=2, Cs=19, Ct=7, h=9, w=9, pool=2, ws=p, nbytes=1 << 30, out=p, grad=0):
        return L.dcfp_pairwise_fwd_f32(s, t, layout, pitch, N, Cs, Ct, h, w, pool, ws, nbytes, out, grad, None)

    def bwd(N=2, Cs=19, Ct=7, h=9, w=9, pool=2, ws=p, nbytes=1 << 30, gout=None, ds=p):
        return L.dcfp_pairwise_bwd_f32(N, Cs, Ct, h, w, pool, ws, nbytes, gout, ds, None)

    assert fwd(s=None) == BAD and fwd(t=None) == BAD and fwd(out=None) == BAD and bwd(ds=None) == BAD
    for key in ("N", "Cs", "Ct", "h", "w", "pool"):
        for call in (fwd, bwd):
            assert call(**{key: 0}) == BAD and call(**{key: -3}) == BAD
    assert fwd(layout=2) == BAD and fwd(layout=-1) == BAD
    assert fwd(layout=1, pitch=6) == BAD                        # a pixel pitch below the channel count
    assert fwd(N=70000) == UNS and bwd(N=70000) == UNS
    for shape in ((2, 19, 7, 9, 9, 2), (2, 7, 19, 9, 9, 2), (1, 1, 1, 1, 1, 1), (3, 2048, 512, 33, 65, 1),
                  (8, 2048, 2048, 97, 97, 2), (1, 33, 64, 5, 4, 7), (1, 130, 67, 7, 5, 2)):
        for grad in (0, 1):
            assert L.dcfp_pairwise_workspace_bytes(*shape, grad) == _want_bytes(*shape, grad), (shape, grad)
    need, need_g = _want_bytes(2, 19, 7, 9, 9, 2, 0), _want_bytes(2, 19, 7, 9, 9, 2, 1)
    assert need_g > need
    assert fwd(nbytes=need - 1) == WS and fwd(ws=None, nbytes=need) == WS
    assert fwd(nbytes=need, grad=1) == WS and fwd(nbytes=need_g - 1, grad=1) == WS
    assert bwd(nbytes=need_g - 1) == WS and bwd(ws=None) == WS
    assert fwd(ws=C.c_void_p(4100)) == WS and bwd(ws=C.c_void_p(4100)) == WS      # not 16-byte aligned
    for bad in ((0, 19, 7, 9, 9, 2), (2, 19, 7, 9, 9, 0), (2, 0, 7, 9, 9, 2), (70000, 19, 7, 9, 9, 2)):
        assert L.dcfp_pairwise_workspace_bytes(*bad, 1) == 0
    # what a gradient costs at the benchmark's shape: D alone, 8 x 2432^2 floats (189 MB) of the 0.51 GB workspace
    assert _want_bytes(8, 2048, 2048, 97, 97, 2, 1) - _want_bytes(8, 2048, 2048, 97, 97, 2, 0) == 4 * 8 * 2432 * 2432


# ------------------------------------------------------------------------------------------------ the driver
@pytest.mark.parametrize("loss_type", ["gsrl,kdpa", "gsrl,kd,kdpa", "ce,kdpa"])
def test_driver_refuses_kdpa_without_a_teacher(monkeypatch, tmp_path, loss_type):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    built = []
    monkeypatch.setattr(train, "build_criterions", lambda *a, **k: built.append(a))
    with pytest.raises(ValueError, match="--teacher-from"):
        train.main(["--loss-type", loss_type, "--ddp", "False", "--snapshot-dir", str(tmp_path / "snap")])
    assert built == [] and not (tmp_path / "snap").exists()      # refused before anything was built or written
    train.check_args(train.get_parser().parse_args(["--loss-type", loss_type, "--teacher-from", "dense.pth"]))
    train.check_args(train.get_parser().parse_args(["--loss-type", "gsrl"]))
