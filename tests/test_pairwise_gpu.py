"""ops.pairwise_kd_loss (dcfp_amd/csrc/pairwise.hip) against the fp64 reference of tests/_pa_ref.py.

Shapes (N, Cs, Ct, h, w, pool) come from the kernels' geometry.  The matrix kernels work on 32 x 32 MFMA tiles, four
waves of 2 x 2 of them per 128-node block tile, node columns padded to 128 and channels to the K loop's block of 32; the
fp32 node kernel and the dot kernel give a lane a node (64 per block) and a block a chunk of 64 channels split over 8
waves, the chunks' partial sums being added by a reduce kernel; the fp16-NHWC node kernel takes 32 nodes and a chunk of
64 channels per block; the gradient GEMM tiles the student's channels by 128.  So: P = 1
(h = w = 1 and pool > h), 31 / 32 / 33, 65, 127 / 128 / 129 (one block tile, and the first pair of tiles: mirror write
and the double count), 289 and 306 (three tiles per side: six tile pairs); channels 1, 2, 3 (waves without a channel),
31 / 32 / 33, 64 (one chunk), 67 and 70 (a second, partial chunk), 130 (a third chunk; a second, partly empty row tile
of the gradient GEMM) and 2048 (32 chunks); Cs != Ct both ways - wider, where the GEMM's result takes the teacher's node
matrix's place in the workspace, and narrower, where it has a place of its own -; pool
1, 2, 3 on maps that are no multiple of it; N = 1, 2, 3.  The kernels add no threshold that picks another code path
besides the teacher's layout.

Inputs are post-ReLU randn; in every image of the student (where it has more than one node) the first and the last node
are set exactly to zero, and every other node norm - student and teacher - is at least 1e-3 (asserted on the CPU: rounding
cannot move a node across the dead-node threshold; with one to three channels the seed is advanced until that holds).

Tolerance: the rule of tests/test_loss_eval_kernels_gpu.py / test_kd_gpu.py with their floors (tests/_pa_ref.py): distance
to fp64 at most max(floor, 3 x the distance of the same formula in fp32), relative for the loss (floor 3e-6),
norm-relative for the gradient (floor 3e-5)."""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pa_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [
    # node counts
    (1, 3, 3, 1, 1, 1),            # h = w = 1: one node
    (2, 5, 5, 2, 3, 4),            # pool > h and > w: one node
    (1, 4, 4, 1, 31, 1),
    (2, 4, 6, 4, 8, 1),            # P = 32
    (1, 6, 4, 3, 11, 1),           # 33
    (1, 5, 5, 5, 13, 1),           # 65: a second block of the node kernel
    (1, 3, 3, 1, 127, 1),
    (1, 3, 5, 8, 16, 1),           # 128: the last single block tile ...
    (1, 3, 3, 3, 43, 1),           # ... 129: tiles (0,0), (0,1), (1,1)
    (2, 7, 5, 17, 17, 1),          # 289: three tiles per side
    (1, 8, 8, 33, 35, 2),          # 17 x 18 = 306 nodes from clipped windows
    # channel counts
    (2, 1, 2, 5, 5, 2),
    (1, 2, 1, 5, 5, 2),
    (1, 3, 64, 6, 7, 2),
    (2, 64, 3, 6, 7, 2),
    (1, 67, 31, 5, 5, 3),
    (1, 32, 33, 5, 5, 3),
    (1, 130, 67, 7, 5, 2),
    (1, 2048, 64, 9, 9, 2),
    (1, 64, 2048, 9, 9, 2),
    # pooling windows and batch
    (2, 5, 5, 7, 9, 2),
    (3, 5, 7, 7, 8, 3),
    (3, 9, 9, 10, 11, 1),
]
# the teacher as the engine holds it: (shape, pixel pitch, channel offset)
F16_CASES = [
    ((2, 5, 6, 7, 9, 2), 16, 3),
    ((1, 4, 70, 6, 11, 1), 80, 8),          # 66 nodes: three blocks of the NHWC node kernel, the last partial; 64 + 6 channels
    ((1, 64, 67, 5, 5, 3), 67, 0),          # pitch == Ct
    ((1, 64, 2048, 9, 9, 2), 2056, 5),
    ((3, 3, 1, 1, 1, 1), 9, 4),
]
BOTH = [(2, 7, 5, 17, 17, 1), (2, 64, 3, 6, 7, 2), (1, 130, 67, 7, 5, 2)]

_REFS = {}


def _sid(shape):
    return "x".join(map(str, shape))


def _one_node(shape):
    return -(-shape[3] // shape[5]) * -(-shape[4] // shape[5]) == 1


def _kill(x, pool):
    """zero the first and the last node of every image (maps with more than one node)"""
    N, _, h, w = x.shape
    hp, wp = -(-h // pool), -(-w // pool)
    if hp * wp > 1:
        x[:, :, :pool, :pool] = 0.0
        x[:, :, (hp - 1) * pool:, (wp - 1) * pool:] = 0.0
    return 2 * N if hp * wp > 1 else 0


def _inputs(shape, scale, f16):
    N, Cs, Ct, h, w, pool = shape
    seed = random.Random(repr((shape, scale, f16))).getrandbits(31)
    for attempt in range(200):
        s, t = pr.features((N, Cs, h, w), (N, Ct, h, w), seed + attempt, scale=scale)
        if f16:
            t = t.half().float()
        killed = _kill(s, pool)
        try:
            dead = pr.assert_nodes_clear_of_threshold(s, pool)
            pr.assert_nodes_clear_of_threshold(t, pool)
        except AssertionError:
            assert min(Cs, Ct) <= 3, "only one to three channels may need another draw"
            continue
        assert dead >= killed
        return s, t
    raise AssertionError(f"no draw of {shape} keeps its nodes clear of the threshold")


def _case(shape, scale=1.0, f16=None):
    """(student, teacher, fp64 (loss, grad), fp32 (loss, grad)) on the CPU, computed once per case and left unchanged.
    f16 = (pitch, offset): the teacher is the fp16 [N,h,w,pitch - offset] view of a NaN-filled NHWC buffer."""
    key = (shape, scale, f16)
    if key not in _REFS:
        s, t = _inputs(shape, scale, f16 is not None)
        N, Cs, Ct, h, w, pool = shape
        if f16 is not None:
            pitch, off = f16
            buf = torch.full((N, h, w, pitch), float("nan"), dtype=torch.float16)
            buf[..., off:off + Ct] = t.permute(0, 2, 3, 1).half()
            t = buf[..., off:]
            assert bool(torch.isnan(t).any()) == (pitch - off > Ct)
        ch = Ct if f16 is not None else None
        _REFS[key] = (s, t, pr.pa_ref(s, t, pool, torch.float64, ch), pr.pa_ref(s, t, pool, torch.float32, ch))
    return _REFS[key]


def _teacher_to(cuda, t):
    """an fp16 view travels with its buffer: same pitch, same offset"""
    if t.dtype != torch.float16:
        return t.to(cuda)
    base = t._base if t._base is not None else t
    off = t.storage_offset() - base.storage_offset()
    return base.to(cuda)[..., off:]


def _run(cuda, s, t, shape, gout=None, f16=False):
    from dcfp_amd import ops
    sd = s.to(cuda).requires_grad_(True)
    td = _teacher_to(cuda, t)
    loss = ops.pairwise_kd_loss(sd, td, pool=shape[5], teacher_channels=shape[2] if f16 else None)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    if gout is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(gout, device=cuda))
    return loss.detach().cpu(), sd.grad.detach().cpu()


def _check(cuda, shape, scale=1.0, f16=None, group="pairwise"):
    s, t, ref64, ref32 = _case(shape, scale, f16)
    loss, grad = _run(cuda, s, t, shape, f16=f16 is not None)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    case = _sid(shape) + ("" if scale == 1.0 else f"-x{scale:g}") + ("" if f16 is None else f"-f16p{f16[0]}o{f16[1]}")
    if _one_node(shape):
        # one live node: A = 1 on both sides and the exact gradient is 0, so the fp64 "reference" gradient is rounding
        # noise and a norm-relative figure means nothing.  The gradient's distance to it is held, by the same rule, in
        # units of what one term of the sum is worth: B[n,c,y,x] = 4/(N P^2) / (r_p |window_p|), |D| and |f| being <= 1.
        pr.check(group, case, loss, None, ref64, ref32)
        u, cnt, index = pr.nodes(s.double(), shape[5])
        unit = float((4.0 / s.shape[0] / (u * u).sum(dim=1).sqrt() / cnt[0]).norm()) * (s.shape[1] * s.shape[2] * s.shape[3]) ** 0.5
        pr.held(group, case, "dstudent (of a term's size)", float((grad.double() - ref64[1]).norm()) / unit,
                float((ref32[1].double() - ref64[1]).norm()) / unit, pr.CE_GFLOOR)
    else:
        pr.check(group, case, loss, grad, ref64, ref32)
    # a dead node gets no gradient at all, not a small one
    pool = shape[5]
    u, _, index = pr.nodes(s.double(), pool)
    dead = ((u * u).sum(dim=1) == 0)[:, index.reshape(-1)].reshape(s.shape[0], 1, s.shape[2], s.shape[3])
    assert float((grad * dead).abs().max()) == 0.0
    return loss, grad


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_against_fp64(cuda, shape):
    _check(cuda, shape)


@pytest.mark.parametrize("shape,pitch,off", F16_CASES, ids=[_sid(c[0]) for c in F16_CASES])
def test_f16_nhwc_teacher_with_pitch_offset_and_nan_padding(cuda, shape, pitch, off):
    _check(cuda, shape, f16=(pitch, off), group="pairwise_f16")


@pytest.mark.parametrize("scale", [1e4, 1e-2])
@pytest.mark.parametrize("shape", [(2, 64, 67, 13, 11, 2), (1, 2048, 64, 9, 9, 2)], ids=_sid)
def test_scaled_features(cuda, shape, scale):
    """the loss does not depend on the features' scale; the gradient scales by its inverse"""
    _check(cuda, shape, scale=scale, group="pairwise_scaled")


def test_a_single_dead_node(cuda):
    """h = w = 1 and an all-zero student: A^S = 0, A^T = 1, loss 1, no gradient"""
    from dcfp_amd import ops
    s = torch.zeros(2, 5, 1, 1, device=cuda, requires_grad=True)
    t = torch.rand(2, 3, 1, 1, device=cuda) + 0.5
    loss = ops.pairwise_kd_loss(s, t, pool=1)
    loss.backward()
    assert abs(float(loss) - 1.0) <= 3e-6 and float(s.grad.abs().max()) == 0.0


@pytest.mark.parametrize("shape", BOTH, ids=_sid)
def test_two_calls_give_identical_bits(cuda, shape):
    s, t, _, _ = _case(shape)
    a, b = _run(cuda, s, t, shape), _run(cuda, s, t, shape)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("shape", BOTH, ids=_sid)
def test_backward_scales_by_grad_output(cuda, shape):
    s, t, _, _ = _case(shape)
    _, g1 = _run(cuda, s, t, shape)
    _, g = _run(cuda, s, t, shape, gout=0.37)
    assert torch.equal(g, g1 * torch.tensor(0.37)) and float(g1.abs().max()) > 0


@pytest.mark.parametrize("shape", BOTH + [(1, 2048, 64, 9, 9, 2)], ids=_sid)
def test_teacher_equal_to_student_is_exactly_zero(cuda, shape):
    from dcfp_amd import ops
    s, _, _, _ = _case(shape)
    sd = s.to(cuda).requires_grad_(True)
    for td in (sd.detach(), sd.detach().clone()):                # the same tensor, and the same values elsewhere
        sd.grad = None
        loss = ops.pairwise_kd_loss(sd, td, pool=shape[5])
        loss.backward()
        assert float(loss) == 0.0 and float(sd.grad.abs().max()) == 0.0


@pytest.mark.parametrize("shape", BOTH, ids=_sid)
def test_teacher_untouched_and_without_gradient(cuda, shape):
    from dcfp_amd import ops
    s, t, _, _ = _case(shape)
    sd, td = s.to(cuda).requires_grad_(True), t.to(cuda)
    before = td.clone()
    ops.pairwise_kd_loss(sd, td, pool=shape[5]).backward()
    assert torch.equal(td, before) and td.grad is None and torch.equal(sd.detach().cpu(), s)
    with pytest.raises(RuntimeError, match="teacher"):
        ops.pairwise_kd_loss(sd, td.clone().requires_grad_(True), pool=shape[5])
    with torch.no_grad():                              # no gradient wanted: the loss alone, same bits
        alone = ops.pairwise_kd_loss(sd.detach(), td, pool=shape[5])
    assert alone.dim() == 0 and not alone.requires_grad
    assert torch.equal(alone, ops.pairwise_kd_loss(sd, td, pool=shape[5]).detach())


@pytest.mark.parametrize("shape", BOTH, ids=_sid)
def test_non_contiguous_student(cuda, shape):
    from dcfp_amd import ops
    s, t, _, _ = _case(shape)
    N, Cs, _, h, w, pool = shape
    wide = torch.zeros(N, Cs, h, 2 * w, device=cuda)
    wide[..., ::2] = s.to(cuda)
    view = wide[..., ::2].requires_grad_(True)
    assert not view.is_contiguous()
    loss = ops.pairwise_kd_loss(view, t.to(cuda), pool=pool)
    loss.backward()
    want_loss, want_grad = _run(cuda, s, t, shape)
    assert torch.equal(loss.detach().cpu(), want_loss) and torch.equal(view.grad.cpu(), want_grad)


def test_argument_errors(cuda):
    from dcfp_amd import ops
    s, t = (v.to(cuda) for v in pr.features((2, 3, 4, 5), (2, 6, 4, 5), 1))
    for bad in (t[:1], t[:, :, :3], t[..., :4]):
        with pytest.raises(RuntimeError, match="same N, h, w"):
            ops.pairwise_kd_loss(s, bad)
    with pytest.raises(RuntimeError, match="float32"):
        ops.pairwise_kd_loss(s.half(), t)
    with pytest.raises(RuntimeError, match="float32"):
        ops.pairwise_kd_loss(s, t.double())
    with pytest.raises(RuntimeError, match="4-dimensional"):
        ops.pairwise_kd_loss(s[0], t)
    for pool in (0, -2, 2.0, True, None):
        with pytest.raises(ValueError, match="pool"):
            ops.pairwise_kd_loss(s, t, pool=pool)
    t16 = t.permute(0, 2, 3, 1).contiguous().half()                      # [N,h,w,6]
    for ch in (0, 7):
        with pytest.raises(ValueError, match="teacher_channels"):
            ops.pairwise_kd_loss(s, t16, teacher_channels=ch)
    with pytest.raises(ValueError, match="teacher_channels"):
        ops.pairwise_kd_loss(s, t, teacher_channels=5)
    with pytest.raises(RuntimeError, match="unit stride"):
        ops.pairwise_kd_loss(s, t.half().permute(0, 2, 3, 1))            # NCHW memory seen as NHWC: channel stride h*w
    with pytest.raises(RuntimeError, match="same N, h, w"):
        ops.pairwise_kd_loss(s, t16[:, :3])


def test_report_largest_share_of_the_bound():
    """not a check: prints the largest observed share of the tolerance of this process's comparisons"""
    for what in ("loss", "dstudent"):
        shares = [(v, g, c) for g, c, w, v in pr.SHARES if w == what]
        if shares:
            v, g, c = max(shares)
            print(f"PARITY-SHARE {what}: largest {v:.3f} of the bound ({g} {c}), {len(shares)} comparisons")
