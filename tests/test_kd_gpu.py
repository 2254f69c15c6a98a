"""ops.kd_loss (dcfp_amd/csrc/kd.hip) against the fp64 reference of tests/_kd_ref.py, both modes.

Shapes come from the kernels' geometry.  pixel: a lane owns a pixel, a block is 64 pixels x K waves that share the
classes; up to 32 classes run 4 waves x 8 classes in registers, up to 192 run 8 waves x 24, more run 8 waves of an
online softmax that reads twice - so one class and two (waves without a class), 19, the 32 / 33 and 192 / 193
thresholds, 59 / 150 / 171, widths that are no multiple of 64, a block that straddles two images, one pixel, several
blocks and a partial last one.  channel: a 1024-thread block owns a row of h*w floats - rows of 1, 63 / 64 / 65 (one
wave, partly idle), 7*15, 33*65 (three trips of the row loop, the last partial) and 129*257 (33 trips: the row that
cannot be held on chip).

Tolerance: the rule of tests/test_loss_eval_kernels_gpu.py with its floors (tests/_kd_ref.py): distance to fp64 at most
max(floor, 3 x the distance of the same formula in fp32), relative for the loss, norm-relative for the gradient."""
import os
import random
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kd_ref as kr  # noqa: E402

pytestmark = pytest.mark.gpu

TEMPS = [1.0, 4.0]
PIXEL_SHAPES = [
    (1, 1, 3, 5),          # one class: loss and gradient are zero
    (1, 2, 1, 1),          # one pixel
    (2, 19, 7, 15),
    (2, 19, 9, 17),        # 153 pixels per image: the third wave holds pixels of both images
    (1, 59, 5, 67),        # width not a multiple of 64
    (2, 150, 3, 5),
    (2, 171, 8, 16),
    (3, 19, 1, 130),       # one row, a partial last wave
    (1, 32, 3, 5),         # the last class count of the 4-wave kernel ...
    (1, 33, 3, 5),         # ... and the first of the 8-wave one
    (1, 192, 3, 5),        # the last class count held in registers ...
    (2, 193, 5, 13),       # ... and the first that is streamed twice (65 pixels per image: two blocks, two images in one)
]
CHANNEL_SHAPES = [
    (2, 2, 1, 1),          # rows of one element: zero
    (1, 19, 7, 9),         # 63
    (2, 2, 8, 8),          # 64
    (1, 19, 5, 13),        # 65
    (2, 19, 7, 15),
    (2, 2, 33, 65),
    (1, 19, 33, 65),
    (1, 2, 129, 257),      # the 1025 x 2049 crop's row: 33 153 floats, more than LDS holds next to the teacher's
]

_REFS = {}


def _sid(shape):
    return "x".join(map(str, shape))


def _case(shape, mode, T, scale=2.5):
    """(student, teacher, fp64 (loss, grad), fp32 (loss, grad)) on the CPU, computed once per case and left unchanged."""
    key = (shape, mode, T, scale)
    if key not in _REFS:
        s, t = kr.logits(shape, random.Random(repr(key)).getrandbits(31))
        if scale != 2.5:                       # the largest |logit| becomes `scale`
            s, t = s * (scale / s.abs().max()), t * (scale / t.abs().max())
        _REFS[key] = (s, t, kr.kd_ref(s, t, T, mode, torch.float64), kr.kd_ref(s, t, T, mode, torch.float32))
    return _REFS[key]


def _run(cuda, s, t, T, mode, gout=None):
    from dcfp_amd import ops
    sd = s.to(cuda).requires_grad_(True)
    td = t.to(cuda)
    loss = ops.kd_loss(sd, td, T=T, mode=mode)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    if gout is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(gout, device=cuda))
    return loss.detach().cpu(), sd.grad.detach().cpu()


def _check(cuda, shape, mode, T, scale=2.5):
    s, t, ref64, ref32 = _case(shape, mode, T, scale)
    loss, grad = _run(cuda, s, t, T, mode)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    kr.check(f"kd_{mode}", f"{_sid(shape)}-T{T:g}" + ("" if scale == 2.5 else f"-max{scale:g}"), loss, grad, ref64, ref32)
    return loss, grad


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("shape", PIXEL_SHAPES, ids=_sid)
def test_pixel(cuda, shape, T):
    loss, grad = _check(cuda, shape, "pixel", T)
    if shape[1] == 1:
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("shape", CHANNEL_SHAPES, ids=_sid)
def test_channel(cuda, shape, T):
    loss, grad = _check(cuda, shape, "channel", T)
    if shape[2] * shape[3] == 1:
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize("mode,shape", [("pixel", (2, 19, 9, 17)), ("pixel", (2, 59, 9, 17)), ("pixel", (1, 200, 3, 5)),
                                        ("channel", (2, 19, 33, 65))],
                         ids=["pixel-4x8", "pixel-8x24", "pixel-stream", "channel"])
def test_logits_of_80_stay_finite(cuda, mode, shape):
    """|logits| up to 80 at T = 1: exponents down to -160, probabilities that underflow to zero"""
    _check(cuda, shape, mode, 1.0, scale=80.0)


BOTH = [("pixel", (2, 19, 9, 17)), ("pixel", (2, 59, 5, 67)), ("pixel", (1, 200, 3, 5)), ("channel", (2, 19, 33, 65))]
BOTH_IDS = ["pixel-4x8", "pixel-8x24", "pixel-stream", "channel"]


@pytest.mark.parametrize("mode,shape", BOTH, ids=BOTH_IDS)
def test_two_calls_give_identical_bits(cuda, mode, shape):
    s, t, _, _ = _case(shape, mode, 4.0)
    a, b = _run(cuda, s, t, 4.0, mode), _run(cuda, s, t, 4.0, mode)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("mode,shape", BOTH, ids=BOTH_IDS)
def test_backward_scales_by_grad_output(cuda, mode, shape):
    s, t, _, _ = _case(shape, mode, 4.0)
    _, g1 = _run(cuda, s, t, 4.0, mode)
    _, g = _run(cuda, s, t, 4.0, mode, gout=0.37)
    assert torch.equal(g, g1 * torch.tensor(0.37))


@pytest.mark.parametrize("mode,shape", BOTH, ids=BOTH_IDS)
def test_teacher_equal_to_student(cuda, mode, shape):
    """loss and gradient are zero: their absolute distance to 0 against that of the formula in fp32"""
    s, _, _, _ = _case(shape, mode, 1.0)
    t = s.clone()
    loss, grad = _run(cuda, s, t, 1.0, mode)
    l32, g32 = kr.kd_ref(s, t, 1.0, mode, torch.float32)
    case = f"{_sid(shape)}-T1-teacher=student"
    kr.held(f"kd_{mode}", case, "loss", abs(float(loss)), abs(float(l32)), kr.CE_FLOOR)
    kr.held(f"kd_{mode}", case, "dlogits", float(grad.double().norm()), float(g32.double().norm()), kr.CE_GFLOOR)


@pytest.mark.parametrize("mode,shape", BOTH, ids=BOTH_IDS)
def test_teacher_untouched_and_without_gradient(cuda, mode, shape):
    from dcfp_amd import ops
    s, t, _, _ = _case(shape, mode, 1.0)
    sd, td = s.to(cuda).requires_grad_(True), t.to(cuda)
    before = td.clone()
    ops.kd_loss(sd, td, mode=mode).backward()
    assert torch.equal(td, before) and td.grad is None and torch.equal(sd.detach().cpu(), s)
    with pytest.raises(RuntimeError, match="teacher"):
        ops.kd_loss(sd, td.clone().requires_grad_(True), mode=mode)
    with torch.no_grad():                              # no gradient wanted: the loss alone, same bits
        alone = ops.kd_loss(sd.detach(), td, mode=mode)
    assert torch.equal(alone, ops.kd_loss(sd, td, mode=mode).detach())


@pytest.mark.parametrize("mode,shape", BOTH, ids=BOTH_IDS)
def test_non_contiguous_student(cuda, mode, shape):
    from dcfp_amd import ops
    s, t, _, _ = _case(shape, mode, 1.0)
    N, Cc, h, w = shape
    wide = torch.zeros(N, Cc, h, 2 * w, device=cuda)
    wide[..., ::2] = s.to(cuda)
    view = wide[..., ::2].requires_grad_(True)
    assert not view.is_contiguous()
    loss = ops.kd_loss(view, t.to(cuda), mode=mode)
    loss.backward()
    want_loss, want_grad = _run(cuda, s, t, 1.0, mode)
    assert torch.equal(loss.detach().cpu(), want_loss) and torch.equal(view.grad.cpu(), want_grad)


def test_argument_errors(cuda):
    from dcfp_amd import ops
    s, t = (v.to(cuda) for v in kr.logits((2, 3, 4, 5), 1))
    with pytest.raises(RuntimeError, match="same"):
        ops.kd_loss(s, t[:, :2])
    with pytest.raises(RuntimeError, match="float32"):
        ops.kd_loss(s, t.double())
    with pytest.raises(RuntimeError, match="float32"):
        ops.kd_loss(s.half(), t)
    with pytest.raises(ValueError, match="mode"):
        ops.kd_loss(s, t, mode="spatial")
    for T in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            ops.kd_loss(s, t, T=T)
