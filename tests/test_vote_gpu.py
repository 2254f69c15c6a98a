"""GPU: ops.multiscale_vote (csrc/vote.hip) and evaluate.predict_vote against the reference's chain in float64
(tests/_vote_ref.py).

Tolerance, per case, from the reference itself on the same inputs: tol = 4 * e_ref + 2^-23 * M (e_ref = max |fp32 chain -
fp64 chain|, M = max |logits|; _vote_common.tolerance_of).  Scores lie within tol of float64; pred equals the float64
argmax wherever the float64 top-two gap exceeds 2 * tol (within tol the order cannot change there), and the pixels left
out are at most 0.5 % of a case (_vote_common.held_to_truth); the fused confusion matrix equals ops.confusion_matrix of
the kernel's own pred.  The behaviour both votes share (labels, accumulation, refused arguments):
tests/test_vote_shared_gpu.py."""
import pytest
import torch

import _vote_ref as vr
from _vote_common import held_to_truth, labels_for

pytestmark = pytest.mark.gpu

#         tag: (N, C, grid, crop, align, scales, flip)
CASES = {
    "recipe": (2, 19, (65, 97), (60, 90), True, vr.SIX_SCALES, True),
    "align_false": (1, 19, (64, 96), (64, 96), False, (0.5, 1.0, 1.75), True),
    "one_map_align": (2, 19, (33, 41), (33, 41), True, (1.0,), False),
    "one_map_noalign": (2, 19, (33, 41), (33, 41), False, (1.0,), False),
    "c150": (1, 150, (33, 41), (33, 41), True, (0.75, 1.25), False),
    "c2": (2, 2, (33, 41), (30, 37), True, (0.75, 1.0), True),
    "lowres_1x1": (2, 19, (9, 9), (9, 9), True, (0.5,), False),
    "crop_1x1": (2, 19, (17, 25), (1, 1), True, (0.75, 1.0), True),
    "out_w3": (1, 19, (3, 4), (3, 3), True, (1.0, 1.5), True),
    "out_w5": (1, 19, (3, 6), (3, 5), False, (1.0, 1.5), True),
    "out_w300": (1, 19, (3, 301), (3, 300), True, (1.0, 1.5), True),
    "maps16": (1, 19, (17, 25), (17, 25), True, (0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0, 2.25), True),
}


@pytest.mark.parametrize("tag", list(CASES))
def test_vote_against_float64(tag, cuda):
    from dcfp_amd import ops
    N, C, grid, crop, align, scales, flip = CASES[tag]
    passes = vr.make_passes(1000 + list(CASES).index(tag), N, C, grid, scales, flip)
    truth, tol, e_ref, M = vr.tolerance(passes, grid, crop, align)
    gt = labels_for(7, N, C, crop).to(cuda)
    conf = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    pred, scores = ops.multiscale_vote(vr.to_maps(passes, cuda), grid, crop, align, labels=gt, conf=conf,
                                       want_scores=True)
    assert tuple(scores.shape) == (N, C) + crop and tuple(pred.shape) == (N,) + crop and pred.dtype == torch.int32
    held_to_truth(tag, scores, pred, truth, tol, e_ref, M)
    assert torch.equal(conf, ops.confusion_matrix(pred, gt, C))
    assert int(conf.sum()) == int((gt != 255).sum())
    # pred alone: the same launch with fewer outputs
    pred2, none = ops.multiscale_vote(vr.to_maps(passes, cuda), grid, crop, align)
    assert none is None and torch.equal(pred2, pred)


class _Recorder:
    """A network that keeps the low-resolution logits it handed out."""

    def __init__(self, net):
        self.net, self.align_corner, self.seen = net, net.align_corner, []

    def lowres_logits(self, image):
        out = self.net.lowres_logits(image)
        self.seen.append(out[0].detach().clone())
        return out


@pytest.fixture(scope="module")
def simple_r50(cuda):
    import _model_cases as mc
    from oracle import fill
    from dcfp_amd import deploy
    model = mc.build_model("simple", "resnet50", True, torch.device("cpu"), criterion=False, deepsup=False).eval()
    engine = deploy.build_engine(model).to(cuda)          # frozen from the host copy, as tools/evaluate.py does
    return model.to(cuda), engine, fill.closed_form_input(2, 65, 97).to(cuda)


@pytest.mark.parametrize("frozen", [False, True], ids=["model", "engine"])
def test_predict_vote_on_a_network(frozen, simple_r50, cuda):
    from dcfp_amd import evaluate as ev
    model, engine, image = simple_r50
    net = _Recorder(engine if frozen else model)
    scales, crop = (0.75, 1.0, 1.25), (60, 90)
    pred, scores = ev.predict_vote(net, image, scales, True, True, out_hw=crop, want_scores=True)
    assert len(net.seen) == 6
    H, W = image.shape[2:]
    passes = [((int(H * s), int(W * s)), net.seen[2 * i].cpu(), net.seen[2 * i + 1].cpu()) for i, s in enumerate(scales)]
    truth, tol, e_ref, M = vr.tolerance(passes, (H, W), crop, True)
    held_to_truth(f"predict_vote frozen={frozen}", scores, pred, truth, tol, e_ref, M)
