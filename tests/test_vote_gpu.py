"""GPU: ops.multiscale_vote (csrc/vote.hip) and evaluate.predict_vote against the reference's chain in float64
(tests/_vote_ref.py).

Tolerance, per case, from the reference itself on the same inputs: tol = 4 * e_ref + 2^-23 * M (e_ref = max |fp32 chain -
fp64 chain|, M = max |logits|; _vote_ref.tolerance).  Scores lie within tol of float64; pred equals the float64 argmax
wherever the float64 top-two gap exceeds 2 * tol (within tol the order cannot change there), and the pixels left out
are at most 0.5 % of a case; the fused confusion matrix equals ops.confusion_matrix of the kernel's own pred."""
import pytest
import torch

import _vote_ref as vr

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


def labels_for(seed, N, C, out_hw, ignore=255):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, C, (N,) + tuple(out_hw), generator=g)
    gt[torch.rand(gt.shape, generator=g) < 0.1] = ignore
    return gt


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
    err = float((scores.double().cpu() - truth).abs().max())
    top = truth.topk(2, dim=1).values
    decided = (top[:, 0] - top[:, 1]) > 2 * tol
    left_out = 1.0 - float(decided.float().mean())
    wrong = int((pred.cpu().long() != truth.argmax(1))[decided].sum())
    print(f"{tag}: e_ref {e_ref:.3e} M {M:.2f} tol {tol:.3e} kernel err {err:.3e} left out {left_out:.5f} wrong {wrong}")
    assert tuple(scores.shape) == (N, C) + crop and tuple(pred.shape) == (N,) + crop and pred.dtype == torch.int32
    assert err <= tol
    assert wrong == 0
    assert left_out <= 0.005
    assert torch.equal(conf, ops.confusion_matrix(pred, gt, C))
    assert int(conf.sum()) == int((gt != 255).sum())
    # pred alone: the same launch with fewer outputs
    pred2, none = ops.multiscale_vote(vr.to_maps(passes, cuda), grid, crop, align)
    assert none is None and torch.equal(pred2, pred)


@pytest.fixture(scope="module")
def small(cuda):
    N, C, grid, crop = 2, 19, (17, 25), (15, 22)
    passes = vr.make_passes(5, N, C, grid, (0.75, 1.0), True)
    return N, C, grid, crop, vr.to_maps(passes, cuda)


def test_all_ignore_leaves_conf_unchanged(small, cuda):
    from dcfp_amd import ops
    N, C, grid, crop, maps = small
    conf = torch.arange(C * C, dtype=torch.int64, device=cuda).view(C, C).contiguous()
    before = conf.clone()
    gt = torch.full((N,) + crop, 255, dtype=torch.int64, device=cuda)
    ops.multiscale_vote(maps, grid, crop, True, labels=gt, conf=conf)
    assert torch.equal(conf, before)


def test_labels_outside_the_classes_are_skipped(small, cuda):
    from dcfp_amd import ops
    N, C, grid, crop, maps = small
    gt = labels_for(3, N, C, crop)
    g = torch.Generator().manual_seed(4)
    r = torch.rand(gt.shape, generator=g)
    gt[r < 0.1] = C            # no class, not ignore
    gt[(r >= 0.1) & (r < 0.2)] = 254
    gt[(r >= 0.2) & (r < 0.3)] = -1
    gt = gt.to(cuda)
    conf = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    pred, _ = ops.multiscale_vote(maps, grid, crop, True, labels=gt, conf=conf)
    assert int(conf.sum()) == int(((gt >= 0) & (gt < C)).sum())
    assert torch.equal(conf, ops.confusion_matrix(pred, gt, C))
    # another ignore index: 255 then counts as out of range, the chosen one is skipped
    conf3 = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    ops.multiscale_vote(maps, grid, crop, True, labels=gt, conf=conf3, ignore_index=3)
    assert int(conf3.sum()) == int(((gt >= 0) & (gt < C) & (gt != 3)).sum())


def test_two_calls_accumulate_and_repeat_bit_for_bit(small, cuda):
    from dcfp_amd import ops
    N, C, grid, crop, maps = small
    gt = labels_for(9, N, C, crop).to(cuda)
    conf = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    pred1, scores1 = ops.multiscale_vote(maps, grid, crop, True, labels=gt, conf=conf, want_scores=True)
    once = conf.clone()
    pred2, scores2 = ops.multiscale_vote(maps, grid, crop, True, labels=gt, conf=conf, want_scores=True)
    assert torch.equal(conf, 2 * once)
    assert torch.equal(pred1, pred2) and torch.equal(scores1.view(torch.int32), scores2.view(torch.int32))
    fresh = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    ops.multiscale_vote(maps, grid, crop, True, labels=gt, conf=fresh, want_pred=False)
    assert torch.equal(fresh, once)


def test_vote_argument_checks(small, cuda):
    from dcfp_amd import ops
    N, C, grid, crop, maps = small
    with pytest.raises(RuntimeError):
        ops.multiscale_vote([], grid, crop, True)
    with pytest.raises(RuntimeError):
        ops.multiscale_vote(maps * 5, grid, crop, True)                     # 20 maps
    with pytest.raises(RuntimeError):
        ops.multiscale_vote(maps, grid, (grid[0] + 1, grid[1]), True)
    with pytest.raises(RuntimeError):
        ops.multiscale_vote(maps, grid, crop, True, conf=torch.zeros((C, C), dtype=torch.int64, device=cuda))
    with pytest.raises(RuntimeError):
        ops.multiscale_vote([(maps[0][0].cpu(),) + maps[0][1:]], grid, crop, True)
    with pytest.raises(RuntimeError):
        ops.multiscale_vote(maps, grid, crop, True, want_pred=False)


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
    err = float((scores.double().cpu() - truth).abs().max())
    top = truth.topk(2, dim=1).values
    decided = (top[:, 0] - top[:, 1]) > 2 * tol
    left_out = 1.0 - float(decided.float().mean())
    print(f"predict_vote frozen={frozen}: e_ref {e_ref:.3e} M {M:.3e} tol {tol:.3e} err {err:.3e} left out {left_out:.5f}")
    assert err <= tol
    assert bool((pred.cpu().long() == truth.argmax(1))[decided].all())
    assert left_out <= 0.005
