"""GPU: ops.gather_tiles / ops.sliding_vote (csrc/slide.hip), evaluate.predict_sliding_vote and the fused sliding branch
of tools/evaluate.py's predict_batch against the reference's sliding-window chain in float64 (tests/_slide_ref.py).

Tolerance, per case, from the reference itself on the same inputs: tol = 4 * e_ref + 2^-23 * M (e_ref = max |fp32 chain -
fp64 chain|, M = max |logits|; _vote_common.tolerance_of).  Scores lie within tol of float64; pred equals the float64
argmax wherever the float64 top-two gap exceeds 2 * tol, and the pixels left out are at most 0.5 % of a case
(_vote_common.held_to_truth); the fused confusion matrix equals ops.confusion_matrix of the kernel's own pred.  The
behaviour both votes share (labels, accumulation, refused arguments): tests/test_vote_shared_gpu.py.

The stride comes from the tile height as the reference computes it, ceil(th * (1 - 1/3)) in double precision: 12 for
17, 23 for 33 and 7 for 9 (9 * (1 - 1/3) is 6.000000000000001)."""
import argparse
import os

import pytest
import torch

import _slide_ref as sr
from _vote_common import held_to_truth, labels_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

#         tag: (N, C, grid, crop, tile, align, scales, flip)
CASES = {
    "triple_rows": (2, 19, (33, 41), (33, 41), (17, 17), True, (1.0,), False),
    "wide_tile": (1, 19, (20, 60), (20, 60), (9, 25), True, (1.0,), False),
    "image_in_tile": (2, 19, (20, 30), (20, 30), (33, 33), True, (1.0,), True),
    "one_tile_exact": (1, 19, (17, 17), (17, 17), (17, 17), True, (1.0,), False),
    "ms_flip": (2, 19, (33, 41), (30, 37), (17, 17), True, (0.75, 1.0, 1.25), True),
    "six_scales": (1, 19, (33, 41), (33, 41), (17, 25), True, sr.SIX_SCALES, True),
    "align_false": (1, 19, (32, 48), (32, 48), (17, 17), False, (0.5, 1.0, 1.75), True),
    "c171": (1, 171, (33, 41), (33, 41), (17, 17), True, (0.75, 1.25), False),
    "c2": (2, 2, (33, 41), (30, 37), (17, 17), True, (0.75, 1.0), True),
    "crop_1x1": (1, 19, (33, 41), (1, 1), (17, 17), True, (1.0, 1.5), True),
}


@pytest.mark.parametrize("tag", list(CASES))
def test_sliding_vote_against_float64(tag, cuda):
    from dcfp_amd import ops
    N, C, grid, crop, tile, align, scales, flip = CASES[tag]
    passes = sr.make_passes(2000 + list(CASES).index(tag), N, C, grid, tile, scales, flip)
    truth, tol, e_ref, M = sr.tolerance(passes, grid, crop, tile, align)
    gt = labels_for(7, N, C, crop).to(cuda)
    conf = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    dev_passes = sr.to_passes(passes, grid, tile, cuda)
    pred, scores = ops.sliding_vote(dev_passes, grid, crop, align, labels=gt, conf=conf, want_scores=True)
    assert tuple(scores.shape) == (N, C) + crop and tuple(pred.shape) == (N,) + crop and pred.dtype == torch.int32
    held_to_truth(tag, scores, pred, truth, tol, e_ref, M)
    assert torch.equal(conf, ops.confusion_matrix(pred, gt, C))
    assert int(conf.sum()) == int((gt != 255).sum())
    # pred alone: the same launch with fewer outputs
    pred2, none = ops.sliding_vote(dev_passes, grid, crop, align)
    assert none is None and torch.equal(pred2, pred)
    if tag == "one_tile_exact":     # one tile that is the image: the plain upsample of its logits
        plain = torch.nn.functional.interpolate(passes[0][1][0].double(), grid, mode="bilinear", align_corners=True)
        assert float((scores.double().cpu() - plain).abs().max()) <= tol


def torch_tiles(image, tile, flip):
    from dcfp_amd import evaluate as ev
    src = torch.flip(image, [3]) if flip else image
    boxes = sr.reference_tiles(image.shape[2], image.shape[3], tile)[0]
    return torch.stack([ev.pad(src[:, :, y1:y2, x1:x2], tile) for y1, y2, x1, x2 in boxes])


@pytest.mark.parametrize("hw,tile", [((33, 41), (17, 17)), ((20, 30), (33, 33)), ((20, 61), (9, 25))])
@pytest.mark.parametrize("flip", [False, True])
def test_gather_tiles_is_the_slicing_chain(hw, tile, flip, cuda):
    from dcfp_amd import evaluate as ev, ops
    g = torch.Generator().manual_seed(11)
    image = torch.randn((2, 3) + hw, generator=g).to(cuda)
    ys, xs = ev.sliding_tiles(hw[0], hw[1], tile)
    got = ops.gather_tiles(image, ys, xs, tile, flip)
    want = torch_tiles(image, tile, flip)
    assert tuple(got.shape) == (len(ys) * len(xs), 2, 3) + tile
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


class _Recorder:
    """A network that keeps the stacked low-resolution logits it handed out."""

    def __init__(self, net):
        self.net, self.align_corner, self.seen = net, net.align_corner, []

    def lowres_logits(self, image):
        out = self.net.lowres_logits(image)
        self.seen.append(out[0].detach().clone())
        return out

    def __call__(self, image):
        return self.net(image)


@pytest.fixture(scope="module")
def simple_r50(cuda):
    import _model_cases as mc
    from oracle import fill
    from dcfp_amd import deploy
    model = mc.build_model("simple", "resnet50", True, torch.device("cpu"), criterion=False, deepsup=False).eval()
    engine = deploy.build_engine(model).to(cuda)          # frozen from the host copy, as tools/evaluate.py does
    return model.to(cuda), engine, fill.closed_form_input(2, 65, 97).to(cuda)


def recorded_passes(seen, N, image_hw, tile, scales, flip):
    """The recorder's calls (any chunking), cut back into (scale, plain [T,N,C,lh,lw], mirrored) per scale."""
    from dcfp_amd import evaluate as ev
    flat = torch.cat([s.cpu() for s in seen])              # [sum of T * N, C, lh, lw], tiles outermost
    passes, at = [], 0
    for s in scales:
        ys, xs = ev.sliding_tiles(int(image_hw[0] * s), int(image_hw[1] * s), tile)
        T = len(ys) * len(xs)
        both = []
        for _ in range(2 if flip else 1):
            both.append(flat[at:at + T * N].reshape((T, N) + tuple(flat.shape[1:])))
            at += T * N
        passes.append((float(s), both[0], both[1] if flip else None))
    assert at == flat.shape[0]
    return passes


@pytest.mark.parametrize("frozen", [False, True], ids=["model", "engine"])
def test_predict_sliding_vote_on_a_network(frozen, simple_r50, cuda):
    from dcfp_amd import evaluate as ev
    model, engine, image = simple_r50
    scales, crop, tile = (0.75, 1.0), (60, 90), (33, 33)
    H, W = image.shape[2:]
    logits = {}
    for tile_batch in (1, 1000):
        net = _Recorder(engine if frozen else model)
        pred, scores = ev.predict_sliding_vote(net, image, tile, scales, True, True, out_hw=crop, want_scores=True,
                                               tile_batch=tile_batch)
        passes = recorded_passes(net.seen, image.shape[0], (H, W), tile, scales, True)
        n_tiles = sum(p[1].shape[0] * 2 for p in passes)
        assert len(net.seen) == (n_tiles if tile_batch == 1 else 2 * len(scales))
        truth, tol, e_ref, M = sr.tolerance(passes, (H, W), crop, tile, True)
        held_to_truth(f"predict_sliding_vote frozen={frozen} tile_batch={tile_batch}", scores, pred, truth, tol, e_ref, M)
        logits[tile_batch] = torch.cat([t.flatten() for p in passes for t in p[1:]])
    print("logits per tile vs batched: max |difference| %.3e of max |logits| %.3e"
          % (float((logits[1] - logits[1000]).abs().max()), float(logits[1].abs().max())))


def test_predict_batch_fused_sliding(simple_r50, cuda):
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_tool_for_slide", os.path.join(ROOT, "tools", "evaluate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from dcfp_amd import ops
    model, _, image = simple_r50
    C, (H, W), scales = 19, tuple(image.shape[2:]), [0.75, 1.0]
    args = argparse.Namespace(input_size="33,33", whole=False, fused_sliding=True, num_classes=C, longsize=-1,
                              shortsize=-1, align_corner=True, flip=True, ignore_label=255)
    label = labels_for(21, image.shape[0], C, (H, W)).to(cuda)
    conf = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    net = _Recorder(model)
    pred, counted, seconds, in_shape = tool.predict_batch(net, image, args, scales, True, (H, W), label, conf)
    assert counted is True and tuple(pred.shape) == (image.shape[0], H, W) and in_shape == tuple(image.shape)
    assert torch.equal(conf, ops.confusion_matrix(pred, label, C))
    passes = recorded_passes(net.seen, image.shape[0], (H, W), (33, 33), scales, True)
    _, tol, _, _ = sr.tolerance(passes, (H, W), (H, W), (33, 33), True)
    # the chain of the flag's other setting, on the same model
    args.fused_sliding = False
    conf_chain = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    pred_chain, counted_chain, _, _ = tool.predict_batch(model, image, args, scales, True, (H, W), label, conf_chain)
    assert counted_chain is False and int(conf_chain.sum()) == 0
    from dcfp_amd import evaluate as ev
    chain_logits = ev.predict_multiscale(model, image, (33, 33), scales, C, True, True, False)
    top = chain_logits.topk(2, dim=1).values
    decided = (top[:, 0] - top[:, 1]) > 2 * tol
    print("predict_batch: tol %.3e, decided %.5f, disagreeing decided pixels %d"
          % (tol, float(decided.float().mean()), int((pred != pred_chain)[decided].sum())))
    assert bool((pred == pred_chain)[decided].all())
