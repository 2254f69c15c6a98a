"""GPU: the behaviour that ops.multiscale_vote (csrc/vote.hip) and ops.sliding_vote (csrc/slide.hip) have from their
shared pixel loop (csrc/vote_core.h) and their shared wrapper (ops._fused_vote): which labels are counted, that the
confusion matrix accumulates, that two calls give the same bits, and which arguments are refused.  Each test runs on
both votes, on a small two-scale + flip geometry of each; what only one vote has is in test_vote_gpu.py and
test_slide_gpu.py."""
import pytest
import torch

from _vote_common import labels_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["whole", "sliding"])
def small(request, cuda):
    """-> (vote, N, C, grid, crop, items): vote(items, grid, crop, align, ...) is the kind's ops function."""
    from dcfp_amd import ops
    if request.param == "whole":
        import _vote_ref as vr
        N, C, grid, crop = 2, 19, (17, 25), (15, 22)
        passes = vr.make_passes(5, N, C, grid, (0.75, 1.0), True)
        return ops.multiscale_vote, N, C, grid, crop, vr.to_maps(passes, cuda)
    import _slide_ref as sr
    N, C, grid, crop, tile = 2, 19, (33, 41), (30, 37), (17, 17)
    passes = sr.make_passes(5, N, C, grid, tile, (0.75, 1.0), True)
    return ops.sliding_vote, N, C, grid, crop, sr.to_passes(passes, grid, tile, cuda)


def test_all_ignore_leaves_conf_unchanged(small, cuda):
    vote, N, C, grid, crop, items = small
    conf = torch.arange(C * C, dtype=torch.int64, device=cuda).view(C, C).contiguous()
    before = conf.clone()
    gt = torch.full((N,) + crop, 255, dtype=torch.int64, device=cuda)
    vote(items, grid, crop, True, labels=gt, conf=conf)
    assert torch.equal(conf, before)


def test_labels_outside_the_classes_are_skipped(small, cuda):
    from dcfp_amd import ops
    vote, N, C, grid, crop, items = small
    gt = labels_for(3, N, C, crop)
    g = torch.Generator().manual_seed(4)
    r = torch.rand(gt.shape, generator=g)
    gt[r < 0.1] = C            # no class, not ignore
    gt[(r >= 0.1) & (r < 0.2)] = 254
    gt[(r >= 0.2) & (r < 0.3)] = -1
    gt = gt.to(cuda)
    conf = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    pred, _ = vote(items, grid, crop, True, labels=gt, conf=conf)
    assert int(conf.sum()) == int(((gt >= 0) & (gt < C)).sum())
    assert torch.equal(conf, ops.confusion_matrix(pred, gt, C))
    # another ignore index: 255 then counts as out of range, the chosen one is skipped
    conf3 = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    vote(items, grid, crop, True, labels=gt, conf=conf3, ignore_index=3)
    assert int(conf3.sum()) == int(((gt >= 0) & (gt < C) & (gt != 3)).sum())


def test_two_calls_accumulate_and_repeat_bit_for_bit(small, cuda):
    vote, N, C, grid, crop, items = small
    gt = labels_for(9, N, C, crop).to(cuda)
    conf = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    pred1, scores1 = vote(items, grid, crop, True, labels=gt, conf=conf, want_scores=True)
    once = conf.clone()
    pred2, scores2 = vote(items, grid, crop, True, labels=gt, conf=conf, want_scores=True)
    assert torch.equal(conf, 2 * once)
    assert torch.equal(pred1, pred2) and torch.equal(scores1.view(torch.int32), scores2.view(torch.int32))
    fresh = torch.zeros((C, C), dtype=torch.int64, device=cuda)
    vote(items, grid, crop, True, labels=gt, conf=fresh, want_pred=False)
    assert torch.equal(fresh, once)


def test_argument_checks(small, cuda):
    from dcfp_amd import ops
    vote, N, C, grid, crop, items = small
    sliding = vote is ops.sliding_vote
    with pytest.raises(RuntimeError):
        vote([], grid, crop, True)
    with pytest.raises(RuntimeError):                                         # 17 passes / 20 maps
        vote((items * 5)[:17] if sliding else items * 5, grid, crop, True)
    with pytest.raises(RuntimeError):
        vote(items, grid, (grid[0] + 1, grid[1]), True)
    with pytest.raises(RuntimeError):
        vote(items, grid, crop, True, conf=torch.zeros((C, C), dtype=torch.int64, device=cuda))
    with pytest.raises(RuntimeError):
        vote([(items[0][0].cpu(),) + items[0][1:]], grid, crop, True)
    with pytest.raises(RuntimeError):
        vote(items, grid, crop, True, want_pred=False)
    if not sliding:
        return
    logits, hw, tile, ys, xs, flip, weight = items[0]
    with pytest.raises(RuntimeError):                                         # 33 tile rows
        many = torch.zeros((33 * len(xs),) + tuple(logits.shape[1:]), device=cuda)
        vote([(many, hw, tile, list(range(33)), xs, flip, weight)], grid, crop, True)
    with pytest.raises(RuntimeError):                                         # a row of pixels under no tile
        gap = [0] + [tile[0] + 1] * (len(ys) - 1)                              # row tile[0] is skipped
        assert len(ys) == 2 and gap[1] < hw[0]
        vote([(logits, hw, tile, gap, xs, flip, weight)], grid, crop, True)
