"""CPU: the host side of dataset evaluation - EvalLoader's sharding and batch cuts, the pad_inf / generate_size sizes,
the descriptor checks of dcfp_vote_multiscale_f32 (no launch without a GPU) and the palette PNG."""
import ctypes

import numpy as np
import pytest


class _Files:
    """What EvalLoader needs of a dataset to plan its batches."""
    split, balance, resample = "val", 0, False

    def __init__(self, n):
        self.files = [{"name": "f%d" % i} for i in range(n)]

    def __len__(self):
        return len(self.files)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_every_file_exactly_once_across_the_ranks(world):
    from dcfp_amd.datasets import EvalLoader
    per_rank = [EvalLoader(_Files(5), 2, "cpu", rank=r, world_size=world).indices() for r in range(world)]
    assert sorted(i for idx in per_rank for i in idx) == [0, 1, 2, 3, 4]        # no wrap-around padding
    for r, idx in enumerate(per_rank):
        assert idx == list(range(r, 5, world))


def test_short_last_batch_and_cut_at_a_size_change():
    from dcfp_amd.datasets import EvalLoader
    one = [(60, 90)] * 5
    ld = EvalLoader(_Files(5), 2, "cpu", rank=0, world_size=1)
    assert ld.batches(one) == [[0, 1], [2, 3], [4]] and len(ld) == 3
    assert EvalLoader(_Files(5), 2, "cpu", rank=1, world_size=2).batches(one) == [[1, 3]]
    assert EvalLoader(_Files(5), 2, "cpu", rank=0, world_size=2).batches(one) == [[0, 2], [4]]
    mixed = [(60, 90), (60, 90), (60, 90), (30, 40), (30, 40)]
    assert EvalLoader(_Files(5), 4, "cpu", rank=0, world_size=1).batches(mixed) == [[0, 1, 2], [3, 4]]
    assert EvalLoader(_Files(5), 2, "cpu", rank=0, world_size=1).batches(mixed) == [[0, 1], [2], [3, 4]]
    swapped = [(60, 90), (90, 60), (60, 90)]
    assert EvalLoader(_Files(3), 4, "cpu", rank=0, world_size=1).batches(swapped) == [[0], [1], [2]]


def test_eval_loader_takes_val_and_test_only():
    from dcfp_amd.datasets import EvalLoader
    ds = _Files(3)
    ds.split = "train"
    with pytest.raises(ValueError):
        EvalLoader(ds, 2, "cpu", rank=0, world_size=1)


def test_pad_inf_and_generate_size():
    from dcfp_amd import evaluate as ev
    assert ev.pad_inf_size(60, 90) == (65, 97)
    assert ev.pad_inf_size(1024, 2048) == (1025, 2049)
    assert ev.pad_inf_size(65, 97) == (65, 97)                    # 8k+1 already
    assert ev.pad_inf_size(64, 66) == (65, 73)
    assert ev.generate_size(60, 90, 120, "long") == (80, 120)
    assert ev.generate_size(60, 90, 120, "short") == (120, 180)
    assert ev.generate_size(1024, 2048, 1000, "long") == (500, 1000)
    assert ev.generate_size(375, 500, 512, "short") == (512, 683)  # int(500 * 512/375 + 0.5) = int(683.17)
    with pytest.raises(NotImplementedError):
        ev.generate_size(60, 90, 120, "area")


def _vote(L, maps, n_maps, N=1, C=19, H=9, W=9, oh=9, ow=9, scores=1, pred=1, gt=0, conf=0):
    p = lambda v: ctypes.c_void_p(0x1000 if v else None)          # never dereferenced: the checks come before the launch
    return L.dcfp_vote_multiscale_f32(maps, n_maps, N, C, H, W, oh, ow, 1, p(scores), p(pred), p(gt), 255, p(conf), None)


def test_vote_descriptor_errors_do_not_need_a_gpu():
    from dcfp_amd import _lib
    L = _lib.lib()
    good = (_lib.VoteMap * 17)(*[_lib.VoteMap(0x1000, 2, 2, 9, 9, 0, 1.0) for _ in range(17)])
    assert _vote(L, good, 0) == _lib.E_BADDESC
    assert _vote(L, good, 17) == _lib.E_BADDESC
    assert _vote(L, None, 1) == _lib.E_BADDESC
    null = (_lib.VoteMap * 2)(_lib.VoteMap(0x1000, 2, 2, 9, 9, 0, 1.0), _lib.VoteMap(None, 2, 2, 9, 9, 0, 1.0))
    assert _vote(L, null, 2) == _lib.E_BADDESC                     # a null map
    assert _vote(L, good, 1, oh=10) == _lib.E_BADDESC              # out_h > H
    assert _vote(L, good, 1, ow=10) == _lib.E_BADDESC
    assert _vote(L, good, 1, C=0) == _lib.E_BADDESC
    assert _vote(L, good, 1, C=-3) == _lib.E_BADDESC
    assert _vote(L, good, 1, gt=0, conf=1) == _lib.E_BADDESC       # conf without gt
    assert _vote(L, good, 1, scores=0, pred=0) == _lib.E_BADDESC   # nothing asked for
    bad = (_lib.VoteMap * 1)(_lib.VoteMap(0x1000, 0, 2, 9, 9, 0, 1.0))
    assert _vote(L, bad, 1) == _lib.E_BADDESC                      # an empty map
    bad = (_lib.VoteMap * 1)(_lib.VoteMap(0x1000, 2, 2, 9, 9, 2, 1.0))
    assert _vote(L, bad, 1) == _lib.E_BADDESC                      # flip is 0 or 1
    assert ctypes.sizeof(_lib.VoteMap) == 32


def test_palette_png_round_trip(tmp_path):
    from PIL import Image
    from dcfp_amd import evaluate as ev
    from dcfp_amd.datasets import cs
    lst = tmp_path / "val.lst"
    lst.write_text("")
    palette = [int(v) for v in cs.DataSet(str(tmp_path), str(lst), split="val").cmap_labels.reshape(-1)]
    assert len(palette) == 19 * 3
    pred = (np.arange(60 * 90).reshape(60, 90) % 19).astype(np.int32)
    path = str(tmp_path / "p.png")
    ev.save_palette_png(pred, palette, path)
    with Image.open(path) as im:
        assert im.mode == "P" and im.size == (90, 60)
        assert np.array_equal(np.asarray(im), pred.astype(np.uint8))
        assert im.getpalette()[:19 * 3] == palette
