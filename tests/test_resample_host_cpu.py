"""CPU: the host half of the `resample` sampler - the epoch index, locate, the class-index tool and the
crop draws - against the restatement in tests/_resample_ref.py; and that restatement's labelling against scipy."""
import os
import pickle
import random

import numpy as np
import pytest

import _resample_ref as R
from dcfp_amd.datasets import AugConfig, AugParams, BaseDataSet, build_dataset, draw_crop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 3, 7]            # 7 % 1 == 0, 7 % 3 != 0, 7 % 7 == 0
CLASS_FILES = {"0": [4], "1": [0, 2, 5], "2": [6, 5, 4, 3, 2, 1, 0]}


class Tiny(BaseDataSet):
    """Three classes over seven files, the index loaded from a pickle as a dataset class does."""

    def __init__(self, index_path, **kwargs):
        super().__init__(split="train", crop_size=(8, 8), **kwargs)
        self.num_classes = 3
        self.files = [{"name": "f%d" % i} for i in range(7)]
        if self.resample:
            self.load_index(index_path)


def write_index(path, class_files=CLASS_FILES):
    index = {c: [{"idx": i, "name": "f%d" % i} for i in files] for c, files in class_files.items()}
    index["label_f"] = np.array([len(class_files[str(c)]) for c in range(3)], dtype=np.float64)
    with open(path, "wb") as f:
        pickle.dump(index, f)
    return str(path)


@pytest.mark.parametrize("seed", [0, 42])
def test_gen_index_len_and_locate(tmp_path, seed):
    ds = Tiny(write_index(tmp_path / "label_index_T.pkl"), resample=True, seed=seed)
    assert len(ds) == 21                                          # label_f.max() * num_classes
    for epoch in (0, 3):
        ds.pre_processing(epoch, 10)
        file_index, class_index = R.gen_index(LENGTHS, seed, epoch)
        assert ds.file_index == file_index and ds.class_index == class_index
        assert class_index == [0] * 7 + [1] * 7 + [2] * 7
        assert file_index[:7] == [0] * 7 and file_index[7:13] == [0, 1, 2, 0, 1, 2] and sorted(file_index[14:]) == list(range(7))
        for i in range(len(ds)):
            c = class_index[i]
            assert ds.locate(i) == (CLASS_FILES[str(c)][file_index[i]], c)


def test_same_index_on_every_rank_and_a_new_one_every_epoch(tmp_path):
    import torch
    from dcfp_amd.datasets import TrainLoader
    path = write_index(tmp_path / "label_index_T.pkl")
    per_rank = []
    for rank in (0, 1):
        ds = Tiny(path, resample=True, balance=2)
        loader = TrainLoader(ds, 2, torch.device("cpu"), seed=11, num_workers=1, rank=rank, world_size=2)
        assert ds.seed == 11 and len(loader) == 5                 # ceil(21 / 2) samples per rank, batches of 2
        epochs = []
        for epoch in range(6):
            ds.pre_processing(epoch, 6)
            epochs.append((list(ds.file_index), list(ds.class_index)))
        per_rank.append((epochs, loader.indices(0)))
    assert per_rank[0][0] == per_rank[1][0]
    # the two shards cover the epoch index; 22 slots for 21 entries: the permutation's first entry wraps around
    assert sorted(per_rank[0][1] + per_rank[1][1]) == sorted(list(range(21)) + [per_rank[0][1][0]])
    assert len({tuple(e[0]) for e in per_rank[0][0]}) > 1         # the remainder sample of class 1 moves with the epoch
    plain = Tiny(path)
    plain.pre_processing(3, 6)
    assert len(plain) == 7 and plain.locate(5) == (5, None)
    with pytest.raises(ValueError):
        TrainLoader(Tiny(path, balance=2), 2, torch.device("cpu"), rank=0, world_size=1)


def test_empty_class_is_refused(tmp_path):
    path = write_index(tmp_path / "label_index_T.pkl", {"0": [4], "1": [], "2": [0, 1]})
    with pytest.raises(ValueError, match="class 1"):
        Tiny(path, resample=True)


# ------------------------------------------------------------------ the class-index tool on Cityscapes files
TRAIN_RAW = [7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33]     # raw id of trainId 0 .. 18


def write_cs(tmp_path):
    from PIL import Image
    ids = [np.array(TRAIN_RAW + [0], dtype=np.uint8).reshape(4, 5),          # every class, and an ignored id
           np.array([[7, 7, 8], [8, 8, 7]], dtype=np.uint8),
           np.array([[7, 0, 0], [1, 2, 3]], dtype=np.uint8),                 # class 0 and ignored ids only
           np.full((3, 4), 33, dtype=np.uint8)]
    os.makedirs(tmp_path / "img")
    os.makedirs(tmp_path / "gt")
    lines = []
    for i, a in enumerate(ids):
        Image.fromarray(np.zeros(a.shape + (3,), dtype=np.uint8)).save(tmp_path / "img" / ("s%d.png" % i))
        Image.fromarray(a).save(tmp_path / "gt" / ("s%d_ids.png" % i))
        lines.append("img/s%d.png gt/s%d_ids.png" % (i, i))
    (tmp_path / "train.lst").write_text("\n".join(lines) + "\n")
    return {"root": str(tmp_path), "list_path": str(tmp_path / "train.lst")}


def test_missing_index_names_the_file_and_the_tool(tmp_path):
    para = write_cs(tmp_path)
    with pytest.raises(NotImplementedError) as e:
        build_dataset("CS", split="train", data_para=dict(para, resample=True))
    assert str(tmp_path / "label_index_CS.pkl") in str(e.value) and "tools/label_index.py" in str(e.value)
    with pytest.raises(NotImplementedError, match="label_index_CStest.pkl"):
        build_dataset("CS", split="test", data_para=dict(para, resample=True))


def test_label_index_tool(tmp_path):
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("label_index_tool", os.path.join(ROOT, "tools", "label_index.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    para = write_cs(tmp_path)
    path = tool.main(["--dataset", "CS", "--data-para", json.dumps(para), "--save-dir", str(tmp_path)])
    assert path == str(tmp_path / "label_index_CS.pkl")
    with open(path, "rb") as f:
        got = pickle.load(f)

    def entry(i):
        return {"idx": i, "name": "s%d_ids" % i}
    want = {str(c): [entry(0)] for c in range(19)}
    want["0"] = [entry(0), entry(1), entry(2)]
    want["1"] = [entry(0), entry(1)]
    want["18"] = [entry(0), entry(3)]
    label_f = got.pop("label_f")
    assert got == want and type(got) is dict and type(got["0"]) is list
    assert label_f.dtype == np.float64 and label_f.tolist() == [3.0, 2.0] + [1.0] * 16 + [2.0]
    ds = build_dataset("CS", split="train", crop_size=(2, 2), balance=2, data_para=dict(para, resample=True, seed=5))
    assert len(ds) == 3 * 19
    file_index, class_index = R.gen_index([3, 2] + [1] * 16 + [2], 5, 0)
    assert ds.file_index == file_index and ds.class_index == class_index
    assert ds.locate(0) == (0, 0) and ds.locate(2) == (2, 0) and ds.locate(3 * 18 + 1) == (3, 18)


# ------------------------------------------------------------------ the crop draws
def blobs(grid, boxes):
    m = np.zeros(grid, dtype=bool)
    for y, x, h, w in boxes:
        m[y:y + h, x:x + w] = True
    return m


CROP_CASES = {
    "nums1": blobs((40, 60), []),                                                       # no component: plain draws
    "nums2": blobs((40, 60), [(15, 20, 6, 9)]),
    "nums5": blobs((40, 60), [(2, 2, 3, 3), (2, 50, 4, 2), (20, 25, 5, 5), (35, 3, 4, 8)]),
    "clip_low": blobs((40, 60), [(0, 0, 2, 2)]),                                        # offsets below 0
    "clip_high": blobs((40, 60), [(38, 58, 2, 2)]),                                     # offsets above size - crop
}


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("case", sorted(CROP_CASES))
def test_draw_crop_replays_the_reference_order(case, mirror):
    mask = CROP_CASES[case]
    lab, roots, sizes = R.label_components(mask)
    assert len(roots) + 1 == {"nums1": 1, "nums2": 2, "nums5": 5, "clip_low": 2, "clip_high": 2}[case]
    cfg = AugConfig(16, 24, mirror=mirror)
    flips, clipped = set(), set()
    for seed in range(12):
        p = AugParams(dst_h=40, dst_w=60)
        asked = []

        def answer(q):
            asked.append(q[0])
            if q[0] == "count":
                return len(roots)
            if q[0] == "size":
                return int(sizes[q[1] - 1])
            return R.kth_pixel(lab, roots[q[1] - 1], q[2])
        pixel = draw_crop(random.Random(seed), p, cfg, answer)
        # the replay, written out: the same generator, the reference's draws in the reference's order
        rng = random.Random(seed)
        if len(roots) >= 1:
            n = rng.randint(1, len(roots))
            where = np.flatnonzero(lab.reshape(-1) == roots[n - 1])
            at = int(where[rng.randint(0, len(where) - 1)])
            want_pixel = (at // 60, at % 60)
            h_off = want_pixel[0] - 8 - rng.randint(-4, 4)
            w_off = want_pixel[1] - 12 - rng.randint(-6, 6)
            assert asked == ["count", "size", "pixel"]
        else:
            want_pixel = None
            h_off, w_off = rng.randint(0, 24), rng.randint(0, 36)
            assert asked == ["count"]
        clipped.add((h_off < 0 or w_off < 0, h_off > 24 or w_off > 36))
        h_off, w_off = int(np.clip(h_off, 0, 24)), int(np.clip(w_off, 0, 36))
        flip = mirror and rng.randint(0, 1) * 2 - 1 < 0
        assert (pixel, p.h_off, p.w_off, p.flip) == (want_pixel, h_off, w_off, flip)
        assert (p.h_off, p.w_off, p.flip, pixel) == R.crop_draws(random.Random(seed), (40, 60), (16, 24), mirror, lab, roots)
        flips.add(p.flip)
        if pixel is not None and not (h_off in (0, 24) or w_off in (0, 36)):
            assert p.h_off <= pixel[0] < p.h_off + 16 and p.w_off <= pixel[1] < p.w_off + 24
    assert flips == ({False, True} if mirror else {False})
    if case == "clip_low":
        assert (True, False) in clipped
    if case == "clip_high":
        assert (False, True) in clipped


def test_restatement_labels_like_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, mask in R.pattern_masks(64).items():
        comp, n = ndimage.label(mask, np.ones((3, 3)))
        lab, roots, sizes = R.label_components(mask)
        assert n == len(roots), name
        assert np.array_equal(R.renumber_by_first_pixel(comp), lab), name
        assert sizes.sum() == mask.sum(), name
