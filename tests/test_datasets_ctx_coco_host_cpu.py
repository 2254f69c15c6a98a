"""CPU: the Pascal-Context (`CTX`) and COCO-Stuff (`COCO`) dataset classes - list parsing, paths, the raw id -> class
table, decoding, the resample index and the palette - on tiny trees written into tmp_path."""
import os
import sys

import numpy as np
import pytest

from dcfp_amd.datasets import BaseDataSet, COCOdatasets, CTXdatasets, build_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"CTX": (59, "labels", ".png", CTXdatasets), "COCO": (171, "annotations", "_labelTrainIds.png", COCOdatasets)}
SIZES = [(24, 36), (30, 20), (24, 36)]


def write_tree(root, key, sizes=SIZES, every_class=True):
    """JPEG images, PNG labels of raw ids (0 = unlabelled, k = class k - 1), two image sizes, a list with blank lines"""
    from PIL import Image
    C, label_dir, suffix, _ = KINDS[key]
    rs = np.random.RandomState(len(key))
    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, label_dir))
    names, labels = [], []
    for i, (h, w) in enumerate(sizes):
        name = "s%d_%s" % (i, key.lower())
        lab = rs.randint(0, C + 1, (h, w)).astype(np.uint8)
        if every_class:                                              # raw ids 1 .. C, spread over the files in turn
            ids = np.arange(1 + i, C + 1, len(sizes), dtype=np.uint8)
            lab.reshape(-1)[:len(ids)] = ids
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, "images", name + ".jpg"))
        Image.fromarray(lab).save(os.path.join(root, label_dir, name + suffix))
        names.append(name)
        labels.append(lab)
    lst = os.path.join(root, "train.lst")
    with open(lst, "w") as f:
        f.write("\n".join([names[0], "", names[1], "   ", names[2]]) + "\n\n")
    return {"root": str(root), "list_path": lst}, names, labels


@pytest.mark.parametrize("key", sorted(KINDS))
def test_list_paths_and_names(tmp_path, key):
    C, label_dir, suffix, module = KINDS[key]
    para, names, _ = write_tree(str(tmp_path), key)
    ds = build_dataset(key, split="train", data_dir="train", data_para=para)
    assert isinstance(ds, module.DataSet) and isinstance(ds, BaseDataSet)
    assert ds.num_classes == C and ds.class_weights is None and ds.ignore_label == 255
    assert len(ds) == 3 and [f["name"] for f in ds.files] == names
    for f, name in zip(ds.files, names):
        assert f["img"] == os.path.join(para["root"], "images", name + ".jpg")
        assert f["label"] == os.path.join(para["root"], label_dir, name + suffix)
        assert os.path.isfile(f["img"]) and os.path.isfile(f["label"])
    assert len(build_dataset(key, split="val", data_para=para)) == 3
    rep = build_dataset(key, split="train", data_para=dict(para, max_iters=7))          # ceil(7 / 3) passes of the list
    assert len(rep) == 9 and [f["name"] for f in rep.files] == names * 3


@pytest.mark.parametrize("key", sorted(KINDS))
def test_errors(tmp_path, key):
    para, _, _ = write_tree(str(tmp_path), key)
    with pytest.raises(NotImplementedError):
        build_dataset(key, split="test", data_para=para)
    with pytest.raises(ValueError):
        build_dataset(key, split="train", ignore_label=254, data_para=para)
    with pytest.raises(ValueError):
        build_dataset(key, split="train", data_para={"root": para["root"]})
    with pytest.raises(NotImplementedError):
        build_dataset("VOC", split="train", data_para=para)


@pytest.mark.parametrize("key", sorted(KINDS))
def test_id_table_and_round_trip(tmp_path, key):
    para, _, _ = write_tree(str(tmp_path), key)
    ds = build_dataset(key, split="train", data_para=para)
    assert np.array_equal(ds.id_table(), (np.arange(256) - 1).astype(np.uint8))
    raw = np.arange(256, dtype=np.uint8).reshape(16, 16)
    train = ds.id2trainId(raw)
    assert np.array_equal(train, ds.id_table()[raw]) and train[0, 0] == 255 and train[0, 1] == 0
    assert np.array_equal(ds.id2trainId(train, reverse=True), raw)


@pytest.mark.parametrize("key", sorted(KINDS))
def test_decode(tmp_path, key):
    from PIL import Image
    para, names, labels = write_tree(str(tmp_path), key)
    ds = build_dataset(key, split="val", data_para=para)
    for i, (h, w) in enumerate(SIZES):
        image, label = ds.decode(i)
        assert image.dtype == np.uint8 and image.shape == (h, w, 3) and image.flags["C_CONTIGUOUS"]
        assert label.dtype == np.uint8 and np.array_equal(label, labels[i])
        with Image.open(ds.files[i]["img"]) as im:                       # BGR: PIL's RGB planes reversed
            assert np.array_equal(image[:, :, ::-1], np.asarray(im.convert("RGB")))
    Image.fromarray(np.zeros((5, 7), dtype=np.uint8)).save(ds.files[1]["label"])
    with pytest.raises(ValueError, match="label size"):
        ds.decode(1)


@pytest.mark.parametrize("key", sorted(KINDS))
def test_resample_index(tmp_path, key):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import label_index
    finally:
        sys.path.pop(0)
    C = KINDS[key][0]
    para, names, labels = write_tree(str(tmp_path), key)
    with pytest.raises(NotImplementedError, match="label_index_%s.pkl" % key):
        build_dataset(key, split="train", data_para=dict(para, resample=True))
    plain = build_dataset(key, split="train", data_para=para)
    index = label_index.build_index(plain)
    for c in range(C):                                                  # class c is raw id c + 1
        assert [e["idx"] for e in index[str(c)]] == [i for i, l in enumerate(labels) if (l == c + 1).any()]
    path = label_index.main(["--dataset", key, "--data-para", __import__("json").dumps(para)])
    assert path == os.path.join(str(tmp_path), "label_index_%s.pkl" % key)
    ds = build_dataset(key, split="train", data_para=dict(para, resample=True))
    longest = int(index["label_f"].max())
    assert len(ds) == longest * C and len(ds.file_index) == len(ds.class_index) == longest * C
    for i in (0, longest, len(ds) - 1):
        f_idx, cls = ds.locate(i)
        assert cls == i // longest and (labels[f_idx] == cls + 1).any()
    first = list(ds.file_index)
    ds.gen_index(1)
    assert len(ds.file_index) == len(first)


@pytest.mark.parametrize("key", sorted(KINDS))
def test_palette(tmp_path, key):
    C = KINDS[key][0]
    para, _, _ = write_tree(str(tmp_path), key)
    cmap = np.asarray(build_dataset(key, split="val", data_para=para).cmap_labels)
    assert cmap.shape == (C, 3) and cmap.min() >= 0 and cmap.max() <= 255
    assert np.array_equal(cmap, cmap.astype(np.uint8))
    assert len({tuple(r) for r in cmap.tolist()}) == C
    assert not (cmap == 0).all(axis=1).any()
    # the bit-reversal rule, restated: entry i + 1; bits 0 / 1 / 2 of each 3-bit group go to R / G / B from the top down
    assert cmap[0].tolist() == [128, 0, 0] and cmap[1].tolist() == [0, 128, 0] and cmap[7].tolist() == [64, 0, 0]
