"""GPU: the Pascal-Context (`CTX`, 59 classes, --longsize) and COCO-Stuff (`COCO`, 171 classes, --shortsize) datasets
through TrainLoader (against tests/_augment_ref.py, the contract of the Cityscapes tests), EvalLoader, two steps of
the fine-tune command line of tools/train.py and one run of tools/evaluate.py.  Fixtures: JPEG images and PNG labels of
at most 64 px with every class in some file."""
import json
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import _augment_ref as ref
import _resample_ref as R
from dcfp_amd.datasets import AugParams, EvalLoader, TrainLoader, base, build_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"CTX": (59, "labels", ".png"), "COCO": (171, "annotations", "_labelTrainIds.png")}
TABLE = (np.arange(256) - 1).astype(np.uint8)                 # raw 0 -> 255 (ignored), raw k -> class k - 1
SIZES = [(40, 60), (50, 44), (33, 47), (64, 64), (36, 60), (48, 48)]


def write_tree(root, key, sizes=SIZES, split="train", index=True):
    """Blocky label maps (4 x 4 blocks, raw ids 0 .. C in turn across the files: every class is in some file), JPEG
    images, the list file and, next to it, the class index of tools/label_index.py."""
    from PIL import Image
    C, label_dir, suffix = KINDS[key]
    rs = np.random.RandomState(C)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, label_dir), exist_ok=True)
    names, first = [], 0
    for i, (h, w) in enumerate(sizes):
        bh, bw = -(-h // 4), -(-w // 4)
        coarse = ((first + np.arange(bh * bw)) % (C + 1)).astype(np.uint8).reshape(bh, bw)
        first += bh * bw
        raw = np.ascontiguousarray(np.kron(coarse, np.ones((4, 4), dtype=np.uint8))[:h, :w])
        name = "%s_%s%d" % (key.lower(), split, i)
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, "images", name + ".jpg"))
        Image.fromarray(raw).save(os.path.join(root, label_dir, name + suffix))
        names.append(name)
    lst = os.path.join(root, split + ".lst")
    with open(lst, "w") as f:
        f.write("\n".join(names) + "\n")
    para = {"root": str(root), "list_path": lst}
    if index:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        try:
            import label_index
        finally:
            sys.path.pop(0)
        idx = label_index.build_index(build_dataset(key, split="train", data_para=para))
        assert all(len(idx[str(c)]) >= 1 for c in range(C))
        with open(os.path.join(root, "label_index_%s.pkl" % key), "wb") as f:
            pickle.dump(idx, f)
    return para, names


def decoded(para, key, name):
    """(BGR uint8, raw uint8) of one sample, through PIL like the dataset"""
    from PIL import Image
    _, label_dir, suffix = KINDS[key]
    with Image.open(os.path.join(para["root"], "images", name + ".jpg")) as im:
        img = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[:, :, ::-1])
    with Image.open(os.path.join(para["root"], label_dir, name + suffix)) as im:
        raw = np.asarray(im.convert("L"), dtype=np.uint8)
    return img, raw


@pytest.mark.parametrize("key,size_arg", [("CTX", {"longsize": 48}), ("COCO", {"shortsize": 40})])
def test_train_loader(cuda, tmp_path, key, size_arg):
    """Mixed source sizes, --longsize / --shortsize scaling, mirror, brightness, balance 1: bit for bit the numpy
    restatement on the same decoded arrays and the same draws."""
    C = KINDS[key][0]
    para, names = write_tree(str(tmp_path), key, index=False)
    crop, seed, bs = (32, 36), 21, 3
    ds = build_dataset(key, split="train", crop_size=crop, scale=True, mirror=True, brightness=True, balance=1,
                       data_para=para, **size_arg)
    loader = TrainLoader(ds, bs, cuda, seed=seed, num_workers=2, rank=0, world_size=1)
    order, rng = loader.indices(0), random.Random(seed)
    assert sorted(order) == list(range(len(SIZES))) and len(loader) == 2
    cfg = base.AugConfig(crop[0], crop[1], scale=True, mirror=True, brightness=True,
                         long_size=size_arg.get("longsize", -1), short_size=size_arg.get("shortsize", -1))
    batches = list(loader)
    assert len(batches) == 2
    scales = set()
    for b, (images, labels) in enumerate(batches):
        assert set(labels) == {"ori", "weight"} and images.shape == (bs, 3) + crop and images.is_cuda
        for j, idx in enumerate(order[bs * b:bs * b + bs]):
            img, raw = decoded(para, key, names[idx])
            p = base.draw_params(rng, img.shape[:2], cfg)
            edge = max(img.shape[:2]) if "longsize" in size_arg else min(img.shape[:2])
            assert abs(p.f_scale * edge - round(p.f_scale * edge)) < 1e-9       # the scaled edge is a whole pixel count
            scales.add(round(p.f_scale * edge))
            want, want_l, _ = ref.augment(img, raw, p, crop, TABLE)
            assert np.array_equal(images[j].cpu().numpy().view(np.uint32), want.view(np.uint32)), (b, j, p)
            got_l = labels["ori"][j].cpu().numpy()
            assert np.array_equal(got_l, want_l), (b, j, p)
            assert set(np.unique(got_l).tolist()) <= set(range(C)) | {255}
            w = labels["weight"][j].cpu().numpy()
            assert np.all(w[want_l == 255] == 0.0)
            assert np.allclose(w, ref.balance_weight(want_l, C, 1), rtol=1e-6, atol=0.0), (b, j)
    assert len(scales) >= 2


@pytest.mark.parametrize("key,size_arg", [("COCO", {"shortsize": 40}), ("CTX", {"longsize": 48})])
def test_resample_loader(cuda, tmp_path, key, size_arg):
    """balance 2 + resample: the crop holds a pixel of the sample's class, image and label equal the restatement, the
    weights equal ref.balance_weight with the class as target (fp64 on both sides, one fp32 rounding)."""
    C = KINDS[key][0]
    para, names = write_tree(str(tmp_path), key)
    with open(os.path.join(str(tmp_path), "label_index_%s.pkl" % key), "rb") as f:
        index = pickle.load(f)
    crop, seed, bs = (16, 16), 13, 3
    ds = build_dataset(key, split="train", crop_size=crop, scale=True, mirror=True, brightness=False, balance=2,
                       data_para=dict(para, resample=True), **size_arg)
    loader = TrainLoader(ds, bs, cuda, seed=seed, num_workers=2, rank=0, world_size=1)
    longest = int(index["label_f"].max())
    assert len(ds) == longest * C and len(loader) == longest * C // bs
    cfg = ds.aug_config
    rng = random.Random(seed)
    it = iter(loader)
    order = loader.indices(0)
    file_index, class_index = R.gen_index([len(index[str(c)]) for c in range(C)], seed, 0)
    placed = 0
    for b in range(3):
        images, labels = next(it)
        assert set(labels) == {"ori", "weight"} and images.shape == (bs, 3) + crop
        children = [random.Random(rng.getrandbits(64)) for _ in range(bs)]
        for j, i in enumerate(order[bs * b:bs * b + bs]):
            cls = class_index[i]
            f_idx = index[str(cls)][file_index[i]]["idx"]
            assert ds.locate(i) == (f_idx, cls)
            img, raw = decoded(para, key, names[f_idx])
            H, W = raw.shape
            child = children[j]
            pre = base.draw_pre(child, (H, W), cfg)                      # the scale draw under --longsize / --shortsize
            f, dst_h, dst_w = pre.f_scale, pre.dst_h, pre.dst_w
            grid = (max(dst_h, crop[0]), max(dst_w, crop[1]))
            mask = R.class_mask(raw, TABLE, R.nearest_map(H, dst_h, f), R.nearest_map(W, dst_w, f), grid, cls)
            lab, roots, _ = R.label_components(mask)
            h_off, w_off, flip, pixel = R.crop_draws(child, grid, crop, True, lab, roots)
            assert loader.last_pixels[j] == pixel, (b, j)
            if pixel is not None:
                assert h_off <= pixel[0] < h_off + crop[0] and w_off <= pixel[1] < w_off + crop[1]
                placed += 1
            p = AugParams(f_scale=f, dst_h=dst_h, dst_w=dst_w, h_off=h_off, w_off=w_off, flip=flip)
            want, want_l, _ = ref.augment(img, raw, p, crop, TABLE)
            assert np.array_equal(images[j].cpu().numpy().view(np.uint32), want.view(np.uint32)), (b, j, p)
            assert np.array_equal(labels["ori"][j].cpu().numpy(), want_l), (b, j, p)
            want_w = ref.balance_weight(want_l, C, 2, 255, cls)
            w = labels["weight"][j].cpu().numpy()
            assert np.all(w[want_l == 255] == 0.0)
            assert np.allclose(w, want_w, rtol=1e-6, atol=0.0), (b, j)
    assert placed >= 6


@pytest.mark.parametrize("key", ["CTX", "COCO"])
def test_eval_loader(cuda, tmp_path, key):
    """every file once, in file order; a batch ends where the source size changes"""
    sizes = [(40, 60), (40, 60), (40, 60), (33, 47), (33, 47), (40, 60)]
    para, names = write_tree(str(tmp_path), key, sizes=sizes, split="val", index=False)
    ds = build_dataset(key, split="val", data_para=para)
    loader = EvalLoader(ds, 2, cuda, num_workers=2, rank=0, world_size=1)
    assert loader.batches(sizes) == [[0, 1], [2], [3, 4], [5]]
    served = []
    lut = base.lut_b(None, ref.MEAN, ref.STD)
    for images, labels, metas in loader:
        assert images.shape[0] == labels.shape[0] == len(metas) <= 2
        assert len({m["size"] for m in metas}) == 1 and tuple(images.shape[2:]) == metas[0]["size"]
        for j, m in enumerate(metas):
            img, raw = decoded(para, key, m["name"])
            assert np.array_equal(images[j].cpu().numpy(), np.stack([lut[c][img[:, :, 2 - c]] for c in range(3)]))
            assert np.array_equal(labels[j].cpu().numpy(), TABLE[raw])
            served.append(m["name"])
    assert served == names


def test_train_tool_coco_finetune(cuda, tmp_path):
    """Two steps of the fine-tune recipe on COCO-Stuff: 171 classes through DeepLabv3's two heads, resample, balance 2,
    GSRL (the chunked weighted-CE backward twice per step)."""
    para, _ = write_tree(str(tmp_path), "COCO")
    snap = tmp_path / "snap"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--model", "deeplabv3", "--backbone", "resnet50",
           "--ddp", "False", "--dataset", "COCO", "--balance", "2", "--data-para", json.dumps(dict(para, resample=True)),
           "--loss-type", "gsrl", "--align-corner", "False", "--random-scale", "--random-mirror", "--random-brightness",
           "--shortsize", "56", "--input-size", "64,64", "--batch-size", "2", "--num-steps", "2", "--snapshot-dir",
           str(snap), "--backbone-para", json.dumps({"pretrained": False}), "--learning-rate", "1e-3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    losses = [float(l.split("loss=")[1]) for l in r.stdout.splitlines() if "loss=" in l]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-2000:]
    saved = [f for f in os.listdir(snap) if f.endswith("_2.pth")]
    assert len(saved) == 1
    state = torch.load(os.path.join(snap, saved[0]), map_location="cpu", weights_only=False)
    assert any(v.shape[0] == 171 for v in state.values() if hasattr(v, "shape") and v.dim() >= 1)


def test_evaluate_tool_ctx(cuda, tmp_path):
    """tools/evaluate.py --dataset CTX --whole True --align-corner False --longsize 48: every labelled pixel of the
    fixture is counted exactly once; --save-predict writes one PNG per file with the dataset's palette."""
    from PIL import Image
    sizes = [(40, 60), (50, 44), (40, 60), (33, 47)]
    para, names = write_tree(str(tmp_path), "CTX", sizes=sizes, split="val", index=False)
    labelled = sum(int((TABLE[decoded(para, "CTX", n)[1]] != 255).sum()) for n in names)
    assert 0 < labelled < sum(h * w for h, w in sizes)
    snap = str(tmp_path / "snap")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), "--model", "simple", "--backbone", "resnet50",
           "--dataset", "CTX", "--whole", "True", "--align-corner", "False", "--longsize", "48", "--batch-size", "1",
           "--num-workers", "2", "--save-predict", "True", "--data-para", json.dumps(para), "--snapshot-dir", snap]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    sums = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"tp"')]
    assert len(sums) == 1 and sums[0]["pos"] == labelled and sums[0]["res"] == labelled and sums[0]["tp"] <= labelled
    palette = [int(v) for v in build_dataset("CTX", split="val", data_para=para).cmap_labels.reshape(-1)]
    for name, (h, w) in zip(names, sizes):
        with Image.open(os.path.join(snap, "outputs", name + ".png")) as im:
            assert im.mode == "P" and im.size == (w, h)
            assert im.getpalette()[:59 * 3] == palette
            assert int(np.asarray(im).max()) < 59
    assert len(os.listdir(os.path.join(snap, "outputs"))) == len(names)
