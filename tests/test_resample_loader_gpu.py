"""GPU: TrainLoader over a `resample` dataset against tests/_augment_ref.py driven by the crop offsets of
the restatement in tests/_resample_ref.py, and two steps of the fine-tune command line of tools/train.py."""
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
from dcfp_amd.datasets import AugParams, TrainLoader, build_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_RAW = sorted(ref.CS_TRAIN_IDS)


def write_cs(tmp_path, sizes):
    """PNG pairs with blocky label maps (5x5 blocks of raw ids, some of them ignored ids), a strip of every class in
    file 0, the list file and the class index the dataset looks for next to it."""
    from PIL import Image
    rs = np.random.RandomState(9)
    table = ref.cs_id_table()
    lines, index = [], {str(c): [] for c in range(19)}
    for i, (h, w) in enumerate(sizes):
        coarse = rs.choice(np.array(TRAIN_RAW[:6] + [0, 3], dtype=np.uint8), size=(-(-h // 5), -(-w // 5)))
        ids = np.ascontiguousarray(np.kron(coarse, np.ones((5, 5), dtype=np.uint8))[:h, :w])
        if i == 0:
            ids[:2, :38] = np.repeat(np.array(TRAIN_RAW, dtype=np.uint8), 2)[None, :]
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(tmp_path / ("im%d.png" % i))
        Image.fromarray(ids).save(tmp_path / ("gt%d.png" % i))
        lines.append("im%d.png gt%d.png" % (i, i))
        for c in np.unique(table[ids]):
            if c < 19:
                index[str(int(c))].append({"idx": i, "name": "gt%d" % i})
    index["label_f"] = np.array([len(index[str(c)]) for c in range(19)], dtype=np.float64)
    (tmp_path / "train.lst").write_text("\n".join(lines) + "\n")
    with open(tmp_path / "label_index_CS.pkl", "wb") as f:
        pickle.dump(index, f)
    return {"root": str(tmp_path), "list_path": str(tmp_path / "train.lst")}, index


def test_resample_loader_end_to_end(cuda, tmp_path):
    from PIL import Image
    para, index = write_cs(tmp_path, [(40, 60), (50, 70), (33, 47), (64, 64), (36, 90), (48, 48)])
    crop, seed, bs = (16, 16), 13, 3
    ds = build_dataset("CS", split="train", crop_size=crop, scale=True, mirror=True, brightness=False, balance=2,
                       data_para=dict(para, resample=True))
    loader = TrainLoader(ds, bs, cuda, seed=seed, num_workers=2, rank=0, world_size=1)
    longest = int(index["label_f"].max())
    assert 3 <= longest <= 6 and len(ds) == longest * 19 and len(loader) == longest * 19 // bs
    table = ref.cs_id_table()
    rng = random.Random(seed)
    it = iter(loader)
    order = loader.indices(0)
    lengths = [len(index[str(c)]) for c in range(19)]
    file_index, class_index = R.gen_index(lengths, seed, 0)
    placed = 0
    for b in range(3):
        images, labels = next(it)
        assert set(labels) == {"ori", "weight"} and images.shape == (bs, 3) + crop
        children = [random.Random(rng.getrandbits(64)) for _ in range(bs)]
        for j, i in enumerate(order[bs * b:bs * b + bs]):
            cls = class_index[i]
            f_idx = index[str(cls)][file_index[i]]["idx"]
            assert ds.locate(i) == (f_idx, cls)
            img = np.ascontiguousarray(np.asarray(Image.open(tmp_path / ("im%d.png" % f_idx)).convert("RGB"))[:, :, ::-1])
            raw = np.asarray(Image.open(tmp_path / ("gt%d.png" % f_idx)))
            H, W = raw.shape
            child = children[j]
            f = 0.5 + child.randint(0, 15) / 10.0
            dst_h, dst_w = max(1, int(round(H * f))), max(1, int(round(W * f)))
            grid = (max(dst_h, crop[0]), max(dst_w, crop[1]))
            mask = R.class_mask(raw, table, R.nearest_map(H, dst_h, f), R.nearest_map(W, dst_w, f), grid, cls)
            lab, roots, _ = R.label_components(mask)
            h_off, w_off, flip, pixel = R.crop_draws(child, grid, crop, True, lab, roots)
            assert loader.last_pixels[j] == pixel, (b, j)
            if pixel is not None:                       # the class is present: the crop (before mirroring) holds the pixel
                assert h_off <= pixel[0] < h_off + crop[0] and w_off <= pixel[1] < w_off + crop[1]
                placed += 1
            p = AugParams(f_scale=f, dst_h=dst_h, dst_w=dst_w, h_off=h_off, w_off=w_off, flip=flip)
            want, want_l, _ = ref.augment(img, raw, p, crop, table)
            assert np.array_equal(images[j].cpu().numpy().view(np.uint32), want.view(np.uint32)), (b, j, p)
            assert np.array_equal(labels["ori"][j].cpu().numpy(), want_l), (b, j, p)
            want_w = ref.balance_weight(want_l, 19, 2, 255, cls)
            w = labels["weight"][j].cpu().numpy()
            assert np.all(w[want_l == 255] == 0.0)
            assert np.allclose(w, want_w, rtol=1e-6, atol=0.0), (b, j)      # fp64 on both sides, one fp32 rounding
    assert placed >= 6


def test_finetune_command_line(cuda, tmp_path):
    """Two steps of the reference's fine-tune recipe on a list file with its index: --balance 2, resample, GSRL."""
    para, _ = write_cs(tmp_path, [(80, 100), (70, 90), (90, 120), (66, 130), (75, 75), (88, 96)])
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--model", "simple", "--ddp", "False",
           "--dataset", "CS", "--balance", "2", "--data-para", json.dumps(dict(para, resample=True)),
           "--loss-type", "gsrl", "--random-scale", "--random-mirror", "--random-brightness", "--input-size", "65,65",
           "--batch-size", "2", "--num-steps", "2", "--snapshot-dir", str(tmp_path / "snap"), "--backbone-para",
           json.dumps({"pretrained": False}), "--learning-rate", "1e-3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    losses = [float(l.split("loss=")[1]) for l in r.stdout.splitlines() if "loss=" in l]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-2000:]
