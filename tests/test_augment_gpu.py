"""GPU: the augmentation kernels (dcfp_amd/csrc/augment.hip) against tests/_augment_ref.py.  The image
path is integers, lookup tables and one fp32 block written one IEEE operation per statement, so images, labels and
histograms must be EQUAL to the reference; only the fp64 -> fp32 balance weights carry a tolerance."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import _augment_ref as ref
from dcfp_amd.datasets import TrainLoader, base, build_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = base.AugParams


def device_augment(dev, sources, params, crop, id_table=None, offset_first=False):
    """sources: [(uint8 [H,W,3], uint8 [H,W] or None)] -> numpy (images, labels, hist) of ops.augment_batch."""
    from dcfp_amd import ops
    hws = [im.shape[:2] for im, _ in sources]
    cfg = base.AugConfig(crop[0], crop[1])
    taps, lut_a, lut_b, recs = base.pack_batch(params, hws, cfg, ref.MEAN, ref.STD)
    d_images = [torch.from_numpy(np.ascontiguousarray(im)).to(dev) for im, _ in sources]
    if offset_first:                                  # the first image starts 1 byte past a 16-byte boundary
        flat = torch.zeros(d_images[0].numel() + 32, dtype=torch.uint8, device=dev)
        start = (-flat.data_ptr()) % 16 + 1
        flat[start:start + d_images[0].numel()] = d_images[0].reshape(-1)
        d_images[0] = flat[start:start + d_images[0].numel()].view(d_images[0].shape)
        assert d_images[0].data_ptr() % 16 == 1
    with_labels = sources[0][1] is not None
    d_labels = [torch.from_numpy(np.ascontiguousarray(lab)).to(dev) for _, lab in sources] if with_labels else None
    out = ops.augment_batch(d_images, d_labels, recs, torch.from_numpy(taps).to(dev),
                            None if lut_a is None else torch.from_numpy(lut_a).to(dev),
                            torch.from_numpy(lut_b).to(dev),
                            None if id_table is None else torch.from_numpy(id_table).to(dev), crop)
    torch.cuda.synchronize()
    return out


def check_equal(out, sources, params, crop, id_table=None):
    images, labels, hist = out
    for i, ((im, lab), p) in enumerate(zip(sources, params)):
        want, want_l, want_h = ref.augment(im, lab, p, crop, id_table)
        got = images[i].cpu().numpy()
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), "sample %d: %d of %d image values differ, first at %s: %r != %r" % (
            i, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0], want[bad][0])
        if lab is not None:
            assert labels.dtype == torch.int64 and np.array_equal(labels[i].cpu().numpy(), want_l), i
            assert hist.dtype == torch.int32 and np.array_equal(hist[i].cpu().numpy(), want_h), i


def rand_source(rs, h, w, classes=34):
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(0, classes, (h, w)).astype(np.uint8)


def params_for(hw, f, crop, at_max, flip, **kw):
    dh, dw = int(round(hw[0] * f)), int(round(hw[1] * f))
    return P(f_scale=f, dst_h=dh, dst_w=dw, flip=flip, h_off=(max(dh, crop[0]) - crop[0]) if at_max else 0,
             w_off=(max(dw, crop[1]) - crop[1]) if at_max else 0, **kw)


def test_identity(cuda):
    """f = 1, no jitter, crop = source: the image is LUT B of the source, the label the id table's lookup."""
    rs = np.random.RandomState(0)
    src = rand_source(rs, 37, 53)
    p = P(dst_h=37, dst_w=53)
    out = device_augment(cuda, [src], [p], (37, 53), ref.cs_id_table())
    lut = base.lut_b(None, ref.MEAN, ref.STD)
    want = np.stack([lut[c][src[0][:, :, 2 - c]] for c in range(3)])
    assert np.array_equal(out[0][0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out[1][0].cpu().numpy(), ref.cs_id_table()[src[1]].astype(np.int64))
    check_equal(out, [src], [p], (37, 53), ref.cs_id_table())


@pytest.mark.parametrize("crop", [(33, 41), (32, 40)])    # scalar stores (41 % 4 != 0) and 16-byte stores
def test_geometry(cuda, crop):
    """Sources of different sizes in one launch; f = 0.5 pads the bottom and right (18x26 < crop); a source one
    pixel wide; offsets at 0 and at the maximum; mirror mixed; the first image 1 byte off a 16-byte boundary."""
    rs = np.random.RandomState(1)
    sizes = [(37, 53), (64, 40), (19, 90), (23, 1)]
    sources = [rand_source(rs, h, w) for h, w in sizes]
    params = [params_for(sizes[0], 0.5, crop, False, True), params_for(sizes[1], 1.3, crop, True, False),
              params_for(sizes[2], 2.0, crop, True, True), params_for(sizes[3], 2.0, crop, False, False)]
    assert params[0].dst_h < crop[0] and params[0].dst_w < crop[1] and params[1].h_off > 0 and params[2].w_off > 0
    out = device_augment(cuda, sources, params, crop, ref.cs_id_table(), offset_first=True)
    check_equal(out, sources, params, crop, ref.cs_id_table())
    assert (out[1][0] == 255).any() and float(out[0][0][:, -1, :].abs().max()) == 0.0      # the padding


def test_more_samples_than_one_launch_and_more_than_one_block_per_row(cuda):
    """18 samples (records travel 16 per launch) and a 260-pixel row (a block covers 256)."""
    rs = np.random.RandomState(2)
    crop = (6, 260)
    sizes = [(5 + i % 4, 200 + 7 * i) for i in range(18)]
    sources = [rand_source(rs, h, w) for h, w in sizes]
    params = [params_for(hw, [1.3, 1.0, 0.8][i % 3], crop, i % 2 == 0, i % 3 == 0) for i, hw in enumerate(sizes)]
    out = device_augment(cuda, sources, params, crop, ref.cs_id_table())
    check_equal(out, sources, params, crop, ref.cs_id_table())


def all_colours():
    lv = np.array(list(range(0, 248, 8)) + [255], dtype=np.uint8)
    assert len(lv) == 32
    b, g, r = np.meshgrid(lv, lv, lv, indexing="ij")
    return np.ascontiguousarray(np.stack([b, g, r], axis=-1).reshape(128, 256, 3))


PHOTOMETRIC = {
    "saturation_low": dict(saturation=0.75), "saturation_high": dict(saturation=1.25),
    "hue_minus": dict(hue=-18), "hue_plus": dict(hue=18), "hue_zero": dict(hue=0),
    "both": dict(saturation=1.1337, hue=-7), "both_high": dict(saturation=0.8123, hue=13),
    "bright_contrast_first": dict(shift=10, mode=1, contrast=0.75),
    "dark_contrast_first": dict(shift=-10, mode=1, contrast=1.25),
    "bright_contrast_last": dict(shift=10, mode=0, contrast=1.25),
    "dark_contrast_last": dict(shift=-10, mode=0, contrast=0.75),
    "everything_first": dict(shift=-10, mode=1, contrast=1.25, saturation=1.25, hue=18),
    "everything_last": dict(shift=10, mode=0, contrast=0.75, saturation=0.75, hue=-18),
}


def test_photometric(cuda):
    """All 32^3 colours on the levels {0, 8, ..., 240, 255}: every hue sector, V = 0, d = 0 and the hue wrap, under
    each parameter set, in one launch."""
    img = all_colours()
    names = list(PHOTOMETRIC)
    params = [P(dst_h=128, dst_w=256, **PHOTOMETRIC[k]) for k in names]
    sources = [(img, None)] * len(names)
    images, labels, hist = device_augment(cuda, sources, params, (128, 256))
    assert labels is None and hist is None
    for i, k in enumerate(names):
        want, _, _ = ref.augment(img, None, params[i], (128, 256))
        got = images[i].cpu().numpy()
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), "%s: %d of %d values differ, first at %s (bgr %s): %r != %r" % (
            k, bad.sum(), bad.size, np.argwhere(bad)[0], img[tuple(np.argwhere(bad)[0][1:])], got[bad][0], want[bad][0])
    plain, _, _ = ref.augment(img, None, P(dst_h=128, dst_w=256), (128, 256))
    assert not np.array_equal(plain, images[0].cpu().numpy())            # (the jitter did something)


@pytest.mark.parametrize("crop", [(32, 48), (33, 47)])
def test_histogram_and_balance_weights(cuda, crop):
    """One class absent, one on a single pixel, ignore and padding present: the histogram is exact, the weights are
    within rel 1e-6 of the float64 formula (fp64 pow to a few ulp against a difference >= 1e-8, then one fp32
    rounding: about 2e-7) and exactly 0 at ignore."""
    from dcfp_amd import ops
    rs = np.random.RandomState(4)
    sources, params = [], []
    for n in range(2):
        im, _ = rand_source(rs, 30, 44)
        lab = rs.choice([0, 1, 2, 5, 9, 18, 255], size=(30, 44), p=[.3, .2, .2, .1, .1, .05, .05]).astype(np.uint8)
        lab[7 + n, 11] = 3                                            # class 3: one pixel; class 7 (and others): absent
        sources.append((im, lab))
        params.append(P(dst_h=30, dst_w=44, flip=bool(n)))
    out = device_augment(cuda, sources, params, crop)
    check_equal(out, sources, params, crop)
    images, labels, hist = out
    h = hist.cpu().numpy()
    assert np.all(h[:, 3] == 1) and np.all(h[:, 7] == 0) and np.all(h.sum(1) == crop[0] * crop[1])
    assert np.all(h[:, 255] > crop[0] * crop[1] - 30 * 44)           # padding and ignore share the ignore bin
    lab_np = labels.cpu().numpy()
    for balance, targets in ((1, None), (2, [3, 0]), (2, [18, 3])):
        w = ops.balance_weight(labels, hist, 19, balance, 255, targets).cpu().numpy()
        assert w.dtype == np.float32 and w.shape == lab_np.shape
        for n in range(2):
            want = ref.balance_weight(lab_np[n], 19, balance, 255, None if targets is None else targets[n])
            assert want.dtype == np.float64
            ign = lab_np[n] == 255
            assert np.all(w[n][ign] == 0.0) and ign.any()
            rel = np.abs(w[n][~ign] - want[~ign]) / want[~ign]
            assert rel.max() <= 1e-6, (balance, targets, n, rel.max())
            assert w[n].max() <= 1.0 and (balance == 2 or w[n][lab_np[n] == 3].max() == 0.5)


def write_cs(tmp_path, sizes):
    from PIL import Image
    rs = np.random.RandomState(5)
    lines = []
    for i, size in enumerate(sizes):
        Image.fromarray(rs.randint(0, 256, size + (3,)).astype(np.uint8)).save(tmp_path / ("im%d.png" % i))
        Image.fromarray(rs.randint(0, 34, size).astype(np.uint8)).save(tmp_path / ("gt%d.png" % i))
        lines.append("im%d.png gt%d.png" % (i, i))
    (tmp_path / "train.lst").write_text("\n".join(lines) + "\n")
    return {"root": str(tmp_path), "list_path": str(tmp_path / "train.lst")}


def test_train_loader_end_to_end(cuda, tmp_path):
    """Two fixed-seed batches of TrainLoader = the reference on the same decoded arrays and the same draws."""
    from PIL import Image
    para = write_cs(tmp_path, [(40, 60), (50, 70), (33, 47), (64, 64)])
    crop, seed = (32, 36), 21
    ds = build_dataset("CS", split="train", crop_size=crop, scale=True, mirror=True, brightness=True, balance=1,
                       data_para=para)
    loader = TrainLoader(ds, 2, cuda, seed=seed, num_workers=2, rank=0, world_size=1)
    order, rng = loader.indices(0), random.Random(seed)
    assert sorted(order) == [0, 1, 2, 3] and len(loader) == 2
    cfg = base.AugConfig(crop[0], crop[1], scale=True, mirror=True, brightness=True)
    batches = list(loader)
    assert len(batches) == 2
    for b, (images, labels) in enumerate(batches):
        assert set(labels) == {"ori", "weight"} and images.shape == (2, 3) + crop and images.is_cuda
        for j, idx in enumerate(order[2 * b:2 * b + 2]):
            img = np.ascontiguousarray(np.asarray(Image.open(tmp_path / ("im%d.png" % idx)).convert("RGB"))[:, :, ::-1])
            lab = np.asarray(Image.open(tmp_path / ("gt%d.png" % idx)))
            p = base.draw_params(rng, img.shape[:2], cfg)
            want, want_l, _ = ref.augment(img, lab, p, crop, ref.cs_id_table())
            assert np.array_equal(images[j].cpu().numpy().view(np.uint32), want.view(np.uint32)), (b, j, p)
            assert np.array_equal(labels["ori"][j].cpu().numpy(), want_l), (b, j, p)
            want_w = ref.balance_weight(want_l, 19, 1)
            w = labels["weight"][j].cpu().numpy()
            assert np.all(w[want_l == 255] == 0.0)
            assert np.allclose(w, want_w, rtol=1e-6, atol=0.0), (b, j)
    ds0 = build_dataset("CS", split="train", crop_size=crop, data_para=para)        # balance 0: the plain label tensor
    images, labels = next(iter(TrainLoader(ds0, 2, cuda, seed=seed, num_workers=1, rank=0, world_size=1)))
    assert isinstance(labels, torch.Tensor) and labels.dtype == torch.int64 and labels.shape == (2,) + crop
    dsv = build_dataset("CS", split="val", data_para=write_cs(tmp_path, [(20, 28)] * 2))
    images, labels = next(iter(TrainLoader(dsv, 2, cuda, num_workers=1, rank=0, world_size=1, shuffle=False)))
    img = np.asarray(Image.open(tmp_path / "im1.png").convert("RGB"))
    lut = base.lut_b(None, ref.MEAN, ref.STD)
    assert np.array_equal(images[1].cpu().numpy(), np.stack([lut[c][img[:, :, c]] for c in range(3)]))
    assert np.array_equal(labels[1].cpu().numpy(), ref.cs_id_table()[np.asarray(Image.open(tmp_path / "gt1.png"))])


def test_train_driver_on_a_list_file(cuda, tmp_path):
    """tools/train.py --dataset CS with every augmentation on and the GSRL loss on real {'ori', 'weight'} labels."""
    para = write_cs(tmp_path, [(80, 100), (70, 90), (90, 120), (66, 130)])
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--model", "simple", "--ddp", "False",
           "--dataset", "CS", "--data-para", json.dumps(para), "--random-scale", "--random-mirror",
           "--random-brightness", "--balance", "1", "--loss-type", "gsrl", "--input-size", "65,65", "--batch-size", "2",
           "--num-steps", "2", "--snapshot-dir", str(tmp_path / "snap"), "--backbone-para",
           json.dumps({"pretrained": False}), "--learning-rate", "1e-3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    losses = [float(l.split("loss=")[1]) for l in r.stdout.splitlines() if "loss=" in l]
    assert len(losses) == 2 and all(np.isfinite(losses)), r.stdout[-2000:]
