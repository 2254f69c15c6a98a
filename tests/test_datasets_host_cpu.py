"""CPU: the host half of dcfp_amd.datasets - the random draws, the geometry tables and lookup tables
against tests/_augment_ref.py, the Cityscapes list parsing and decoding, the C-ABI's descriptor checks and the
driver's flags.  Nothing here launches a kernel."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import _augment_ref as ref
from dcfp_amd import _lib
from dcfp_amd.datasets import base, build_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ draw_params
def replay(seed, H, W, ch, cw):
    """The reference's __getitem__ draws (scale, jitter, crop, mirror all on), written out by hand."""
    r = random.Random(seed)
    out = {}
    f = 0.5 + r.randint(0, 15) / 10.0
    out["f"] = f
    dh, dw = int(round(H * f)), int(round(W * f))
    out["shift"] = None if r.random() < 0.5 else r.randint(-10, 10)
    out["mode"] = r.randint(0, 1)
    out["contrast"] = None
    if out["mode"] == 1:
        out["contrast"] = None if r.random() < 0.5 else r.uniform(0.75, 1.25)
    out["saturation"] = None if r.random() < 0.5 else r.uniform(0.75, 1.25)
    out["hue"] = None if r.random() < 0.5 else r.randint(-18, 18)
    if out["mode"] == 0:
        out["contrast"] = None if r.random() < 0.5 else r.uniform(0.75, 1.25)
    out["h_off"] = r.randint(0, max(dh, ch) - ch)
    out["w_off"] = r.randint(0, max(dw, cw) - cw)
    out["flip"] = r.randint(0, 1) * 2 - 1 == -1
    out["next"] = r.random()
    return out


def _seeds():
    """three seeds: brightness skipped with mode 0, brightness drawn with mode 1, and one more of each mode"""
    found = {}
    for seed in range(200):
        e = replay(seed, 100, 200, 64, 64)
        found.setdefault((e["shift"] is None, e["mode"]), seed)
    return [found[(True, 0)], found[(False, 1)], found[(True, 1)], found[(False, 0)]]


@pytest.mark.parametrize("seed", _seeds())
def test_draw_params_replays_the_reference_order(seed):
    cfg = base.AugConfig(64, 64, scale=True, mirror=True, brightness=True)
    e = replay(seed, 100, 200, 64, 64)
    rng = random.Random(seed)
    p = base.draw_params(rng, (100, 200), cfg)
    assert (p.f_scale, p.shift, p.mode, p.contrast, p.saturation, p.hue, p.h_off, p.w_off, p.flip) == \
        (e["f"], e["shift"], e["mode"], e["contrast"], e["saturation"], e["hue"], e["h_off"], e["w_off"], e["flip"])
    assert (p.dst_h, p.dst_w) == (int(round(100 * e["f"])), int(round(200 * e["f"])))
    assert rng.random() == e["next"]                 # and not one draw more or less


def test_draw_params_draws_nothing_for_disabled_steps():
    rng = random.Random(5)
    p = base.draw_params(rng, (40, 50), base.AugConfig(40, 50))
    assert p == base.AugParams(dst_h=40, dst_w=50)
    r = random.Random(5)
    r.randint(0, 0), r.randint(0, 0)                 # the two crop offsets are always drawn
    assert rng.random() == r.random()
    p = base.draw_params(random.Random(1), (100, 200), base.AugConfig(64, 64, scale=True, long_size=300))
    k = random.Random(1).randint(0, 15)
    assert p.f_scale == int(300 * (0.5 + k / 10.0) + 0.5) / 200
    p = base.draw_params(random.Random(1), (100, 200), base.AugConfig(64, 64, scale=True, short_size=80))
    assert p.f_scale == int(80 * (0.5 + k / 10.0) + 0.5) / 100


# ------------------------------------------------------------------ tables
def gather(img, lab, cols, rows):
    """What the device does with the two tables, in numpy integers: (uint8 [ch,cw,3], int64 [ch,cw], pad mask)."""
    H, W = img.shape[:2]
    S = img.astype(np.int64)
    pad = (rows[:, 0] < 0)[:, None] | (cols[:, 0] < 0)[None, :]
    sx0 = np.clip(cols[:, 0], 0, W - 1); sx1 = np.minimum(sx0 + 1, W - 1)
    sy0 = np.clip(rows[:, 0], 0, H - 1); sy1 = np.minimum(sy0 + 1, H - 1)
    a0, a1 = cols[:, 1].astype(np.int64)[None, :, None], cols[:, 2].astype(np.int64)[None, :, None]
    b0, b1 = rows[:, 1].astype(np.int64)[:, None, None], rows[:, 2].astype(np.int64)[:, None, None]
    h0 = S[sy0][:, sx0] * a0 + S[sy0][:, sx1] * a1
    h1 = S[sy1][:, sx0] * a0 + S[sy1][:, sx1] * a1
    out = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
    l = lab[np.clip(rows[:, 3], 0, H - 1)][:, np.clip(cols[:, 3], 0, W - 1)].astype(np.int64)
    l[pad] = 255
    return out.astype(np.uint8), l, pad


@pytest.mark.parametrize("f", [0.5, 1.0, 1.3, 2.0])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("at_max", [False, True])
def test_tables_against_the_reference(f, flip, at_max):
    """The crop through the tables = the reference's resize -> pad -> crop -> mirror; crop 33x41 exceeds the scaled
    37x53 source at f = 0.5 (18x26: padding at the bottom and right)."""
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    lab = rs.randint(0, 19, (37, 53)).astype(np.uint8)
    ch, cw = 33, 41
    dh, dw = int(round(37 * f)), int(round(53 * f))
    p = base.AugParams(f_scale=f, dst_h=dh, dst_w=dw, flip=flip,
                       h_off=(max(dh, ch) - ch) if at_max else 0, w_off=(max(dw, cw) - cw) if at_max else 0)
    cols = base.axis_table(53, dw, f, cw, p.w_off, flip)
    rows = base.axis_table(37, dh, f, ch, p.h_off)
    assert cols.dtype == np.int32 and cols.shape == (cw, 4) and rows.shape == (ch, 4)
    got, got_l, pad = gather(img, lab, cols, rows)
    # the reference with an identity normalisation (mean 0, std 1/255 would round): compare uint8 through LUT B instead
    lut = base.lut_b(None, ref.MEAN, ref.STD)
    want, want_l, _ = ref.augment(img, lab, p, (ch, cw))
    mine = np.stack([lut[c][got[:, :, 2 - c]] for c in range(3)])
    mine[:, pad] = 0.0
    assert np.array_equal(mine, want)
    assert np.array_equal(got_l, want_l)
    assert pad.any() == (f == 0.5)
    inside = cols[cols[:, 0] >= 0]
    assert np.all(inside[:, 1] + inside[:, 2] == 2048) and inside[:, 0].max() <= 52 and inside[:, 3].max() <= 52


def test_tables_of_a_one_pixel_wide_source():
    t = base.resize_taps(1, 3, 2.6)
    assert np.array_equal(t, np.array([[0, 2048, 0, 0]] * 3, dtype=np.int32))


# ------------------------------------------------------------------ lookup tables
def test_lut_b_identity_is_input_transform_of_arange_bit_for_bit():
    lut = base.lut_b(base.AugParams(), ref.MEAN, ref.STD)
    image = np.repeat(np.arange(256, dtype=np.uint8).reshape(256, 1, 1), 3, axis=2)
    image = image.astype(np.float32)[:, :, ::-1]
    image = image / 255.0
    image -= [0.485, 0.456, 0.406]
    image /= [0.229, 0.224, 0.225]
    assert lut.dtype == np.float32 and lut.shape == (3, 256)
    for c in range(3):
        assert np.array_equal(lut[c].view(np.uint32), np.ascontiguousarray(image[:, 0, c]).view(np.uint32))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shift,alpha", [(10, 0.75), (-10, 1.25), (None, 1.1), (7, None)])
def test_luts_compose_to_the_reference_chain(mode, shift, alpha):
    p = base.AugParams(dst_h=1, dst_w=256, shift=shift, mode=mode, contrast=alpha)
    img = np.repeat(np.arange(256, dtype=np.uint8).reshape(1, 256, 1), 3, axis=2)
    want, _, _ = ref.augment(img, None, p, (1, 256))
    a = base.lut_a(p)
    u = np.arange(256) if a is None else a
    got = base.lut_b(p, ref.MEAN, ref.STD)[:, u]
    assert np.array_equal(got.view(np.uint32), want[:, 0, :].view(np.uint32))
    if shift is None and (mode == 0 or alpha is None):
        assert a is None


# ------------------------------------------------------------------ Cityscapes
def _write_cs(tmp_path, n=3, size=(12, 20)):
    from PIL import Image
    rs = np.random.RandomState(0)
    lines, arrays = [], []
    for i in range(n):
        rgb = rs.randint(0, 256, size + (3,)).astype(np.uint8)
        ids = rs.randint(0, 34, size).astype(np.uint8)
        os.makedirs(tmp_path / "img" / "a", exist_ok=True)
        os.makedirs(tmp_path / "gt" / "a", exist_ok=True)
        Image.fromarray(rgb).save(tmp_path / "img" / "a" / ("s%d_leftImg8bit.png" % i))
        Image.fromarray(ids).save(tmp_path / "gt" / "a" / ("s%d_gtFine_labelIds.png" % i))
        lines.append("img/a/s%d_leftImg8bit.png gt/a/s%d_gtFine_labelIds.png" % (i, i))
        arrays.append((rgb, ids))
    (tmp_path / "train.lst").write_text("\n".join(lines) + "\n")
    return arrays


def test_cs_list_parsing_and_decoding(tmp_path):
    arrays = _write_cs(tmp_path)
    para = {"root": str(tmp_path), "list_path": str(tmp_path / "train.lst")}
    ds = build_dataset("CS", split="train", crop_size=(8, 8), scale=True, mirror=True, brightness=True, balance=1,
                       data_para=para)
    assert len(ds) == 3 and ds.num_classes == 19 and ds.ignore_label == 255 and ds.balance == 1
    assert ds.files[1] == {"img": str(tmp_path / "img/a/s1_leftImg8bit.png"),
                           "label": str(tmp_path / "gt/a/s1_gtFine_labelIds.png"), "name": "s1_gtFine_labelIds"}
    assert ds.cmap_labels.shape == (19, 3) and len(ds.class_weights) == 19
    img, lab = ds.decode(2)
    assert img.dtype == np.uint8 and np.array_equal(img, arrays[2][0][:, :, ::-1])      # BGR, as cv2.imread gives it
    assert lab.dtype == np.uint8 and np.array_equal(lab, arrays[2][1])
    ds = build_dataset("CS", split="train", crop_size=(8, 8), data_para=dict(para, max_iters=7))
    assert len(ds) == 9                                                                 # 3 * ceil(7 / 3)
    ds = build_dataset("CS", split="test", data_para=para)
    assert ds.files[0] == {"img": str(tmp_path / "img/a/s0_leftImg8bit.png"), "name": "s0_leftImg8bit"}
    assert ds.decode(0)[1] is None
    with pytest.raises(ValueError):
        build_dataset("CS", data_para={"root": str(tmp_path)})
    with pytest.raises(NotImplementedError):
        build_dataset("ADE", data_para=para)
    with pytest.raises(NotImplementedError):
        build_dataset("CS", data_para=dict(para, resample=True))


def test_id2trainid_and_reverse(tmp_path):
    _write_cs(tmp_path, n=1)
    ds = build_dataset("CS", data_para={"root": str(tmp_path), "list_path": str(tmp_path / "train.lst")})
    ids = np.arange(34, dtype=np.uint8).reshape(2, 17)
    train = ds.id2trainId(ids)
    assert np.array_equal(train.reshape(-1), ref.cs_id_table()[:34])
    assert np.array_equal(ds.id_table(), ref.cs_id_table())
    assert sorted(set(train.reshape(-1).tolist())) == list(range(19)) + [255]
    back = ds.id2trainId(train, reverse=True)
    valid = train != 255
    assert np.array_equal(back[valid], ids[valid])          # the 19 classes return to their ids
    assert np.all(back[~valid] == 30)                        # ignore returns to the last id that maps to it


def test_loader_shards_like_distributed_sampler(tmp_path):
    import torch
    from torch.utils.data.distributed import DistributedSampler
    from dcfp_amd.datasets import TrainLoader
    _write_cs(tmp_path, n=3)
    ds = build_dataset("CS", split="train", data_para={"root": str(tmp_path), "list_path": str(tmp_path / "train.lst"),
                                                       "max_iters": 7})
    for rank in range(2):
        loader = TrainLoader(ds, 2, torch.device("cpu"), seed=11, num_workers=1, rank=rank, world_size=2)
        s = DistributedSampler(ds, num_replicas=2, rank=rank, shuffle=True, seed=11)
        for epoch in (0, 3):
            s.set_epoch(epoch)
            assert loader.indices(epoch) == list(iter(s))
        assert len(loader) == 2                              # 9 samples -> 5 per rank -> 2 full batches


# ------------------------------------------------------------------ C-ABI
def test_bad_descriptors_are_refused_on_the_host():
    L = _lib.lib()
    aug, bal = L.dcfp_augment_u8_to_f32_nchw, L.dcfp_balance_weight_f32
    P = ctypes.c_void_p

    def sample(**kw):
        f = dict(image=0x1000, label=0x2000, src_h=8, src_w=8, col_off=0, row_off=16, lut_a_off=-1, lut_b_off=0,
                 hsv_flags=0, hue_delta=0, sat_alpha=1.0, pad_=0)
        f.update(kw)
        return (_lib.AugSample * 1)(_lib.AugSample(**f))

    def call(s, N=1, ch=16, cw=16, taps=0x3000, n_taps=32, lut_a=None, a_bytes=0, lut_b=0x4000, b_floats=768,
             ignore=255, images=0x5000, labels=0x6000, hist=0x7000):
        return aug(s, N, ch, cw, P(taps), n_taps, lut_a, a_bytes, P(lut_b), b_floats, None, ignore, P(images),
                   P(labels) if labels else None, P(hist) if hist else None, None)
    E = _lib.E_BADDESC
    assert call(sample(), N=0) == E
    assert call(None) == E
    assert call(sample(col_off=16, row_off=0), cw=17) == E                     # the crop is wider than the column table
    assert call(sample(), ch=17) == E                        # ... taller than the row table
    assert call(sample(col_off=-1)) == E
    assert call(sample(image=None)) == E                     # a null image
    assert call(sample(label=None)) == E                     # labels asked for, none given
    assert call(sample(src_w=0)) == E
    assert call(sample(lut_b_off=1)) == E                    # LUT B ends past the table
    assert call(sample(lut_a_off=0)) == E                    # LUT A named, no table
    assert call(sample(hsv_flags=4)) == E
    assert call(sample(), ignore=256) == E
    assert call(sample(), taps=0x3004) == E                  # records are read 16 bytes at a time
    assert call(sample(), labels=None) == E                  # a histogram without labels
    for balance in (-1, 3):
        assert bal(P(0x1000), P(0x2000), None, 1, 64, 19, 255, balance, 0.9999, P(0x3000), None) == E
    assert bal(P(0x1000), P(0x2000), None, 0, 64, 19, 255, 1, 0.9999, P(0x3000), None) == E      # N <= 0
    assert bal(None, P(0x2000), None, 1, 64, 19, 255, 1, 0.9999, P(0x3000), None) == E
    assert bal(P(0x1000), P(0x2000), None, 1, 64, 19, 255, 2, 0.9999, P(0x3000), None) == E      # balance 2, no target
    assert bal(P(0x1000), P(0x2000), None, 1, 64, 300, 255, 1, 0.9999, P(0x3000), None) == E
    assert bal(None, None, None, 1, 64, 19, 255, 0, 0.9999, None, None) == 0                      # balance 0: nothing to do
    assert L.dcfp_abi_version() == 2


def test_wrappers_have_no_cpu_path():
    import torch
    from dcfp_amd import ops
    with pytest.raises(RuntimeError):
        ops.augment_batch([torch.zeros(4, 4, 3, dtype=torch.uint8)], None, [(0, 4, -1, 0, 0, 0, 1.0)],
                          torch.zeros(8, 4, dtype=torch.int32), None, torch.zeros(768), None, (4, 4))
    with pytest.raises(RuntimeError):
        ops.balance_weight(torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(1, 256, dtype=torch.int32), 19, 1)


# ------------------------------------------------------------------ driver
def test_train_help_lists_the_data_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train.py"), "--help"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--dataset", "--data-dir", "--random-scale", "--random-mirror", "--random-brightness", "--balance",
                 "--longsize", "--shortsize", "--data-para"):
        assert flag in r.stdout, flag
