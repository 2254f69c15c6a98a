"""BaseDataSet: the host half of the device-side training augmentation.

The reference's `datasets/Base.py` runs its train-split chain (id -> trainId, random scale, photometric jitter,
input_transform, pad + random crop, mirror, get_label) with cv2 on CPU workers.  Here the host only draws the random
parameters (`draw_params`, the reference's draws in the reference's order) and folds them into small tables
(`pack_batch`); `dcfp_amd/csrc/augment.hip` does the per-pixel work.  The image path is defined as integer and
lookup-table arithmetic, so the device result is defined bit for bit:

  resize   destination size round(H*f), round(W*f) (half to even); per destination column, in float64 then float32,
           fx = float32((dx+0.5)/f - 0.5), sx = floor(fx), fx -= sx, clamped to (0, 0) / (W-1, 0) at the borders,
           coefficients rint((1-fx)*2048), rint(fx*2048); rows alike; the device combines
           h = S[sx]*a0 + S[sx+1]*a1, out = (((b0*(h0>>4))>>16) + ((b1*(h1>>4))>>16) + 2) >> 2.
           The label takes min(floor(dx/f), W-1).  This is MODELLED on OpenCV's 8-bit linear resize as read from
           memory; it has not been compared with cv2 and no bit parity with cv2 is claimed: the contract is the formula.
  LUT A    brightness clip(u+shift), then contrast clip(rint(float32(u)*float32(alpha))) when mode == 1.
  HSV      ONE BGR -> HSV -> BGR round trip in fp32 that applies saturation and hue together, only when one of them
           fired.  The reference makes two cv2 round trips with a uint8 image between them: a documented deviation.
  LUT B    contrast when mode == 0, then input_transform (Base.py:91-96), built by running the reference's numpy
           statements on arange(256).
  tables   crop offset, mirror and padding folded into one column and one row table per sample.

The `resample` sampler (`resample=True`, the reference's fine-tune recipes): `tools/label_index.py` writes
label_index_<DATASET>.pkl (per class, the files that hold it); `gen_index` builds the epoch index from it (every class
as often as the most frequent one, `locate(index) -> (file, class)`); the crop is placed on a random pixel of a random
8-connected component of that class on the scaled, padded label (`draw_pre` / `draw_crop`; the labelling and the pixel
selection are ops.label_components / ops.component_pixel, csrc/components.hip) and `balance=2` takes the class as its
target.  Out of scope: any claim of bit parity with cv2, its component numbering included.
"""
import os
import pickle
import random
from dataclasses import dataclass
from typing import Optional

import numpy as np

COEF_ONE = 2048


@dataclass
class AugParams:
    """One sample's random draws (the parameter record shared with the tests' reference)."""
    f_scale: float = 1.0
    dst_h: int = 0
    dst_w: int = 0
    shift: Optional[int] = None          # brightness; None: skipped
    mode: int = 0                        # 1: contrast before saturation / hue, 0: after
    contrast: Optional[float] = None
    saturation: Optional[float] = None
    hue: Optional[int] = None
    h_off: int = 0
    w_off: int = 0
    flip: bool = False


@dataclass
class AugConfig:
    crop_h: int
    crop_w: int
    scale: bool = False
    mirror: bool = False
    brightness: bool = False
    long_size: int = -1
    short_size: int = -1


def draw_params(rng, src_hw, cfg):
    """The reference's draws in the reference's order (Base.py:98-110, 112-182, 203-222, 240-258) from a
    random.Random; a step that returns early draws nothing more."""
    p = draw_pre(rng, src_hw, cfg)
    p.h_off = rng.randint(0, max(p.dst_h, cfg.crop_h) - cfg.crop_h)
    p.w_off = rng.randint(0, max(p.dst_w, cfg.crop_w) - cfg.crop_w)
    if cfg.mirror:
        p.flip = rng.randint(0, 1) * 2 - 1 < 0          # image[:, :, ::flip]
    return p


def draw_pre(rng, src_hw, cfg):
    """The draws before the crop: scale and photometric jitter."""
    H, W = int(src_hw[0]), int(src_hw[1])
    p = AugParams(dst_h=H, dst_w=W)
    if cfg.scale:
        f = 0.5 + rng.randint(0, 15) / 10.0
        if cfg.long_size > 0:
            f = int(cfg.long_size * f + 0.5) * 1.0 / max(H, W)
        elif cfg.short_size > 0:
            f = int(cfg.short_size * f + 0.5) * 1.0 / min(H, W)
        p.f_scale, p.dst_h, p.dst_w = f, max(1, int(round(H * f))), max(1, int(round(W * f)))
    if cfg.brightness:
        if not rng.random() < 0.5:
            p.shift = rng.randint(-10, 10)
        p.mode = rng.randint(0, 1)

        def contrast():
            if not rng.random() < 0.5:
                p.contrast = rng.uniform(0.75, 1.25)
        if p.mode == 1:
            contrast()
        if not rng.random() < 0.5:
            p.saturation = rng.uniform(0.75, 1.25)
        if not rng.random() < 0.5:
            p.hue = rng.randint(-18, 18)
        if p.mode == 0:
            contrast()
    return p


def crop_steps(rng, p, cfg):
    """The `resample` crop and mirror draws of one sample, in the reference's order (Base.py:203-222, 253-256), as a
    generator of the questions only the device can answer: it yields ("count",) and is sent the number C of
    components of the sample's class (the reference's nums - 1); with C >= 1 it draws n in 1..C, yields ("size", n)
    and is sent that component's pixel count, draws k, yields ("pixel", n, k) and is sent (y, x), then makes the two
    jitter draws; with C == 0 it makes the two plain draws.  Clipping and the mirror draw follow.  Fills p.h_off,
    p.w_off, p.flip and returns the chosen pixel or None.  A batch advances its samples' generators in step, so that
    each question costs one device call for all of them (loader.TrainLoader)."""
    Hp, Wp = max(p.dst_h, cfg.crop_h), max(p.dst_w, cfg.crop_w)
    pixel = None
    count = yield ("count",)
    if count >= 1:
        n = rng.randint(1, count)
        size = yield ("size", n)
        k = rng.randint(0, size - 1)
        pixel = yield ("pixel", n, k)
        pixel = (int(pixel[0]), int(pixel[1]))
        h_off = pixel[0] - cfg.crop_h // 2 - rng.randint(-(cfg.crop_h // 4), cfg.crop_h // 4)
        w_off = pixel[1] - cfg.crop_w // 2 - rng.randint(-(cfg.crop_w // 4), cfg.crop_w // 4)
    else:
        h_off = rng.randint(0, Hp - cfg.crop_h)
        w_off = rng.randint(0, Wp - cfg.crop_w)
    p.h_off = min(max(h_off, 0), Hp - cfg.crop_h)
    p.w_off = min(max(w_off, 0), Wp - cfg.crop_w)
    if cfg.mirror:
        p.flip = rng.randint(0, 1) * 2 - 1 < 0
    return pixel


def draw_crop(rng, p, cfg, counts_cb):
    """crop_steps for one sample on its own: `counts_cb(question)` answers ("count",), ("size", n) and
    ("pixel", n, k) as each draw needs it.  -> the chosen pixel or None."""
    steps = crop_steps(rng, p, cfg)
    try:
        q = next(steps)
        while True:
            q = steps.send(counts_cb(q))
    except StopIteration as done:
        return done.value


def index_seed(seed, epoch):
    """The seed of one epoch's index: plain integer arithmetic, the same in every process (hash() is salted)."""
    return int(seed) * 1000003 + int(epoch)


def resize_taps(src_n, dst_n, f):
    """[dst_n, 4] int32 (src, c0, c1, lsrc) of one axis of the resize; f == 1 is the identity."""
    d = np.arange(dst_n, dtype=np.float64)
    fx = ((d + 0.5) / f - 0.5).astype(np.float32)
    sx = np.floor(fx)
    fx = fx - sx
    sx = sx.astype(np.int64)
    lo, hi = sx < 0, sx >= src_n - 1
    fx[lo | hi] = 0.0
    sx[lo] = 0
    sx[hi] = src_n - 1
    t = np.empty((dst_n, 4), dtype=np.int32)
    t[:, 0] = sx
    t[:, 1] = np.rint((np.float32(1.0) - fx) * np.float32(COEF_ONE))
    t[:, 2] = np.rint(fx * np.float32(COEF_ONE))
    t[:, 3] = np.minimum(np.floor(d / f), src_n - 1)
    return t


def axis_table(src_n, dst_n, f, crop_n, off, flip=False):
    """The crop's view of one axis: record i describes output pixel i (mirror, crop offset and padding folded in)."""
    taps = resize_taps(src_n, dst_n, f)
    o = np.arange(crop_n)
    if flip:
        o = crop_n - 1 - o
    pos = off + o
    inside = pos < dst_n
    t = np.empty((crop_n, 4), dtype=np.int32)
    t[:] = (-1, 0, 0, -1)
    t[inside] = taps[pos[inside]]
    return t


def _u8(x):
    return np.clip(np.around(x), 0, 255).astype(np.uint8)


def brightness_lut(u, shift):
    img = u.astype(np.float32)
    img[:] += shift
    return _u8(img)


def contrast_lut(u, alpha):
    img = u.astype(np.float32)
    img = img * alpha                               # float32 array * Python float: a float32 product
    return _u8(img)


def lut_a(p):
    """uint8 [256], or None when it is the identity."""
    if p.shift is None and not (p.mode == 1 and p.contrast is not None):
        return None
    u = np.arange(256, dtype=np.uint8)
    if p.shift is not None:
        u = brightness_lut(u, p.shift)
    if p.mode == 1 and p.contrast is not None:
        u = contrast_lut(u, p.contrast)
    return u


def lut_b(p, mean, std):
    """float32 [3, 256]: row c is output plane c (R, G, B).  The statements of input_transform on arange(256)."""
    u = np.arange(256, dtype=np.uint8)
    if p is not None and p.mode == 0 and p.contrast is not None:
        u = contrast_lut(u, p.contrast)
    image = np.repeat(u.reshape(256, 1, 1), 3, axis=2)
    image = image.astype(np.float32)[:, :, ::-1]
    image = image / 255.0
    image -= mean
    image /= std
    return np.ascontiguousarray(image[:, 0, :].T)


def pack_batch(params, src_hws, cfg, mean, std):
    """-> (taps int32 [T,4], lut_a uint8 [A] or None, lut_b float32 [N*768], records) for ops.augment_batch;
    records[i] = (col_off, row_off, lut_a_off, lut_b_off, hsv_flags, hue_delta, sat_alpha)."""
    taps, las, lbs, recs = [], [], [], []
    n_taps = n_a = 0
    for p, (H, W) in zip(params, src_hws):
        taps.append(axis_table(W, p.dst_w, p.f_scale, cfg.crop_w, p.w_off, p.flip))
        taps.append(axis_table(H, p.dst_h, p.f_scale, cfg.crop_h, p.h_off))
        col_off, row_off = n_taps, n_taps + cfg.crop_w
        n_taps += cfg.crop_w + cfg.crop_h
        a = lut_a(p)
        a_off = -1
        if a is not None:
            a_off = n_a
            las.append(a)
            n_a += 256
        lbs.append(lut_b(p, mean, std).reshape(-1))
        flags = (1 if p.saturation is not None else 0) | (2 if p.hue is not None else 0)
        recs.append((col_off, row_off, a_off, 768 * (len(lbs) - 1), flags, p.hue or 0,
                     float(np.float32(p.saturation if p.saturation is not None else 1.0))))
    return (np.ascontiguousarray(np.concatenate(taps)), np.concatenate(las) if las else None,
            np.concatenate(lbs).astype(np.float32), recs)


def bitrev_palette(n, first=1):
    """uint8 [n, 3] RGB: the bit-reversal colour map of PASCAL VOC tooling, entries first .. first + n - 1.  Bit k of
    the entry's index (k = 0, 1, 2 in turn, three bits per round) goes to the highest free bit of R, G, B: distinct
    indices below 256 give distinct colours, and only index 0 is black."""
    out = np.zeros((n, 3), dtype=np.uint8)
    for row in range(n):
        v, bit = row + first, 7
        while v and bit >= 0:
            for ch in range(3):
                out[row, ch] |= ((v >> ch) & 1) << bit
            v >>= 3
            bit -= 1
    return out


class BaseDataSet:
    """Configuration and host-side table building of one dataset; subclasses provide `files`, `num_classes`,
    `class_weights` and `id_to_trainid`."""

    def __init__(self, split="train", crop_size=(321, 321), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                 scale=True, mirror=True, brightness=True, ignore_label=255, balance=0, longsize=-1, shortsize=-1,
                 **kwargs):
        if balance not in (0, 1, 2):
            raise ValueError("balance must be 0, 1 or 2")
        self.resample = bool(kwargs.get("resample", False))
        self.seed = int(kwargs.get("seed", 0))         # of the epoch index; TrainLoader sets its own
        self.class_files = None
        self.file_index, self.class_index = [], []
        self.split = split
        self.crop_h, self.crop_w = crop_size
        self.mean, self.std = list(mean), list(std)
        self.scale, self.is_mirror, self.brightness = scale, mirror, brightness
        self.ignore_label = ignore_label
        self.balance = balance
        self.beta = kwargs.get("beta", 0.9999)
        self.long_size, self.short_size = longsize, shortsize
        self.files = []
        self.id_to_trainid = {}

    def __len__(self):
        if self.resample:
            return int(self.class_files["label_f"].max() * self.num_classes)
        return len(self.files)

    def load_index(self, path):
        """label_index_<DATASET>.pkl of tools/label_index.py (or of the reference's label_index.py): {str(class):
        [{'idx': file index, 'name': ...}], 'label_f': float64 [num_classes] list lengths}."""
        if not os.path.isfile(path):
            raise NotImplementedError("resample=True needs the class index %s, which does not exist: write it with "
                                      "tools/label_index.py" % path)
        with open(path, "rb") as f:
            self.class_files = pickle.load(f)
        for c in range(self.num_classes):
            if len(self.class_files.get(str(c), ())) == 0:
                raise ValueError("%s: class %d is in no file of the list, the resample index cannot balance it"
                                 % (path, c))
        self.gen_index(0)

    def gen_index(self, epoch=0):
        """Base.py:43-58: every class `length` times, its files in turn and a random sample for the remainder.  The
        draws come from a generator seeded by (seed, epoch): every rank builds the same index without a broadcast."""
        rng = random.Random(index_seed(self.seed, epoch))
        length = int(self.class_files["label_f"].max())
        self.file_index, self.class_index = [], []
        for c in range(self.num_classes):
            len_c = len(self.class_files[str(c)])
            self.file_index += list(range(len_c)) * (length // len_c) + rng.sample(list(range(len_c)), length % len_c)
            self.class_index += [c] * length

    def pre_processing(self, epoch, max_epoch=None):
        if self.resample:
            self.gen_index(epoch)

    def locate(self, index):
        """-> (index into `files`, class the sample was drawn for or None)."""
        if not self.resample:
            return index, None
        c = self.class_index[index]
        return int(self.class_files[str(c)][self.file_index[index]]["idx"]), c

    @property
    def aug_config(self):
        train = self.split == "train"
        return AugConfig(self.crop_h, self.crop_w, train and self.scale, train and self.is_mirror,
                         train and self.brightness, self.long_size, self.short_size)

    def draw_params(self, rng, src_hw):
        """train: the random draws; val / test: the identity (no scale, no jitter, crop = source, Base.py:228-238)."""
        if self.split == "train":
            return draw_params(rng, src_hw, self.aug_config)
        return AugParams(dst_h=int(src_hw[0]), dst_w=int(src_hw[1]))

    def id_table(self):
        """uint8 [256]: raw id -> trainId (ids the table does not name stay as they are)."""
        t = np.arange(256, dtype=np.uint8)
        for k, v in self.id_to_trainid.items():
            if 0 <= k < 256:
                t[k] = v
        return t

    def id2trainId(self, label, reverse=False):
        """CSdatasets.py:71-79; a value the label's dtype cannot hold (the id -1 in a uint8 map) wraps, as it did there."""
        label_copy = label.copy()
        for k, v in self.id_to_trainid.items():
            if reverse:
                k, v = v, k
            label_copy[label == k] = np.array(v).astype(label_copy.dtype)
        return label_copy

    def decode(self, index):
        """-> (uint8 [H,W,3] BGR, uint8 [H,W] raw ids or None): cv2.imread(IMREAD_COLOR / IMREAD_GRAYSCALE) through PIL
        (PNG is lossless; a JPEG goes through PIL's decoder, and no pixel parity with cv2's is claimed)."""
        from PIL import Image
        item = self.files[index]
        with Image.open(item["img"]) as im:
            image = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[:, :, ::-1])
        label = None
        if "label" in item:
            with Image.open(item["label"]) as im:
                label = np.ascontiguousarray(np.asarray(im.convert("L"), dtype=np.uint8))
            if label.shape != image.shape[:2]:
                raise ValueError("%s: label size %s differs from image size %s" % (item["name"], label.shape, image.shape[:2]))
        return image, label

    def pack_batch(self, params, src_hws, crop_size=None):
        cfg = self.aug_config
        if crop_size is not None:
            cfg.crop_h, cfg.crop_w = crop_size
        return pack_batch(params, src_hws, cfg, self.mean, self.std)


class NameListDataSet(BaseDataSet):
    """A dataset whose list file holds one sample name per line (Pascal-Context, COCO-Stuff): images at
    root/images/<name>.jpg, labels at root/<LABEL_DIR>/<name><LABEL_SUFFIX>, raw label 0 unlabelled and raw k the class
    k - 1.  Subclasses set KEY (of label_index_<KEY>.pkl), NUM_CLASSES, LABEL_DIR and LABEL_SUFFIX."""
    KEY = NUM_CLASSES = LABEL_DIR = LABEL_SUFFIX = None
    class_weights = None

    def __init__(self, root, list_path, max_iters=None, split="train", crop_size=(321, 321),
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), scale=True, mirror=True, brightness=True,
                 ignore_label=255, balance=0, longsize=-1, shortsize=-1, **kwargs):
        if split not in ("train", "val"):
            raise NotImplementedError("%s: split %r is not built (train and val are)" % (self.KEY, split))
        if ignore_label != 255:
            # the reference shifts the uint8 map by one (0 - 1 wraps to 255): the table below is that only at 255
            raise ValueError("%s: ignore_label must be 255, the value raw label 0 maps to (got %r)"
                             % (self.KEY, ignore_label))
        super().__init__(split=split, crop_size=crop_size, mean=mean, std=std, scale=scale, mirror=mirror,
                         brightness=brightness, ignore_label=ignore_label, balance=balance, longsize=longsize,
                         shortsize=shortsize, **kwargs)
        self.num_classes = self.NUM_CLASSES
        self.root, self.list_path = root, list_path
        self.id_to_trainid = {0: ignore_label}
        self.id_to_trainid.update({k: k - 1 for k in range(1, 256)})
        self.cmap_labels = bitrev_palette(self.num_classes, first=1)
        with open(list_path) as f:
            self.img_ids = [line.strip() for line in f if line.strip()]
        if max_iters is not None:
            self.img_ids = self.img_ids * int(np.ceil(float(max_iters) / len(self.img_ids)))
        self.files = [{"img": os.path.join(root, "images", name + ".jpg"),
                       "label": os.path.join(root, self.LABEL_DIR, name + self.LABEL_SUFFIX), "name": name}
                      for name in self.img_ids]
        if self.resample:
            self.load_index(os.path.join(os.path.dirname(list_path), "label_index_%s.pkl" % self.KEY))
