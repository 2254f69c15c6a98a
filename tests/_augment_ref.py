"""The augmentation contract restated in numpy: integers and float32, one statement per operation, whole
images at a time (resize the source, jitter it, normalise, pad, crop, mirror, weigh) the way datasets/Base.py:224-261
orders it - not the table-driven gather the device runs.  It takes nothing from dcfp_amd but the parameter record."""
import numpy as np

from dcfp_amd.datasets.base import AugParams  # noqa: F401  (the parameter record only)

F32 = np.float32
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
CS_TRAIN_IDS = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13,
                27: 14, 28: 15, 31: 16, 32: 17, 33: 18}


def cs_id_table(ignore_label=255):
    t = np.arange(256, dtype=np.uint8)
    for k in range(34):
        t[k] = CS_TRAIN_IDS.get(k, ignore_label)
    return t


def axis_coefficients(src_n, dst_n, f):
    """(index of the first tap, coefficient of it, coefficient of the next) per destination position."""
    idx = np.zeros(dst_n, dtype=np.int64)
    c0 = np.zeros(dst_n, dtype=np.int64)
    c1 = np.zeros(dst_n, dtype=np.int64)
    for dx in range(dst_n):
        fx = F32((dx + 0.5) / f - 0.5)
        sx = int(np.floor(fx))
        fx = F32(fx - F32(sx))
        if sx < 0:
            sx, fx = 0, F32(0)
        if sx >= src_n - 1:
            sx, fx = src_n - 1, F32(0)
        idx[dx] = sx
        c0[dx] = int(np.rint(F32(F32(1) - fx) * F32(2048)))
        c1[dx] = int(np.rint(fx * F32(2048)))
    return idx, c0, c1


def resize_linear(img, dst_h, dst_w, f):
    H, W = img.shape[:2]
    sx, a0, a1 = axis_coefficients(W, dst_w, f)
    sy, b0, b1 = axis_coefficients(H, dst_h, f)
    S = img.astype(np.int64)
    sx1 = np.minimum(sx + 1, W - 1)
    sy1 = np.minimum(sy + 1, H - 1)
    h = S[:, sx, :] * a0[None, :, None] + S[:, sx1, :] * a1[None, :, None]         # [H, dst_w, 3]
    h0 = h[sy] >> 4
    h1 = h[sy1] >> 4
    out = (((b0[:, None, None] * h0) >> 16) + ((b1[:, None, None] * h1) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_nearest(lab, dst_h, dst_w, f):
    H, W = lab.shape
    lx = np.minimum(np.floor(np.arange(dst_w, dtype=np.float64) / f), W - 1).astype(np.int64)
    ly = np.minimum(np.floor(np.arange(dst_h, dtype=np.float64) / f), H - 1).astype(np.int64)
    return lab[ly][:, lx]


def brightness(img, shift):
    img = img.astype(F32)
    img[:, :, :] += shift
    img = np.around(img)
    return np.clip(img, 0, 255).astype(np.uint8)


def contrast(img, alpha):
    img = img.astype(F32)
    img = img * alpha
    img = np.around(img)
    return np.clip(img, 0, 255).astype(np.uint8)


def hsv_round_trip(img, sat_alpha, hue_delta):
    """BGR uint8 -> HSV -> (saturation, hue) -> BGR uint8, every statement one float32 operation."""
    b = img[:, :, 0].astype(F32)
    g = img[:, :, 1].astype(F32)
    r = img[:, :, 2].astype(F32)
    V = np.maximum(np.maximum(r, g), b)
    m = np.minimum(np.minimum(r, g), b)
    d = V - m
    with np.errstate(divide="ignore", invalid="ignore"):
        n = F32(255) * d
        q = n / V
        S = np.where(V != 0, np.rint(q), F32(0)).astype(F32)
        nr = F32(30) * (g - b)
        ng = F32(30) * (b - r)
        nb = F32(30) * (r - g)
        hr = nr / d
        qg = ng / d
        hg = F32(60) + qg
        qb = nb / d
        hb = F32(120) + qb
    H = np.where(V == r, hr, np.where(V == g, hg, hb)).astype(F32)
    H = np.where(d == 0, F32(0), H).astype(F32)
    H = np.where(H < 0, H + F32(180), H).astype(F32)
    H = np.rint(H)
    H = np.where(H == 180, F32(0), H).astype(F32)
    if sat_alpha is not None:
        t = S * F32(sat_alpha)
        S = np.clip(np.rint(t), 0, 255).astype(F32)
    if hue_delta is not None:
        H = H + F32(hue_delta)
        H = np.where(H < 0, H + F32(180), H).astype(F32)
        H = np.where(H >= 180, H - F32(180), H).astype(F32)
    assert S.dtype == F32 and H.dtype == F32 and V.dtype == F32
    s = S / F32(255)
    h6 = H / F32(30)
    fi = np.floor(h6)
    f = h6 - fi
    oms = F32(1) - s
    p = V * oms
    sf = s * f
    omsf = F32(1) - sf
    q = V * omsf
    omf = F32(1) - f
    st = s * omf
    omst = F32(1) - st
    t = V * omst
    i = fi.astype(np.int64)
    assert i.min() >= 0 and i.max() <= 5
    R = np.choose(i, [V, q, p, p, t, V])
    G = np.choose(i, [t, V, V, q, p, p])
    B = np.choose(i, [p, p, t, V, V, q])
    assert R.dtype == F32
    out = np.stack([B, G, R], axis=2)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def input_transform(image, mean=MEAN, std=STD):
    image = image.astype(np.float32)[:, :, ::-1]
    image = image / 255.0
    image -= mean
    image /= std
    return image


def augment(img, lab, p, crop, id_table=None, ignore_label=255, mean=MEAN, std=STD):
    """img uint8 [H,W,3] BGR, lab uint8 [H,W] raw ids or None, p AugParams, crop (h, w)
    -> (float32 [3,ch,cw], int64 [ch,cw] or None, int64 [256] histogram or None)"""
    ch, cw = crop
    if lab is not None and id_table is not None:
        lab = id_table[lab]
    img = resize_linear(img, p.dst_h, p.dst_w, p.f_scale)              # (f = 1 is the identity by the formula itself)
    if lab is not None:
        lab = resize_nearest(lab, p.dst_h, p.dst_w, p.f_scale)
    if p.shift is not None:
        img = brightness(img, p.shift)
    if p.mode == 1 and p.contrast is not None:
        img = contrast(img, p.contrast)
    if p.saturation is not None or p.hue is not None:
        img = hsv_round_trip(img, p.saturation, p.hue)
    if p.mode == 0 and p.contrast is not None:
        img = contrast(img, p.contrast)
    image = input_transform(img, mean, std)
    H, W = image.shape[:2]
    Hp, Wp = max(H, ch), max(W, cw)
    pad = np.zeros((Hp, Wp, 3), dtype=np.float32)
    pad[:H, :W] = image
    image = pad[p.h_off:p.h_off + ch, p.w_off:p.w_off + cw].transpose(2, 0, 1)
    if p.flip:
        image = image[:, :, ::-1]
    image = np.ascontiguousarray(image)
    assert image.dtype == np.float32 and image.shape == (3, ch, cw)
    if lab is None:
        return image, None, None
    lpad = np.full((Hp, Wp), ignore_label, dtype=np.int64)
    lpad[:H, :W] = lab
    label = lpad[p.h_off:p.h_off + ch, p.w_off:p.w_off + cw]
    if p.flip:
        label = label[:, ::-1]
    label = np.ascontiguousarray(label)
    return image, label, np.bincount(label.reshape(-1), minlength=256)


def balance_weight(label, num_classes, balance, ignore_label=255, target_class=None, beta=0.9999):
    """get_label (Base.py:73-89) in float64."""
    label_balance = label.copy()
    label_balance[label == ignore_label] = num_classes
    class_num = np.bincount(label_balance.reshape(-1), minlength=num_classes + 1)[:-1]
    if balance == 1:
        weight_class = 1 / (class_num + 1)
    else:
        weight_class = (1 + 1e-8 - beta ** class_num[target_class]) / (1 + 1e-8 - beta ** class_num)
    weight_class = np.clip(weight_class, 0.0, 1.0)
    weight_class = np.append(weight_class, 0)
    return weight_class[label_balance]
