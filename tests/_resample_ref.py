"""numpy-only restatement of the `resample` sampler's contract: the class mask on the scaled, padded label
grid, its 8-connected components numbered by first pixel, the k-th pixel of a component, the epoch index and the crop
draws.  Written from the contract, slow and plain; the tests hold the product to it bit for bit."""
import random

import numpy as np


def nearest_map(src_n, dst_n, f):
    """Source row / column of every destination row / column of the label resize: min(floor(d / f), src_n - 1)."""
    return np.minimum(np.floor(np.arange(dst_n, dtype=np.float64) / f), src_n - 1).astype(np.int32)


def class_mask(raw, id_table, row_map, col_map, grid_hw, cls):
    """bool [Hp,Wp]: id_table[raw[row_map[y], col_map[x]]] == cls inside len(row_map) x len(col_map), False in the padding."""
    mask = np.zeros(grid_hw, dtype=bool)
    table = np.arange(256, dtype=np.uint8) if id_table is None else np.asarray(id_table, dtype=np.uint8)
    scaled = table[raw[np.asarray(row_map)[:, None], np.asarray(col_map)[None, :]]]
    mask[:len(row_map), :len(col_map)] = scaled == cls
    return mask


def label_components(mask):
    """-> (int32 [H,W] label map: smallest linear index of the pixel's 8-connected component, -1 background;
    ascending component labels; their pixel counts).  Union-find over row runs, the smaller run id on top: run ids
    rise in raster order, so the top run of a set holds the set's first pixel."""
    H, W = mask.shape
    parent, start, rows = [], [], []

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    prev = []
    for y in range(H):
        d = np.diff(np.concatenate(([0], mask[y].astype(np.int8), [0])))
        cur, j = [], 0
        for s, e in zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()):       # run [s, e)
            rid = len(parent)
            parent.append(rid)
            start.append(y * W + s)
            rows.append((y, s, e))
            cur.append((s, e, rid))
            while j < len(prev) and prev[j][1] < s:           # runs of the row above that end left of column s - 1
                j += 1
            jj = j
            while jj < len(prev) and prev[jj][0] <= e:        # [ps, pe) touches [s - 1, e + 1)
                a, b = find(rid), find(prev[jj][2])
                if a != b:
                    parent[max(a, b)] = min(a, b)
                jj += 1
        prev = cur
    lab = np.full((H, W), -1, dtype=np.int32)
    for rid, (y, s, e) in enumerate(rows):
        lab[y, s:e] = start[find(rid)]
    roots, sizes = np.unique(lab[lab >= 0], return_counts=True)
    return lab, roots.astype(np.int32), sizes.astype(np.int32)


def kth_pixel(label_map, root, k):
    """(y, x) of the k-th pixel, in linear-index order, of the component labelled `root`."""
    p = int(np.flatnonzero(label_map.reshape(-1) == root)[k])
    return p // label_map.shape[1], p % label_map.shape[1]


def renumber_by_first_pixel(comp):
    """A labelling with arbitrary positive component numbers (0 background) -> the label map of the contract."""
    flat = comp.reshape(-1)
    out = np.full(flat.shape, -1, dtype=np.int32)
    ids, first = np.unique(flat, return_index=True)
    for i, p in zip(ids, first):
        if i > 0:
            out[flat == i] = p
    return out.reshape(comp.shape)


def index_seed(seed, epoch):
    return int(seed) * 1000003 + int(epoch)


def gen_index(list_lengths, seed, epoch):
    """The epoch index from the per-class list lengths -> (file_index, class_index)."""
    rng = random.Random(index_seed(seed, epoch))
    length = int(max(list_lengths))
    file_index, class_index = [], []
    for c, n in enumerate(list_lengths):
        file_index += list(range(n)) * (length // n) + rng.sample(list(range(n)), length % n)
        class_index += [c] * length
    return file_index, class_index


def crop_draws(rng, grid_hw, crop_hw, mirror, label_map=None, roots=None):
    """The crop and mirror draws on a labelled grid -> (h_off, w_off, flip, chosen pixel or None).  `roots` empty or
    None: the plain draws."""
    (Hp, Wp), (ch, cw) = grid_hw, crop_hw
    pixel = None
    if roots is not None and len(roots) >= 1:                       # nums = len(roots) + 1 >= 2
        n = rng.randint(1, len(roots))
        size = int((label_map == roots[n - 1]).sum())
        k = rng.randint(0, size - 1)
        pixel = kth_pixel(label_map, roots[n - 1], k)
        h_off = pixel[0] - ch // 2 - rng.randint(-(ch // 4), ch // 4)
        w_off = pixel[1] - cw // 2 - rng.randint(-(cw // 4), cw // 4)
    else:
        h_off = rng.randint(0, Hp - ch)
        w_off = rng.randint(0, Wp - cw)
    h_off = min(max(h_off, 0), Hp - ch)
    w_off = min(max(w_off, 0), Wp - cw)
    flip = False
    if mirror:
        flip = rng.randint(0, 1) * 2 - 1 < 0
    return h_off, w_off, flip, pixel


# ---- the masks of tests/test_components_gpu.py (shared with the scipy cross-check of the host tests)
def serpentine(H, W):
    """A one-pixel-wide path: every second row in full, joined alternately at its right and left end."""
    m = np.zeros((H, W), dtype=bool)
    m[0::2] = True
    for i, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = True
    return m


def spiral(H, W):
    """A one-pixel-wide rectangular spiral with a one-pixel gap between its turns."""
    m = np.zeros((H, W), dtype=bool)
    top, left, bottom, right = 0, 0, H - 1, W - 1
    while top <= bottom and left <= right:
        m[top, left:right + 1] = True
        m[top:bottom + 1, right] = True
        if bottom - top >= 2:
            m[bottom, left + 2 if left else left:right + 1] = True
        if right - left >= 2 and bottom - top >= 2:
            m[top + 2:bottom + 1, left + 2 if left else left] = True
        top, left, bottom, right = top + 2, left + 2 if left else 2, bottom - 2, right - 2
        if top <= bottom and left <= right:
            m[top, left - 2:left + 1] = True      # the step inwards
    return m


def pattern_masks(T):
    """name -> bool mask; T is the tile edge of the device's tile pass."""
    rng = np.random.RandomState(20240613)
    grids = {"1x1": (1, 1), "row": (1, 2 * T + 3), "col": (2 * T + 3, 1), "tile": (T, T),
             "odd": (T + 1, 2 * T - 1), "big": (300, 520)}
    out = {}
    for g, (H, W) in grids.items():
        out["empty_" + g] = np.zeros((H, W), dtype=bool)
        out["full_" + g] = np.ones((H, W), dtype=bool)
        out["checker_" + g] = (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0
        out["random40_" + g] = rng.rand(H, W) < 0.4
    for name, boxes in (("diag", ((T - 8, T - 8), (T, T))), ("anti", ((T - 8, T), (T, T - 8))),
                        ("apart", ((T - 9, T - 9), (T, T)))):
        m = np.zeros((2 * T, 2 * T), dtype=bool)
        for y, x in boxes:
            m[y:y + 8, x:x + 8] = True
        out["corner_" + name] = m
    out["serpentine"] = serpentine(4 * T, 4 * T)
    out["spiral"] = spiral(2 * T + 7, 3 * T + 2)
    iso = np.zeros((2 * T + 3, 2 * T + 1), dtype=bool)
    iso[0::2, 0::2] = True
    out["isolated"] = iso
    for d in (10, 40, 60, 90):
        out["random%d" % d] = rng.rand(T + 70, 2 * T + 45) < d / 100.0
    return out
