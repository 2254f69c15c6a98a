"""What the boundary tests share (tests/test_boundary_host_cpu.py, tests/test_boundary_gpu.py): a brute-force numpy
restatement of the label-boundary transform, written from its definition and never importing the product, and the
closed-form inputs of the GPU cases.  A plain helper module like tests/_parity.py: no fixtures, no tests.

Definition: a pixel is valid if 0 <= L < C.  Per class c, mask = (L == c) gets a ring of one zero pixel, is eroded d
times by 3x3 ones, and the boundary of c is mask minus eroded mask.  out = c on the boundary of c, background
everywhere else (invalid pixels belong to no mask, so they erode their neighbours and come out as background)."""
import functools

import numpy as np


def _erode3x3(m):
    """One erosion by 3x3 ones; outside the array counts as set (the zero ring is what erodes at the border)."""
    p = np.pad(m, 1, constant_values=True)
    h, w = m.shape
    out = np.ones_like(m)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + h, dx:dx + w]
    return out


def _reference_one(lab, C, d, background):
    out = np.full(lab.shape, background, dtype=lab.dtype)
    for c in np.unique(lab):
        if not 0 <= c < C:
            continue
        mask = lab == c
        er = np.pad(mask, 1, constant_values=False)
        for _ in range(d):
            if not er.any():
                break
            er = _erode3x3(er)
        out[mask & ~er[1:-1, 1:-1]] = c
    return out


def reference(labels, C, d, background):
    """labels: integer [H,W] or [N,H,W] numpy array -> array of the same shape and dtype."""
    labels = np.asarray(labels)
    if labels.ndim == 2:
        return _reference_one(labels, C, d, background)
    return np.stack([_reference_one(l, C, d, background) for l in labels])


def interior_mask(labels, C, d):
    """valid and not boundary, by the reference alone."""
    labels = np.asarray(labels)
    valid = (labels >= 0) & (labels < C)
    return valid & (reference(labels, C, d, -7) == -7)


def probe():
    """41x53 of class 3 with one pixel of class 5 at (20, 30); with d = 4 the boundary has 41*53 - 33*45 + 81 = 769
    pixels: the border band, plus the 9x9 window round the odd pixel, which itself is the only one labelled 5."""
    l = np.full((41, 53), 3, dtype=np.int64)
    l[20, 30] = 5
    return l


def make_map(pattern, N, H, W, C, bh, bw, dtype=np.int64):
    """The closed-form label maps of the GPU cases: blocks of bh x bw pixels, overlaid with invalid values (255, C,
    -1), a one-pixel-wide line and single odd pixels."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    maps = []
    for n in range(N):
        l = (((y // bh) * 5 + (x // bw) * 3 + n) % C).astype(np.int64)
        if pattern == "dense":
            l[H // 3 + n: H // 3 + n + max(1, H // 6), W // 4: W // 4 + max(1, W // 5)] = 255
            l[:, W // 2] = C - 1
            l[(2 * H) // 3, :] = 255 if n % 2 else C
            l[H - 1, W - 1] = -1
            l[0, 0] = (l[0, 0] + 1) % C
        else:
            assert pattern == "sparse"
            l[0:4, 0:6] = 255
            l[H - 1, W - 1] = -1
            l[H // 2 + n, W // 4] = (l[H // 2 + n, W // 4] + 1) % C
        maps.append(l)
    return np.stack(maps).astype(dtype)


# (pattern, N, H, W, C, d, bh, bw)
CASES = (
    ("dense", 3, 33, 65, 19, 2, 11, 13),
    ("dense", 3, 33, 65, 19, 5, 16, 32),
    ("dense", 2, 64, 64, 19, 3, 32, 32),
    ("dense", 2, 67, 131, 150, 4, 20, 40),
    ("dense", 2, 40, 300, 19, 7, 20, 64),
    ("dense", 2, 300, 40, 59, 7, 64, 20),
    ("sparse", 2, 200, 420, 19, 46, 200, 210),
    ("sparse", 1, 300, 200, 19, 46, 150, 200),
    ("sparse", 1, 97, 200, 19, 46, 97, 200),
)
# everything valid is boundary: the window never fits
DEGENERATE = (
    ("dense", 1, 1, 1, 1, 1, 1, 1),
    ("dense", 1, 1, 7, 3, 2, 1, 3),
    ("dense", 1, 7, 1, 3, 2, 3, 1),
    ("dense", 2, 5, 9, 19, 1, 2, 3),
    ("dense", 2, 5, 9, 19, 9, 2, 3),
    ("dense", 1, 67, 131, 171, 70, 20, 40),
    ("dense", 1, 130, 517, 19, 46, 130, 259),
)


# beyond the listed cases: rows longer than the row pass's 1024-pixel chunk, so that a run start and a run end are
# carried from chunk to chunk (three chunks; one width a multiple of 4, one not: vector and element accesses)
LONG_ROWS = (
    ("dense", 1, 40, 2300, 19, 3, 20, 800),
    ("dense", 2, 20, 2303, 19, 3, 7, 1200),
)


def case_id(case):
    return "%s-%dx%dx%d-C%d-d%d" % (case[0], case[1], case[2], case[3], case[4], case[5])


@functools.lru_cache(maxsize=None)
def case_data(case, background=255):
    """(labels int64 [N,H,W], reference output) of a case: computed once, shared by the tests, read-only."""
    pattern, N, H, W, C, d, bh, bw = case
    lab = make_map(pattern, N, H, W, C, bh, bw)
    ref = reference(lab, C, d, background)
    lab.setflags(write=False)
    ref.setflags(write=False)
    return lab, ref
