"""The multi-scale + flip sliding-window vote of the reference (evaluate.py:145-227, whole=False) as the project pins it:
oracle.evalmetrics.predict_multiscale(..., whole=False) on the CPU, driven by a stub network that ignores the pixels and
hands out prepared low-resolution logits, upsampled to the tile size as a model's forward does.

A `pass` is (scale, logits [T,N,C,lh,lw], logits of the mirrored image's tiles or None); the stub is called per scale
for the plain pass's tiles row-major, then for the mirrored pass's.  `chain(..., torch.float64)` is the truth,
`chain(..., torch.float32)` the reference's own arithmetic; `tolerance` is what a test may allow the kernel (the rule of
tests/_vote_common.py)."""
from math import ceil

import torch
import torch.nn.functional as F

from _vote_common import tolerance_of
from oracle import evalmetrics

SIX_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def reference_tiles(h, w, tile):
    """The loop of evaluate.py:145-184, literally -> [(y1, y2, x1, x2)] in call order, rows, cols."""
    overlap = 1 / 3
    stride = ceil(tile[0] * (1 - overlap))
    tile_rows = int(ceil((h - tile[0]) / stride) + 1)
    tile_cols = int(ceil((w - tile[1]) / stride) + 1)
    boxes = []
    for row in range(tile_rows):
        for col in range(tile_cols):
            x1, y1 = int(col * stride), int(row * stride)
            x2 = min(x1 + tile[1], w)
            y2 = min(y1 + tile[0], h)
            x1 = max(int(x2 - tile[1]), 0)
            y1 = max(int(y2 - tile[0]), 0)
            boxes.append((y1, y2, x1, x2))
    return boxes, tile_rows, tile_cols


def lowres_size(th, tw):
    """Size of an output-stride-8 network's logits for a th x tw tile."""
    return (th - 1) // 8 + 1, (tw - 1) // 8 + 1


def make_passes(seed, N, C, grid_hw, tile, scales, flip, sigma=3.0):
    """Seeded N(0, sigma^2) logits per tile and image for every (scale, flip) pass of a grid."""
    g = torch.Generator().manual_seed(seed)
    lh, lw = lowres_size(*tile)
    passes = []
    for s in scales:
        T = len(reference_tiles(int(grid_hw[0] * s), int(grid_hw[1] * s), tile)[0])
        a = torch.randn(T, N, C, lh, lw, generator=g) * sigma
        b = torch.randn(T, N, C, lh, lw, generator=g) * sigma if flip else None
        passes.append((float(s), a, b))
    return passes


class _Stub:
    """On its k-th call the k-th prepared logits, resized to the tile as a model's forward resizes them."""

    def __init__(self, queue, tile, align_corners, dtype):
        self.queue, self.tile, self.align, self.dtype, self.calls = queue, tuple(tile), align_corners, dtype, 0

    def __call__(self, image):
        assert tuple(image.shape[2:]) == self.tile
        low = self.queue[self.calls]
        self.calls += 1
        return [F.interpolate(low.to(self.dtype), self.tile, mode="bilinear", align_corners=self.align)]


def chain(passes, grid_hw, out_hw, tile, align_corners, dtype):
    queue = []
    for _, a, b in passes:
        queue += list(a)
        if b is not None:
            queue += list(b)
    N, C = passes[0][1].shape[1:3]
    flip = passes[0][2] is not None
    stub = _Stub(queue, tile, align_corners, dtype)
    image = torch.zeros((N, 3) + tuple(grid_hw), dtype=dtype)
    full = evalmetrics.predict_multiscale(stub, image, tuple(tile), [s for s, _, _ in passes], C, flip, align_corners,
                                          whole=False)
    assert stub.calls == len(queue) and full.dtype == dtype
    return full[:, :, :out_hw[0], :out_hw[1]]


def to_passes(passes, grid_hw, tile, device):
    """The passes as ops.sliding_vote takes them."""
    from dcfp_amd import evaluate as ev
    out = []
    for s, a, b in passes:
        hs, ws = int(grid_hw[0] * s), int(grid_hw[1] * s)
        ys, xs = ev.sliding_tiles(hs, ws, tile)
        weight = (0.5 if b is not None else 1.0) / len(passes)
        out.append((a.to(device), (hs, ws), tuple(tile), ys, xs, False, weight))
        if b is not None:
            out.append((b.to(device), (hs, ws), tuple(tile), ys, xs, True, weight))
    return out


def tolerance(passes, grid_hw, out_hw, tile, align_corners):
    """-> (truth fp64, tol, e_ref, M) by the rule of _vote_common.tolerance_of."""
    return tolerance_of(chain(passes, grid_hw, out_hw, tile, align_corners, torch.float64),
                        chain(passes, grid_hw, out_hw, tile, align_corners, torch.float32),
                        [t for _, a, b in passes for t in (a, b)])
