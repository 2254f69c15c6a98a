"""The multi-scale + flip vote of the reference (evaluate.py:198-227, whole=True) as it stands there, written with
F.interpolate on the CPU from the network's low-resolution logits on: resize up to the size the network saw,
0.5 * (plain + flip(mirrored)), resize to the voting grid, sum over the scales, divide by their number, crop.

A `pass` is ((hs, ws), logits [N,C,h,w], logits of the mirrored image or None).  `chain(..., torch.float64)` is the
truth, `chain(..., torch.float32)` the reference's own arithmetic; `tolerance` is what a test may allow the kernel."""
import torch
import torch.nn.functional as F

from _vote_common import tolerance_of

SIX_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def lowres_size(hs, ws):
    """Size of an output-stride-8 network's logits for an hs x ws input."""
    return (hs - 1) // 8 + 1, (ws - 1) // 8 + 1


def make_passes(seed, N, C, grid_hw, scales, flip, sigma=3.0):
    """Seeded N(0, sigma^2) logits for every (scale, flip) pass of a grid."""
    g = torch.Generator().manual_seed(seed)
    passes = []
    for s in scales:
        hs, ws = int(grid_hw[0] * s), int(grid_hw[1] * s)
        h, w = lowres_size(hs, ws)
        a = torch.randn(N, C, h, w, generator=g) * sigma
        b = torch.randn(N, C, h, w, generator=g) * sigma if flip else None
        passes.append(((hs, ws), a, b))
    return passes


def chain(passes, grid_hw, out_hw, align_corners, dtype):
    full = None
    for (hs, ws), a, b in passes:
        probs = F.interpolate(a.to(dtype), size=(hs, ws), mode="bilinear", align_corners=align_corners)
        if b is not None:
            flipped = F.interpolate(b.to(dtype), size=(hs, ws), mode="bilinear", align_corners=align_corners)
            probs = 0.5 * (probs + torch.flip(flipped, [3]))
        probs = F.interpolate(probs, size=tuple(grid_hw), mode="bilinear", align_corners=align_corners)
        full = probs if full is None else full + probs
    full = full / len(passes)
    return full[:, :, :out_hw[0], :out_hw[1]]


def to_maps(passes, device):
    """The passes as ops.multiscale_vote takes them."""
    maps = []
    for (hs, ws), a, b in passes:
        weight = (0.5 if b is not None else 1.0) / len(passes)
        maps.append((a.to(device), (hs, ws), False, weight))
        if b is not None:
            maps.append((b.to(device), (hs, ws), True, weight))
    return maps


def tolerance(passes, grid_hw, out_hw, align_corners):
    """-> (truth fp64, tol, e_ref, M) by the rule of _vote_common.tolerance_of."""
    return tolerance_of(chain(passes, grid_hw, out_hw, align_corners, torch.float64),
                        chain(passes, grid_hw, out_hw, align_corners, torch.float32),
                        [t for _, a, b in passes for t in (a, b)])
