#!/usr/bin/env python
"""Times ops.label_boundary at N 4, 1024x2048, d = 46, 19 classes on the evaluation driver's seeded
rectangle labels, int32 and int64: device events around --iters launches after a warm-up.  Prints one JSON line per
dtype: microseconds per call, the algorithmic bytes (labels read once + output written once) over that time as a share
of the copy rate DESIGN §11 uses as the memory bound, and the workspace traffic of the two passes, listed apart.
--host also times a numpy restatement of the transform for ONE 1024x2048 map on the host (context only)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from dcfp_amd import ops  # noqa: E402
from dcfp_amd.utils.edge_utils import boundary_dilation  # noqa: E402
from evaluate import SyntheticSegDataset  # noqa: E402  (tools/evaluate.py)

COPY_RATE = 6.29e12      # B/s, read + write counted: the device copy rate of DESIGN §11
BAND = 32                # rows per column-pass wave (csrc/boundary.hip)


def host_restatement(lab, C, d, background):
    """out = label where valid and the (2d+1)^2 window is not uniformly that label: per class present, a minimum
    filter over the one-hot mask as two separable passes of running sums (numpy, one thread)."""
    import numpy as np
    h, w = lab.shape
    out = np.full_like(lab, background)
    for c in np.unique(lab):
        if not 0 <= c < C:
            continue
        m = np.zeros((h + 2 * d + 1, w + 2 * d + 1), dtype=np.int64)
        m[d + 1:d + 1 + h, d + 1:d + 1 + w] = lab == c
        s = m.cumsum(0).cumsum(1)
        k = 2 * d + 1
        win = s[k:, k:] - s[:-k, k:] - s[k:, :-k] + s[:-k, :-k]
        out[(lab == c) & (win != k * k)] = c
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=str, default="1024,2048")
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    h, w = map(int, a.size.split(","))
    d = boundary_dilation(h, w)
    dev = torch.device("cuda:0")
    lab64 = SyntheticSegDataset(a.classes, 255, (h, w), 12345).labels(a.batch)
    pixels = a.batch * h * w
    for dtype in (torch.int32, torch.int64):
        x = lab64.to(dtype).to(dev)
        for _ in range(a.warmup):
            out = ops.label_boundary(x, a.classes, d)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            out = ops.label_boundary(x, a.classes, d)
        e.record()
        torch.cuda.synchronize()
        us = s.elapsed_time(e) * 1e3 / a.iters
        esz = x.element_size()
        algorithmic = 2 * esz * pixels
        warm = sum(min(d, y0) + min(d, h - min(y0 + BAND, h)) for y0 in range(0, h, BAND)) / h
        extra = {"row_pass_key_bytes_written": 2 * pixels, "row_pass_key_bytes_reread": pixels,
                 "col_pass_key_bytes_read": int(pixels * (2 + warm)), "col_pass_label_bytes_reread": esz * pixels}
        print(json.dumps({"op": "label_boundary", "dtype": str(dtype), "shape": [a.batch, h, w], "d": d,
                          "boundary_share": float((out != 255).float().mean()), "iters": a.iters,
                          "us_per_call": round(us, 2), "algorithmic_bytes": algorithmic,
                          "algorithmic_TBps": round(algorithmic / us / 1e6, 3),
                          "share_of_copy_rate": round(algorithmic / (us * 1e-6) / COPY_RATE, 3),
                          "workspace_traffic_bytes": extra}), flush=True)
    if a.host:
        import numpy as np
        one = lab64[0].numpy()
        t0 = time.perf_counter()
        ref = host_restatement(one, a.classes, d, 255)
        dt = time.perf_counter() - t0
        same = bool(np.array_equal(ref, ops.label_boundary(lab64[:1].to(dev), a.classes, d)[0].cpu().numpy()))
        print(json.dumps({"op": "host numpy restatement (not the reference's OpenCV path)", "shape": [h, w], "d": d,
                          "seconds": round(dt, 3), "equals_device": same}), flush=True)


if __name__ == "__main__":
    main()
