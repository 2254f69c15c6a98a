#!/usr/bin/env python
"""Times the crop location of the `resample` sampler: ops.label_components and ops.component_pixel for
batches of 4 and 8 synthetic 1024x2048 label maps at f = 2.0 and f = 1.0 (crop 769x769), on two kinds of class mask -
a few large blobs, and a thin-structure class of a few thousand small components - with device events (median of
--iters), next to the two host round trips of a batch (counts, then sizes; the pixels) and to the bytes the labelling
must move at the least: per sample the source label bytes, 8 bytes per grid pixel written by the tile pass and 4 read
by each of the flatten and compact passes (16 * Hp * Wp + H * W); component_pixel reads 4 * Hp * Wp.
Where scipy imports, scipy.ndimage.label with a 3x3 structure labels the same masks on one host thread beside it."""
import argparse
import json
import os.path as osp
import sys
import time

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def blob_labels(rs, H, W):
    """Class 1 in about a quarter of the 128x128 blocks of a coarse grid: a few large components."""
    coarse = (rs.rand(H // 128, W // 128) < 0.25).astype(np.uint8)
    return np.ascontiguousarray(np.kron(coarse, np.ones((128, 128), dtype=np.uint8)))


def thin_labels(rs, H, W, n=3000):
    """Class 1 in n short bars 2 pixels wide (poles, signs): a few thousand small components."""
    lab = np.zeros((H, W), dtype=np.uint8)
    for y, x, h in zip(rs.randint(0, H - 40, n), rs.randint(0, W - 2, n), rs.randint(5, 40, n)):
        lab[y:y + h, x:x + 2] = 1
    return lab


def median_ms(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", type=str, default="1024,2048")
    ap.add_argument("--crop", type=str, default="769,769")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    import torch
    from dcfp_amd import ops
    from dcfp_amd.datasets import base
    H, W = map(int, args.source.split(","))
    ch, cw = map(int, args.crop.split(","))
    dev = torch.device("cuda:0")
    ndimage = None
    if not args.no_scipy:
        try:
            from scipy import ndimage
        except ImportError:
            pass
    for kind, make in (("blobs", blob_labels), ("thin", thin_labels)):
        for f in (2.0, 1.0):
            for batch in (4, 8):
                rs = np.random.RandomState(batch)
                raws = [make(rs, H, W) for _ in range(batch)]
                dh, dw = int(round(H * f)), int(round(W * f))
                Hp, Wp = max(dh, ch), max(dw, cw)
                rm, cm = base.resize_taps(H, dh, f)[:, 3], base.resize_taps(W, dw, f)[:, 3]
                maps = torch.from_numpy(np.concatenate([rm, cm] * batch)).to(dev)
                recs = [(dh, dw, Hp, Wp, i * (dh + dw), i * (dh + dw) + dh, 1) for i in range(batch)]
                labels = [torch.from_numpy(r).to(dev) for r in raws]
                rec = {"mask": kind, "scale": f, "batch": batch, "grid": [Hp, Wp]}
                box = {}

                def label():
                    box["comp"] = ops.label_components(labels, recs, maps, None, 255)
                ms, ms_min = median_ms(label, args.iters)
                moved = batch * (16 * Hp * Wp + H * W)
                comp = box["comp"]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                counts = comp.counts()
                n = [max(1, c // 2) if c else 0 for c in counts]
                sizes = comp.sizes(n)
                t1 = time.perf_counter()
                k = [s // 2 for s in sizes]
                pms, pms_min = median_ms(lambda: ops.component_pixel(comp, n, k), args.iters)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                ops.component_pixel(comp, n, k).tolist()
                t3 = time.perf_counter()
                rec.update(components=counts, label_components_ms=round(ms, 4), label_components_ms_min=round(ms_min, 4),
                           label_bytes_min=int(moved), label_gb_per_s=round(moved / ms / 1e6, 1),
                           component_pixel_ms=round(pms, 4), component_pixel_ms_min=round(pms_min, 4),
                           pixel_bytes_min=int(batch * 4 * Hp * Wp),
                           counts_and_sizes_round_trip_ms=round((t1 - t0) * 1e3, 4),
                           pixel_call_and_round_trip_ms=round((t3 - t2) * 1e3, 4))
                if ndimage is not None:
                    times = []
                    for raw in raws[:2]:
                        mask = np.zeros((Hp, Wp), dtype=bool)
                        mask[:dh, :dw] = raw[rm[:, None], cm[None, :]] == 1
                        t = time.perf_counter()
                        _, c = ndimage.label(mask, np.ones((3, 3)))
                        times.append(time.perf_counter() - t)
                    rec["scipy_label_one_thread_ms_per_sample"] = round(float(np.median(times)) * 1e3, 2)
                print(json.dumps(rec), flush=True)
                del comp, box


if __name__ == "__main__":
    main()
