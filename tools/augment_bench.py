#!/usr/bin/env python
"""Times the device-side augmentation: one ops.augment_batch + one ops.balance_weight call for a batch of
4 sources of 1024x2048 at f = 1.3, crops 769x769 and 1024x2048, with device events, next to the bytes the call must
move (the three fp32 planes, the int64 labels, the fp32 weights and the source bytes its taps touch).
--host-reference also times the numpy restatement of the contract (tests/_augment_ref.py - NOT cv2) on the same inputs."""
import argparse
import json
import os.path as osp
import sys
import time

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--source", type=str, default="1024,2048")
    ap.add_argument("--scale", type=float, default=1.3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-reference", action="store_true")
    ap.add_argument("--host-only", action="store_true", help="time the host reference alone (needs no GPU)")
    args = ap.parse_args()
    from dcfp_amd.datasets import base
    H, W = map(int, args.source.split(","))
    rs = np.random.RandomState(0)
    sources = [(rs.randint(0, 256, (H, W, 3)).astype(np.uint8), rs.randint(0, 34, (H, W)).astype(np.uint8))
               for _ in range(args.batch)]
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    f = args.scale
    dh, dw = int(round(H * f)), int(round(W * f))
    if not args.host_only:
        import torch
        from dcfp_amd import ops
        dev = torch.device("cuda:0")
        d_images = [torch.from_numpy(im).to(dev) for im, _ in sources]
        d_labels = [torch.from_numpy(lab).to(dev) for _, lab in sources]
        id_table = torch.arange(256, dtype=torch.uint8, device=dev)
    for crop in ((769, 769), (1024, 2048)):
        params = [base.AugParams(f_scale=f, dst_h=dh, dst_w=dw, shift=5, mode=i % 2, contrast=1.1, saturation=1.2, hue=9,
                                 h_off=(dh - crop[0]) // 2, w_off=(dw - crop[1]) // 2, flip=bool(i % 2))
                  for i in range(args.batch)]
        rec = {"crop": list(crop), "batch": args.batch, "source": [H, W], "scale": f}
        if not args.host_only:
            taps, lut_a, lut_b, recs = base.pack_batch(params, [(H, W)] * args.batch, base.AugConfig(*crop), mean, std)
            src_bytes = 0
            for r in recs:
                cols, rows = taps[r[0]:r[0] + crop[1]], taps[r[1]:r[1] + crop[0]]
                nx = len(np.unique(np.concatenate([cols[:, 0], np.minimum(cols[:, 0] + 1, W - 1)])))
                ny = len(np.unique(np.concatenate([rows[:, 0], np.minimum(rows[:, 0] + 1, H - 1)])))
                src_bytes += nx * ny * 3 + len(np.unique(cols[:, 3])) * len(np.unique(rows[:, 3]))
            pix = args.batch * crop[0] * crop[1]
            moved = pix * (12 + 8 + 8 + 4) + src_bytes      # planes, labels written, labels read back, weights
            t_taps, t_a, t_b = (torch.from_numpy(x).to(dev) for x in (taps, lut_a, lut_b))

            def call():
                images, labels, hist = ops.augment_batch(d_images, d_labels, recs, t_taps, t_a, t_b, id_table, crop)
                return images, ops.balance_weight(labels, hist, 19, 1)
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            ms = float(np.median(times))
            rec.update(device_ms=round(ms, 4), device_ms_min=round(min(times), 4), bytes=int(moved),
                       source_bytes=int(src_bytes), gb_per_s=round(moved / ms / 1e6, 1))
        if args.host_reference or args.host_only:
            sys.path.insert(0, osp.join(ROOT, "tests"))
            import _augment_ref as ref
            t0 = time.perf_counter()
            for (im, lab), p in zip(sources, params):
                _, label, _ = ref.augment(im, lab, p, crop)
                ref.balance_weight(label, 19, 1)
            rec["host_numpy_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
