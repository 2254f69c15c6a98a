#!/usr/bin/env python
"""Times the label-PNG export of one batch: four 1024x2048 int32 predictions on the device, both PNGs of
each (paletted train ids, grey label ids), from the synchronised prediction to finished byte strings in host memory.

  path A: the maps to the host, the reverse id table on the host, PIL (zlib) - what `--device-png False` does;
  path B: evaluate.encode_label_pngs - deflated on the device, two small device-to-host copies.

Maps: `rectangles` (19 classes, 300 random rectangles per image), `noisy` (the same with 2 % of the pixels redrawn at
random) and `model` (the argmax of a randomly initialised simple-R50 on N(0,1) images; `--model-map False` skips
it).  Per map: `--warmup` untimed rounds, then the median of `--iters` rounds of each path, the two paths taking
turns; wall clock around each round with the device idle before and after, HIP events around the device part of path B
(the three launches of ops.png_deflate_labels) and of path A (the copy of the maps).  One JSON line per map."""
import argparse
import io
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dcfp_amd import evaluate as ev, networks, ops  # noqa: E402
from dcfp_amd.datasets import cs  # noqa: E402


def rectangles(rng, n, h, w, classes=19, count=300):
    maps = np.empty((n, h, w), dtype=np.int32)
    for m in maps:
        m[:] = rng.randint(0, classes)
        for _ in range(count):
            rh, rw = rng.randint(h // 32, h // 3), rng.randint(w // 32, w // 3)
            y, x = rng.randint(0, h - rh + 1), rng.randint(0, w - rw + 1)
            m[y:y + rh, x:x + rw] = rng.randint(0, classes)
    return maps


def path_a(pred, reverse, palette):
    from PIL import Image
    files = []
    for seg in pred.cpu().numpy().astype(np.uint8):
        pal, ids = io.BytesIO(), io.BytesIO()
        Image.fromarray(reverse[seg]).save(ids, format="PNG")
        im = Image.fromarray(seg)
        im.putpalette(palette)
        im.save(pal, format="PNG")
        files.append([pal.getvalue(), ids.getvalue()])
    return files


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(name, pred, luts, reverse, palette, warmup, iters):
    from PIL import Image
    fa = lambda: path_a(pred, reverse, palette)                            # noqa: E731
    fb = lambda: ev.encode_label_pngs(pred, luts, [palette, None])         # noqa: E731
    for _ in range(warmup):
        fa(), fb()
    ta, tb, da, db = [], [], [], []
    for _ in range(iters):
        ms, files_a = timed(fa)
        ta.append(ms)
        ms, files_b = timed(fb)
        tb.append(ms)
        da.append(device_ms(lambda: pred.cpu()))
        db.append(device_ms(lambda: ops.png_deflate_labels(pred, luts)))
    for a, b in zip(files_a, files_b):                                     # both paths hold the same images
        for p in range(2):
            with Image.open(io.BytesIO(a[p])) as ia, Image.open(io.BytesIO(b[p])) as ib:
                assert ia.mode == ib.mode and np.array_equal(np.asarray(ia), np.asarray(ib))
    med = lambda v: float(np.median(v))                                    # noqa: E731
    return {"map": name, "batch": list(pred.shape), "iters": iters,
            "path_a_ms": med(ta), "path_a_min_ms": min(ta), "path_a_copy_ms": med(da),
            "path_b_ms": med(tb), "path_b_min_ms": min(tb), "path_b_device_ms": med(db),
            "path_a_bytes": sum(len(f) for fs in files_a for f in fs),
            "path_b_bytes": sum(len(f) for fs in files_b for f in fs),
            "b_faster_by": 1.0 - med(tb) / med(ta)}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--size", type=str, default="1024,2048")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--model-map", type=lambda v: v.lower() in ("1", "true", "yes"), default=True)
    args = p.parse_args(argv)
    h, w = map(int, args.size.split(","))
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(args.seed)
    lst = os.devnull                                                       # an empty list: the tables need no files
    dataset = cs.DataSet("", lst, split="test")
    reverse = ev.reverse_id_table(dataset)
    palette = [int(v) for v in dataset.cmap_labels.reshape(-1)]
    luts = torch.from_numpy(np.stack([np.arange(256, dtype=np.uint8), reverse])).to(dev)
    rect = rectangles(rng, args.batch, h, w)
    noisy = rect.copy()
    redraw = rng.rand(*noisy.shape) < 0.02
    noisy[redraw] = rng.randint(0, 19, int(redraw.sum()))
    maps = [("rectangles", torch.from_numpy(rect).to(dev)), ("noisy", torch.from_numpy(noisy).to(dev))]
    if args.model_map:
        torch.manual_seed(args.seed)
        model = networks.simple.Seg_Model(backbone="resnet50", backbone_para={"pretrained": False}, num_classes=19,
                                          align_corner=True, criterion=None, deepsup=False).eval().to(dev)
        with torch.no_grad():
            pred = torch.cat([ev.predict_labels(model, torch.randn(1, 3, h, w, device=dev)) for _ in range(args.batch)])
        del model
        torch.cuda.empty_cache()
        maps.append(("model", pred.contiguous()))
    for name, pred in maps:
        print(json.dumps(measure(name, pred, luts, reverse, palette, args.warmup, args.iters)), flush=True)


if __name__ == "__main__":
    main()
