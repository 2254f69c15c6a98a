#!/usr/bin/env python
"""Interleaved A/B of the sliding-window evaluation of one batch, in one process, by device events:

  A  evaluate.predict_multiscale(whole=False) + ops.upsample_argmax      (one network call per tile, N x C x hs x ws tensors)
  B  evaluate.predict_sliding_vote                                       (batched tiles, one vote launch)

DeepLabv3-R101 in fp32 (`--precision fp32`) or through its fp16 engine (`--precision fp16`) at 1024 x 2048 with
769 x 769 tiles, batch 1 and 4, one scale without flip (`--ms 1 --flip False`) or scales 0.5 .. 1.75 + flip.  Per batch
size: median and minimum of `--rounds` rounds after `--warmup`; the network alone on one tile x N images and on a
batch of tiles as path B stacks them, per tile; the vote launch alone on seeded logits of the same geometry (no
network); torch.cuda.max_memory_allocated of each path.  Prints one JSON line per batch size."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dcfp_amd import deploy, evaluate as ev, networks, ops  # noqa: E402


def str2bool(v):
    return v.lower() in ("yes", "true", "t", "y", "1")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def stats(v):
    return {"median": statistics.median(v), "min": min(v)}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=str, default="1024,2048")
    p.add_argument("--tile", type=str, default="769,769")
    p.add_argument("--batches", type=str, default="1,4")
    p.add_argument("--ms", type=str, default="0.5,0.75,1,1.25,1.5,1.75")
    p.add_argument("--flip", type=str2bool, default="True")
    p.add_argument("--precision", type=str, default="fp16", choices=("fp32", "fp16"))
    p.add_argument("--backbone", type=str, default="resnet101")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--num-classes", type=int, default=19)
    args = p.parse_args(argv)
    H, W = map(int, args.size.split(","))
    tile = tuple(map(int, args.tile.split(",")))
    scales = [float(s) for s in args.ms.split(",")]
    C = args.num_classes
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = networks.deeplabv3.Seg_Model(backbone=args.backbone, backbone_para={"pretrained": False}, num_classes=C,
                                         align_corner=True, criterion=None, deepsup=False).eval()
    net = deploy.build_engine(model).to(dev) if args.precision == "fp16" else model.to(dev)
    for n in [int(b) for b in args.batches.split(",")]:
        image = torch.randn(n, 3, H, W, device=dev)
        tile_batch = max(1, ev.TILE_PIXELS_PER_CALL // (n * tile[0] * tile[1]))
        geometry = [((int(H * s), int(W * s)),) + ev.sliding_tiles(int(H * s), int(W * s), tile) for s in scales]
        tiles_per_pass = [len(ys) * len(xs) for _, ys, xs in geometry]
        tile_batch = min(tile_batch, max(tiles_per_pass))
        out = {}

        def path_a():
            full = ev.predict_multiscale(net, image, tile, scales, C, args.flip, True, False)
            out["a"] = ops.upsample_argmax(full, (H, W), True)

        def path_b():
            out["b"] = ev.predict_sliding_vote(net, image, tile, scales, args.flip, True)[0]

        with torch.no_grad():
            for _ in range(args.warmup):
                path_a()
                path_b()
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(timed(path_a))
                tb.append(timed(path_b))
            agree = float((out["a"] == out["b"]).float().mean())
            out.clear()
            one = torch.randn(n, 3, tile[0], tile[1], device=dev)
            many = torch.randn(tile_batch * n, 3, tile[0], tile[1], device=dev)
            net.lowres_logits(one), net.lowres_logits(many)
            t_one = [timed(lambda: net.lowres_logits(one)) for _ in range(args.rounds)]
            t_many = [timed(lambda: net.lowres_logits(many)) / tile_batch for _ in range(args.rounds)]
            del one, many
            # the vote launch alone: seeded logits of the same geometry, no network
            lh, lw = (tile[0] - 1) // 8 + 1, (tile[1] - 1) // 8 + 1
            weight = (0.5 if args.flip else 1.0) / len(scales)
            passes = []
            for (hw, ys, xs) in geometry:
                for mirrored in ((False, True) if args.flip else (False,)):
                    passes.append((torch.randn(len(ys) * len(xs), n, C, lh, lw, device=dev), hw, tile, ys, xs, mirrored,
                                   weight))
            ops.sliding_vote(passes, (H, W), (H, W), True)
            tv = [timed(lambda: ops.sliding_vote(passes, (H, W), (H, W), True)) for _ in range(args.rounds)]
            del passes
            mem_a, mem_b = peak(path_a), peak(path_b)
            out.clear()
        print(json.dumps({"precision": args.precision, "backbone": args.backbone, "batch": n, "size": [H, W],
                          "tile": list(tile), "scales": scales, "flip": bool(args.flip), "rounds": args.rounds,
                          "tiles_per_pass": tiles_per_pass, "tile_batch": tile_batch,
                          "A_chain_ms": stats(ta), "B_fused_ms": stats(tb),
                          "net_ms_per_tile_single_call": stats(t_one), "net_ms_per_tile_batched": stats(t_many),
                          "vote_launch_ms": stats(tv), "A_peak_MiB": mem_a, "B_peak_MiB": mem_b,
                          "pred_agreement": agree}), flush=True)


if __name__ == "__main__":
    main()
