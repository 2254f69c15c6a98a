#!/usr/bin/env python
"""Interleaved A/B of the multi-scale + flip evaluation of one batch, in one process, by device events:

  A  evaluate.predict_multiscale + ops.upsample_argmax + evaluate.get_confusion_matrix   (N x C x hs x ws tensors)
  B  evaluate.predict_vote with the labels and the matrix                                 (one launch after the network)

DeepLabv3-R50 through the fp16 engine at 1025 x 2049, batch 1 and 4, scales 0.5 .. 1.75 + flip (the recipe every
finetune.sh of the reference quotes).  Per batch size: median and minimum of `--rounds` rounds after `--warmup`, the
vote launch alone on the maps of one forward, and torch.cuda.max_memory_allocated of each path.  Prints one JSON line
per batch size."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dcfp_amd import deploy, evaluate as ev, networks, ops  # noqa: E402


class _Keep:
    """The network, remembering the maps of its last passes (for the timing of the vote launch alone)."""

    def __init__(self, net):
        self.net, self.align_corner, self.seen = net, net.align_corner, []

    def lowres_logits(self, image):
        out = self.net.lowres_logits(image)
        self.seen.append(out[0])
        return out


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


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=str, default="1025,2049")
    p.add_argument("--batches", type=str, default="1,4")
    p.add_argument("--ms", type=str, default="0.5,0.75,1,1.25,1.5,1.75")
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--num-classes", type=int, default=19)
    args = p.parse_args(argv)
    H, W = map(int, args.size.split(","))
    scales = [float(s) for s in args.ms.split(",")]
    C = args.num_classes
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = networks.deeplabv3.Seg_Model(backbone="resnet50", backbone_para={"pretrained": False}, num_classes=C,
                                         align_corner=True, criterion=None, deepsup=False).eval()
    net = deploy.build_engine(model).to(dev)
    for n in [int(b) for b in args.batches.split(",")]:
        image = torch.randn(n, 3, H, W, device=dev)
        label = torch.randint(0, C, (n, H, W), device=dev)
        conf_a = torch.zeros((C, C), dtype=torch.int64, device=dev)
        conf_b = torch.zeros((C, C), dtype=torch.int64, device=dev)

        def path_a():
            out = ev.predict_multiscale(net, image, (H, W), scales, C, True, True, True)
            pred = ops.upsample_argmax(out, (H, W), True)
            ev.get_confusion_matrix(label, pred, C, 255, out=conf_a)

        def path_b(n_=net):
            ev.predict_vote(n_, image, scales, True, True, labels=label, conf=conf_b)

        with torch.no_grad():
            for _ in range(args.warmup):
                path_a()
                path_b()
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(timed(path_a))
                tb.append(timed(path_b))
            keep = _Keep(net)
            path_b(keep)
            maps, weight = [], 0.5 / len(scales)
            for i, s in enumerate(scales):
                size = (int(H * s), int(W * s))
                maps += [(keep.seen[2 * i], size, False, weight), (keep.seen[2 * i + 1], size, True, weight)]
            tv = [timed(lambda: ops.multiscale_vote(maps, (H, W), (H, W), True, labels=label, conf=conf_b))
                  for _ in range(args.rounds)]
            del keep, maps
            mem_a, mem_b = peak(path_a), peak(path_b)
        same = bool(torch.equal(conf_a.sum(), conf_b.sum() - (1 + args.rounds) * n * H * W))
        print(json.dumps({"batch": n, "size": [H, W], "scales": scales, "flip": True, "rounds": args.rounds,
                          "A_multiscale_ms": {"median": statistics.median(ta), "min": min(ta)},
                          "B_vote_ms": {"median": statistics.median(tb), "min": min(tb)},
                          "vote_launch_ms": {"median": statistics.median(tv), "min": min(tv)},
                          "A_peak_MiB": mem_a, "B_peak_MiB": mem_b, "counts_agree": same}), flush=True)


if __name__ == "__main__":
    main()
