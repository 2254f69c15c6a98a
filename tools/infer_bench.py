#!/usr/bin/env python
"""Inference FPS of predict_whole-style evaluation (evaluate.py:314-337,365-368 prints the same
figure): DeepLabv3-R101 (or --model simple / deeplabv3p / psp), one 1024x2048 image per call, eval-mode BN folded into the convs,
fused upsample+argmax.  5 warm-up calls like the reference, then timed calls."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from dcfp_amd import evaluate as ev, networks  # noqa: E402

_NAMES = {"simple": "simple", "deeplabv3": "DeepLabv3", "deeplabv3p": "DeepLabv3+", "psp": "PSPNet"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="deeplabv3", choices=("simple", "deeplabv3", "deeplabv3p", "psp"))
    ap.add_argument("--backbone", default="resnet101")
    ap.add_argument("--size", default="1024,2048")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--fp16", action="store_true", help="time predict_labels through the frozen fp16 engine (dcfp_amd/deploy.py)")
    ap.add_argument("--channel-cfg", default=None, help="slim the model with this channel_cfg.pth (pruners.init_pruned_model)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h, w = [int(v) for v in a.size.split(",")]
    bb = {"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128, "pretrained": False}
    m = getattr(networks, a.model).Seg_Model(backbone=a.backbone, backbone_para=bb, num_classes=19, align_corner=True,
                                             deepsup=False)
    if a.channel_cfg:
        from dcfp_amd.pruners import init_pruned_model
        init_pruned_model(m, torch.load(a.channel_cfg, weights_only=False))
    m = m.to(dev).eval()
    if a.fp16:
        from dcfp_amd import deploy
        m = deploy.build_engine(m.cpu()).to(dev)
    x = torch.randn(a.batch, 3, h, w, device=dev)
    for _ in range(5):
        ev.predict_labels(m, x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        ev.predict_labels(m, x)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"inference: {a.batch * a.iters / dt:.2f} images/s ({dt / a.iters * 1e3:.1f} ms per batch of {a.batch}) "
          f"{_NAMES[a.model]}-{a.backbone}{' slim' if a.channel_cfg else ''} {h}x{w} " + ("fp16 engine" if a.fp16 else "fp32") + (" (conv math: bf16x3 split)" if os.environ.get("DCFP_CONV_MATH") == "bf16x3" else ""))


if __name__ == "__main__":
    main()
