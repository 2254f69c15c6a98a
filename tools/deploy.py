#!/usr/bin/env python
"""Deployment driver — the command line and protocol of the reference's totrt.py (scripts/cs/trt.sh): build the
(optionally slimmed) model, freeze it into an fp16 engine (dcfp_amd/deploy.py) - or, with --precision fp8, calibrate that engine on
--calib-batches batches and build the e4m3 engine - save the engine, reload it, and time
it as totrt.benchmark does: 10 warm-up calls, 50 timed calls, each timed call synchronised; prints the average batch
time.  Without --restore-from the model keeps its initial weights (synthetic, as tools/train.py starts from)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dcfp_amd import deploy, networks  # noqa: E402
from dcfp_amd.pruners import init_pruned_model  # noqa: E402
from dcfp_amd.utils.pyt_utils import load_model  # noqa: E402


def str2bool(v):
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def get_parser():
    p = argparse.ArgumentParser(description="DCFP")
    p.add_argument("--input-size", type=str, default="1025,2049")
    p.add_argument("--batch-size", type=int, default=1)
    p.add_argument("--model", type=str, default="deeplabv3")
    p.add_argument("--backbone", type=str, default="resnet101")
    p.add_argument("--backbone-para", type=str, default='{"pretrained": false}')
    p.add_argument("--model-para", type=str, default="{}")
    p.add_argument("--align-corner", type=str2bool, default="True")
    p.add_argument("--dataset", type=str, default="CS")
    p.add_argument("--restore-from", type=str, default=None)
    p.add_argument("--channel-cfg", type=str, default=None)
    p.add_argument("--save-dir", type=str, default="./ckpt")
    p.add_argument("--precision", type=str, default="fp16", choices=("fp16", "fp8"),
                   help="fp8: the calibrated e4m3 engine (opt-in; accuracy on trained weights is unmeasured)")
    p.add_argument("--calib-batches", type=int, default=2,
                   help="fp8: batches the activation maxima are taken over (synthetic images without --data-para)")
    p.add_argument("--data-para", type=str, default=None,
                   help='fp8: JSON {"root": ..., "list_path": ...}: calibrate on the first batches of --dataset')
    p.add_argument("--seed", type=int, default=12345)
    return p


def get_num_classes(dataset):
    for prefix, n in (("CS", 19), ("CTX", 59), ("ADE", 150), ("COCO", 171)):
        if dataset.startswith(prefix):
            return n
    raise ValueError(dataset)


def benchmark(engine, x, nwarmup=10, nruns=50):
    """totrt.benchmark: warm-up, then nruns calls timed one by one with a synchronise around each."""
    for _ in range(nwarmup):
        engine(x)
    torch.cuda.synchronize()
    times = []
    for _ in range(nruns):
        t0 = time.perf_counter()
        engine(x)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sum(times) / len(times)


def calibration_batches(args, h, w, dev):
    """--calib-batches float32 batches: the first of the dataset's validation list with --data-para, else seeded
    N(0,1) images of the timed shape."""
    if args.data_para:
        from dcfp_amd.datasets import EvalLoader, build_dataset
        dataset = build_dataset(args.dataset, split="val", data_para=json.loads(args.data_para))
        for i, (image, _, _) in enumerate(EvalLoader(dataset, args.batch_size, dev, num_workers=2)):
            if i >= args.calib_batches:
                break
            yield image
        return
    gen = torch.Generator().manual_seed(args.seed)
    for _ in range(args.calib_batches):
        yield torch.randn(args.batch_size, 3, h, w, generator=gen).to(dev)


def main(argv=None):
    args = get_parser().parse_args(argv)
    h, w = map(int, args.input_size.split(","))
    model = getattr(networks, args.model).Seg_Model(
        backbone=args.backbone, backbone_para=json.loads(args.backbone_para), model_para=json.loads(args.model_para),
        num_classes=get_num_classes(args.dataset), align_corner=args.align_corner, criterion=None, deepsup=False)
    if args.channel_cfg:
        init_pruned_model(model, torch.load(args.channel_cfg, weights_only=False))
    if args.restore_from:
        load_model(model, args.restore_from)
    dev = torch.device("cuda:0")
    engine = deploy.build_engine(model.eval())
    if args.precision == "fp8":
        amax = deploy.calibrate(engine.to(dev), calibration_batches(args, h, w, dev))
        engine = deploy.build_engine(model, precision="fp8", amax=amax)
    os.makedirs(args.save_dir, exist_ok=True)
    path = os.path.join(args.save_dir, f"engine_{args.precision}.pth")
    torch.save(engine.state_dict(), path)
    print(f"saved {path}: {len(engine.plan)} layer records, "
          f"{sum(t.numel() * t.element_size() for t in engine.tensors) / 2 ** 20:.1f} MiB")
    engine = deploy.load_engine(path, dev)
    x = torch.randn(args.batch_size, 3, h, w, device=dev)
    avg = benchmark(engine, x)
    print(f"Average batch time: {avg * 1e3:.2f} ms ({args.batch_size / avg:.2f} images/s) "
          f"{args.model}-{args.backbone} {h}x{w} batch {args.batch_size} {args.precision} engine")
    return avg


if __name__ == "__main__":
    main()
