#!/usr/bin/env python
"""Evaluation driver — the command line and protocol of the reference's evaluate.py main() (evaluate.py:249-393): build
the (optionally slimmed, optionally frozen-to-fp16) model - or load a saved fp16 / fp8 engine (`--engine-file`) - predict batch by batch, accumulate the confusion matrix on
the device, print {'meanIU', 'IU_array'} and append IoU / precision / recall / FPS to result.txt in the snapshot
directory.  `--iou-type boundary` scores class boundaries only.

Without `--dataset` the data are SYNTHETIC (seeded rectangles).  With `--dataset CS|CTX|COCO --data-para '{"root": ...,
"list_path": ...}'` the validation list is read through datasets.EvalLoader: --longsize / --shortsize, the 8k+1 padding
of `--whole True --align-corner True`, palette PNGs with `--save-predict True`, and one process per GPU under
torchrun (`--ddp`, every file counted exactly once, the matrix summed over the ranks).  `--whole True` with more than
one scale or with --flip then runs evaluate.predict_vote: prediction, argmax and confusion matrix are one launch after
the network (`--fused-vote False`: the N x C x H x W path, for A/B).  `--whole False --fused-sliding True` runs
evaluate.predict_sliding_vote: the tiles of a pass as batches, then one vote launch.  `--device-png True` deflates
the palette PNGs of `--save-predict` on the device.  The test-split export is tools/evaluate_test.py, which shares
`build_model` and `predict_batch` with this file.  The ADE dataset is not part of it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dcfp_amd import deploy, evaluate as ev, networks, ops  # noqa: E402
from dcfp_amd.pruners import init_pruned_model  # noqa: E402
from dcfp_amd.utils.pyt_utils import load_model  # noqa: E402

FPS_WARMUP = 5        # evaluate.py:314


def str2bool(v):
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def get_parser():
    p = argparse.ArgumentParser(description="DCFP")
    p.add_argument("--ignore-label", type=int, default=255)
    p.add_argument("--batch-size", type=int, default=4)
    p.add_argument("--input-size", type=str, default="769,769")
    p.add_argument("--whole", type=str2bool, default="False", help="whole-image instead of sliding-window prediction")
    p.add_argument("--flip", type=str2bool, default="False")
    p.add_argument("--ms", type=str, default="1", help="comma-separated scales")
    p.add_argument("--iou-type", type=str, default="segm", choices=("segm", "boundary"))
    p.add_argument("--dilation-ratio", type=float, default=0.02)
    p.add_argument("--model", type=str, default="deeplabv3")
    p.add_argument("--backbone", type=str, default="resnet50")
    p.add_argument("--backbone-para", type=str, default='{"pretrained": false}')
    p.add_argument("--model-para", type=str, default="{}")
    p.add_argument("--align-corner", type=str2bool, default="True")
    p.add_argument("--restore-from", type=str, default=None)
    p.add_argument("--channel-cfg", type=str, default=None, help="path to channel_cfg.")
    p.add_argument("--use-trt", type=str2bool, default="False", help="evaluate through the frozen fp16 engine")
    p.add_argument("--engine-file", type=str, default=None,
                   help="evaluate through an engine saved by tools/deploy.py (fp16 or fp8); no model is built")
    p.add_argument("--num-classes", type=int, default=19)
    p.add_argument("--num-images", type=int, default=40)
    p.add_argument("--seed", type=int, default=12345)
    p.add_argument("--snapshot-dir", type=str, default="ckpt")
    p.add_argument("--dataset", type=str, default=None, help="choose dataset (default: synthetic data)")
    p.add_argument("--data-dir", type=str, default="val", help="choose data type.")
    p.add_argument("--data-para", type=str, default="{}", help='JSON: {"root": ..., "list_path": ...}')
    p.add_argument("--num-workers", type=int, default=8)
    p.add_argument("--longsize", type=int, default=-1)
    p.add_argument("--shortsize", type=int, default=-1)
    p.add_argument("--save-predict", type=str2bool, default="False", help="save predict images")
    p.add_argument("--ddp", type=str2bool, default="True")
    p.add_argument("--dist-backend", type=str, default=None, help="default: the engine's choice (nccl on a GPU)")
    p.add_argument("--fused-vote", type=str2bool, default=None,
                   help="multi-scale / flip whole-image prediction through evaluate.predict_vote "
                        "(default: True with --dataset, False without)")
    p.add_argument("--device-png", type=str2bool, default="False",
                   help="deflate the PNGs of --save-predict on the device (evaluate.encode_label_pngs)")
    p.add_argument("--fused-sliding", type=str2bool, default="False",
                   help="sliding-window prediction (--whole False) through evaluate.predict_sliding_vote: batched "
                        "tiles, one vote launch (DESIGN §12)")
    return p


class SyntheticSegDataset:
    """Images N(0,1); ground truth piecewise constant, so that a boundary metric means something: one class per image
    overlaid with seeded random rectangles of random classes, then ignore rectangles over about 5 % of the area."""

    def __init__(self, num_classes, ignore_label, size, seed, rectangles=24, ignore_rectangles=5):
        self.num_classes, self.ignore_label, self.size = num_classes, ignore_label, size
        self.rectangles, self.ignore_rectangles = rectangles, ignore_rectangles
        self.gen = torch.Generator().manual_seed(seed)

    def _int(self, lo, hi):
        return int(torch.randint(lo, max(lo + 1, hi), (1,), generator=self.gen))

    def labels(self, n):
        h, w = self.size
        lab = torch.empty((n, h, w), dtype=torch.int64)
        ih, iw = max(1, round(h * 0.1)), max(1, round(w * 0.1))     # 5 of 1 % each, overlaps aside
        for i in range(n):
            lab[i] = self._int(0, self.num_classes)
            for _ in range(self.rectangles):
                rh, rw = self._int(max(1, h // 16), max(2, h // 2)), self._int(max(1, w // 16), max(2, w // 2))
                y, x = self._int(0, h - rh + 1), self._int(0, w - rw + 1)
                lab[i, y:y + rh, x:x + rw] = self._int(0, self.num_classes)
            for _ in range(self.ignore_rectangles):
                y, x = self._int(0, h - ih + 1), self._int(0, w - iw + 1)
                lab[i, y:y + ih, x:x + iw] = self.ignore_label
        return lab

    def batch(self, n, device):
        h, w = self.size
        images = torch.randn(n, 3, h, w, generator=self.gen)
        return images.to(device), self.labels(n).to(device)


def build_model(args):
    model = getattr(networks, args.model).Seg_Model(
        backbone=args.backbone, backbone_para=json.loads(args.backbone_para), model_para=json.loads(args.model_para),
        num_classes=args.num_classes, align_corner=args.align_corner, criterion=None, deepsup=False)
    if args.channel_cfg:
        init_pruned_model(model, torch.load(args.channel_cfg, weights_only=False))
    if args.restore_from:
        load_model(model, args.restore_from)
    return model.eval()


def load_engine_file(args, device):
    """The saved engine of --engine-file on `device`; its class count and align_corner replace the command line's."""
    if deploy.is_flat_file(args.engine_file):       # a flat engine file (its magic says so): the C runtime runs it
        engine = deploy.CEngine(args.engine_file, device)
        records = engine.n_records
    else:
        engine = deploy.load_engine(args.engine_file, device)
        records = len(engine.plan)
    args.num_classes, args.align_corner = engine.num_classes, engine.align_corner
    print(f"engine {args.engine_file}: format {engine.format}, {engine.meta['dtype']}, {engine.meta['model']}, "
          f"{records} layer records" + (", C runtime" if isinstance(engine, deploy.CEngine) else ""), flush=True)
    return engine


def predict_batch(model, image, args, scales, fused, size, label=None, conf=None):
    """One batch of a dataset through the prediction branch the command line selects (module docstring).  image: as
    the loader served it; size: the files' own (H, W).  With `label` and `conf`, and where the branch allows it, the
    confusion matrix is counted in the same launch.  -> (pred int32 [N,H,W], counted, seconds of the prediction, the
    network's input size)."""
    h, w = map(int, args.input_size.split(","))
    C = args.num_classes
    resized = args.longsize > 0 or args.shortsize > 0
    if args.longsize > 0:
        image = ev.generate_size_image(image, args.longsize, "long")
    elif args.shortsize > 0:
        image = ev.generate_size_image(image, args.shortsize, "short")
    size_scale = tuple(image.shape[2:])
    if args.whole and args.align_corner:
        image = ev.pad_inf(image)
    torch.cuda.synchronize()
    start_time = time.perf_counter()
    counted = False
    if args.whole and scales == [1.0] and not args.flip and not resized:
        pred = ev.predict_labels(model, image)[:, :size_scale[0], :size_scale[1]].contiguous()
    elif (fused if args.whole else getattr(args, "fused_sliding", False)):
        counted = not resized and conf is not None        # vote, argmax and confusion: one launch after the network
        outputs = dict(out_hw=size_scale, labels=label if counted else None, conf=conf if counted else None,
                       want_scores=resized, ignore_index=args.ignore_label)
        if args.whole:
            pred, scores = ev.predict_vote(model, image, scales, args.flip, args.align_corner, **outputs)
        else:
            pred, scores = ev.predict_sliding_vote(model, image, (h, w), scales, args.flip, args.align_corner, **outputs)
        if resized:
            pred = ops.upsample_argmax(scores, size, False)
    else:
        output = ev.predict_multiscale(model, image, (h, w), scales, C, args.flip, args.align_corner,
                                       args.whole)
        output = output[:, :, :size_scale[0], :size_scale[1]].contiguous()
        pred = ops.upsample_argmax(output, size, not resized)   # same size, corners aligned: the plain argmax
    torch.cuda.synchronize()
    return pred, counted, time.perf_counter() - start_time, tuple(image.shape)


def main(argv=None):
    parser = get_parser()
    if parser.parse_known_args(argv)[0].dataset is not None:
        return main_dataset(parser, argv)
    args = parser.parse_args(argv)
    h, w = map(int, args.input_size.split(","))
    scales = [float(s) for s in args.ms.split(",")]
    device = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    if args.engine_file:
        model = load_engine_file(args, device)
    else:
        model = build_model(args)
        model = deploy.build_engine(model).to(device) if args.use_trt else model.to(device)
    C = args.num_classes
    dataset = SyntheticSegDataset(C, args.ignore_label, (h, w), args.seed)
    boundary = args.iou_type == "boundary"
    conf = torch.zeros((C, C + 1 if boundary else C), dtype=torch.int64, device=device)
    nbatches = max(1, (args.num_images + args.batch_size - 1) // args.batch_size)
    warmup = min(FPS_WARMUP, nbatches - 1)       # (the reference needs more than 5 batches; fewer are all timed but one)
    pure_inf_time, metric_time, timed_images, fps = 0.0, 0.0, 0, 0.0
    for idx in range(nbatches):
        n = min(args.batch_size, args.num_images - idx * args.batch_size) if args.num_images > 0 else args.batch_size
        image, label = dataset.batch(n, device)
        with torch.no_grad():
            torch.cuda.synchronize()
            start_time = time.perf_counter()
            if args.whole and scales == [1.0]:
                pred = ev.predict_labels(model, image)
            elif args.whole and args.fused_vote:
                pred, _ = ev.predict_vote(model, image, scales, args.flip, args.align_corner)
            elif not args.whole and args.fused_sliding:
                pred, _ = ev.predict_sliding_vote(model, image, (h, w), scales, args.flip, args.align_corner)
            else:
                output = ev.predict_multiscale(model, image, (h, w), scales, C, args.flip, args.align_corner, args.whole)
                pred = ops.upsample_argmax(output, (h, w), True)      # same size, corners aligned: the plain argmax
            torch.cuda.synchronize()
            elapsed = time.perf_counter() - start_time
            if boundary:
                ev.boundary_confusion_matrix(label, pred, C, args.dilation_ratio, args.ignore_label, out=conf)
            else:
                ev.get_confusion_matrix(label, pred, C, args.ignore_label, out=conf)
            torch.cuda.synchronize()
            metric = time.perf_counter() - start_time - elapsed
        print_str = " Iter%d/%d" % (idx + 1, nbatches)
        if idx >= warmup:
            pure_inf_time += elapsed
            metric_time += metric
            timed_images += n
            fps = timed_images / pure_inf_time
            print_str += f" FPS: {fps:.2f} img / s, metric {metric * 1e3:.3f} ms"
        print(print_str, flush=True)

    return report(args, conf, C, fps, timed_images, metric_time * 1e3 / max(1, nbatches - warmup))


def report(args, conf, C, fps, timed_images, metric_ms_per_batch):
    """Metrics of the accumulated matrix: printed, and appended to result.txt in the snapshot directory."""
    boundary = args.iou_type == "boundary"
    if boundary:
        mean_IU, IU_array = ev.boundary_iou(conf)
    else:
        mean_IU, IU_array = ev.mean_iou(conf)
    cm = conf.double().cpu()
    pos, res, tp = cm.sum(1), cm[:, :C].sum(0), cm[:, :C].diag()
    IU_array = IU_array.cpu().numpy()
    p, r = tp / (res + 1e-5), tp / (pos + 1e-5)
    print({"meanIU": mean_IU, "IU_array": IU_array})
    os.makedirs(args.snapshot_dir, exist_ok=True)
    with open(os.path.join(args.snapshot_dir, "result.txt"), "a") as f:
        f.write("test with {}\n".format(args.restore_from))
        f.write(json.dumps({"meanIU": mean_IU, "IU_array": IU_array.tolist()}) + "\n")
        f.write(json.dumps({"meanP": p.mean().item(), "p": p.tolist()}) + "\n")
        f.write(json.dumps({"meanR": r.mean().item(), "r": r.tolist()}) + "\n")
        f.write(json.dumps({"FPS": fps, "iou_type": args.iou_type, "images": timed_images,
                            "metric_ms_per_batch": metric_ms_per_batch,
                            "tp": tp.tolist(), "pos": pos.tolist(), "res": res.tolist()}) + "\n")
        f.write("--------\n")
    return mean_IU


def main_dataset(parser, argv=None):
    """The reference's protocol on a dataset's validation list (module docstring)."""
    import torch.distributed as dist
    from dcfp_amd.datasets import EvalLoader, build_dataset
    from dcfp_amd.engine import Engine
    if argv is not None:
        sys.argv = [sys.argv[0]] + list(argv)            # the engine reads --ddp / --local_rank from the command line
    backend = parser.parse_known_args(argv)[0].dist_backend
    with Engine(custom_parser=parser, backend=backend) as engine:
        args = parser.parse_args(argv)
        scales = [float(s) for s in args.ms.split(",")]
        fused = True if args.fused_vote is None else args.fused_vote
        rank, world = (dist.get_rank(), engine.world_size) if engine.distributed else (0, 1)
        device = torch.device("cuda", engine.local_rank if engine.distributed else 0)
        torch.cuda.set_device(device)
        torch.manual_seed(args.seed)
        dataset = build_dataset(args.dataset, split="val", data_dir=args.data_dir, ignore_label=args.ignore_label,
                                data_para=json.loads(args.data_para))
        C = args.num_classes = dataset.num_classes
        loader = EvalLoader(dataset, max(1, args.batch_size // world), device, num_workers=args.num_workers,
                            rank=rank, world_size=world)
        if args.engine_file:
            model = load_engine_file(args, device)
            if model.num_classes != dataset.num_classes:
                raise ValueError(f"--engine-file has {model.num_classes} classes, the dataset {dataset.num_classes}")
        else:
            model = build_model(args)
            model = deploy.build_engine(model).to(device) if args.use_trt else model.to(device)
        palette = [int(v) for v in dataset.cmap_labels.reshape(-1)]
        save_path = os.path.join(args.snapshot_dir, "outputs")
        if args.save_predict:
            os.makedirs(save_path, exist_ok=True)
        boundary = args.iou_type == "boundary"
        conf = torch.zeros((C, C + 1 if boundary else C), dtype=torch.int64, device=device)
        nbatches = len(loader)
        warmup = min(FPS_WARMUP, nbatches - 1)
        pure_inf_time, metric_time, timed_images, timed_batches, fps = 0.0, 0.0, 0, 0, 0.0
        for idx, (image, label, metas) in enumerate(loader):
            size = metas[0]["size"]
            with torch.no_grad():
                pred, counted, elapsed, in_shape = predict_batch(model, image, args, scales, fused, size, label,
                                                                 None if boundary else conf)
                start_time = time.perf_counter()
                if boundary:
                    ev.boundary_confusion_matrix(label, pred, C, args.dilation_ratio, args.ignore_label, out=conf)
                elif not counted:
                    ev.get_confusion_matrix(label, pred, C, args.ignore_label, out=conf)
                torch.cuda.synchronize()
                metric = time.perf_counter() - start_time
            if args.save_predict and args.device_png:
                for meta, files in zip(metas, ev.encode_label_pngs(pred, None, [palette])):
                    with open(os.path.join(save_path, meta["name"] + ".png"), "wb") as f:
                        f.write(files[0])
            elif args.save_predict:
                for i, meta in enumerate(metas):
                    ev.save_palette_png(pred[i].cpu().numpy(), palette, os.path.join(save_path, meta["name"] + ".png"))
            print_str = " Iter%d/%d" % (idx + 1, nbatches)
            if idx >= warmup:
                pure_inf_time += elapsed
                metric_time += metric
                timed_images += in_shape[0]
                timed_batches += 1
                fps = timed_images / pure_inf_time
                print_str += f" FPS: {fps:.2f} img / s, metric {metric * 1e3:.3f} ms"
            if rank == 0:
                print(print_str, flush=True)
        if engine.distributed:
            if dist.get_backend() == "gloo":                      # gloo reduces on the host
                total = conf.cpu()
                dist.all_reduce(total)
                conf = total.to(device)
            else:
                dist.all_reduce(conf)
            torch.cuda.synchronize()
            dist.destroy_process_group()
        if rank != 0:
            return None
        cm = conf[:, :C]
        print(json.dumps({"tp": int(cm.diag().sum()), "pos": int(conf.sum()), "res": int(cm.sum())}))
        return report(args, conf, C, fps, timed_images, metric_time * 1e3 / max(1, timed_batches))

if __name__ == "__main__":
    main()
