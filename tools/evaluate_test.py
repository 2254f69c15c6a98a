#!/usr/bin/env python
"""Test-split export — the command line and output layout of the reference's evaluate_test.py: predict a list of
unlabelled images and write, per image, `outputs/test_pred/<name>.png` (train ids, paletted with the dataset's
`cmap_labels`) and `outputs/test_id/<name before '_leftImg8bit'>.png` (grey, the dataset's own label ids: the
Cityscapes benchmark submission) under the directory of `--restore-from` (or `--snapshot-dir`).

Model building and the prediction branch are tools/evaluate.py's (`build_model`, `predict_batch`): predict_labels for
one scale without flip, predict_vote for `--whole True` with scales or flip, predict_multiscale otherwise, and with
--longsize / --shortsize the scores resized back to the file's own size before the argmax.  One process per GPU under
torchrun through Engine; datasets.EvalLoader serves every file to exactly one rank, so every PNG is written once.

`--device-png True` deflates both PNGs of a batch on the device in one launch sequence (evaluate.encode_label_pngs,
csrc/png.hip): the identity table and the reverse id table over the same int32 prediction, two small
device-to-host copies, files written by a few threads behind the next batch.  `--device-png False` copies the map to
the host and writes the same two files through PIL.  `--split val` exports a labelled list (labels are ignored): the
way to export Pascal-Context and COCO-Stuff, whose `test` split is not built."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:      # (a script's own directory already is)
    sys.path.append(os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import evaluate as tool  # noqa: E402  (tools/evaluate.py: build_model, predict_batch, str2bool)
from dcfp_amd import deploy, evaluate as ev  # noqa: E402

# --device-png: True because path B of tools/png_bench.py beats path A on both of its maps by far more than the 10 %
# that the rule of DESIGN §15 asks for
DEVICE_PNG_DEFAULT = "True"


def get_parser():
    str2bool = tool.str2bool
    p = argparse.ArgumentParser(description="DCFP")
    p.add_argument("--dataset", type=str, default="CS", help="choose dataset.")
    p.add_argument("--ignore-label", type=int, default=255)
    p.add_argument("--batch-size", type=int, default=4)
    p.add_argument("--restore-from", type=str, default=None)
    p.add_argument("--input-size", type=str, default="769,769")
    p.add_argument("--longsize", type=int, default=-1)
    p.add_argument("--shortsize", type=int, default=-1)
    p.add_argument("--num-workers", type=int, default=8)
    p.add_argument("--ddp", type=str2bool, default="True")
    p.add_argument("--align-corner", type=str2bool, default="True")
    p.add_argument("--whole", type=str2bool, default="False", help="whole-image instead of sliding-window prediction")
    p.add_argument("--flip", type=str2bool, default="False")
    p.add_argument("--ms", type=str, default="1", help="comma-separated scales")
    p.add_argument("--model", type=str, default="deeplabv3")
    p.add_argument("--backbone", type=str, default="resnet50")
    p.add_argument("--backbone-para", type=str, default='{"pretrained": false}')
    p.add_argument("--model-para", type=str, default="{}")
    p.add_argument("--channel-cfg", type=str, default=None, help="path to channel_cfg.")
    # this project's own
    p.add_argument("--data-para", type=str, default="{}", help='JSON: {"root": ..., "list_path": ...}')
    p.add_argument("--data-dir", type=str, default="test", help="choose data type.")
    p.add_argument("--split", type=str, default="test", choices=("test", "val"),
                   help="val: export a labelled list, labels ignored")
    p.add_argument("--use-trt", type=str2bool, default="False", help="predict through the frozen fp16 engine")
    p.add_argument("--seed", type=int, default=12345)
    p.add_argument("--dist-backend", type=str, default=None, help="default: the engine's choice (nccl on a GPU)")
    p.add_argument("--fused-vote", type=str2bool, default="True",
                   help="multi-scale / flip whole-image prediction through evaluate.predict_vote")
    p.add_argument("--snapshot-dir", type=str, default=None,
                   help="where outputs/ goes (default: the directory of --restore-from)")
    p.add_argument("--save-predict", type=str2bool, default="True",
                   help="accepted for the evaluation scripts' command line; the export always writes")
    p.add_argument("--device-png", type=str2bool, default=DEVICE_PNG_DEFAULT,
                   help="deflate the PNGs on the device (evaluate.encode_label_pngs)")
    return p


def output_names(name):
    """-> (file name under test_pred, file name under test_id) of the image `name` (evaluate_test.py:156,161)."""
    return name + ".png", name.split("_leftImg8bit")[0] + ".png"


def output_root(args):
    if args.snapshot_dir:
        return os.path.join(args.snapshot_dir, "outputs")
    if args.restore_from:
        return os.path.join(os.path.dirname(args.restore_from), "outputs")
    raise SystemExit("evaluate_test.py: --restore-from or --snapshot-dir must say where outputs/ goes")


def main(argv=None):
    import numpy as np
    import torch.distributed as dist
    from PIL import Image
    from dcfp_amd.datasets import EvalLoader, build_dataset
    from dcfp_amd.engine import Engine
    parser = get_parser()
    if argv is not None:
        sys.argv = [sys.argv[0]] + list(argv)            # the engine reads --ddp / --local_rank from the command line
    backend = parser.parse_known_args(argv)[0].dist_backend
    with Engine(custom_parser=parser, backend=backend) as engine:
        args = parser.parse_args(argv)
        scales = [float(s) for s in args.ms.split(",")]
        rank, world = (dist.get_rank(), engine.world_size) if engine.distributed else (0, 1)
        device = torch.device("cuda", engine.local_rank if engine.distributed else 0)
        torch.cuda.set_device(device)
        torch.manual_seed(args.seed)
        dataset = build_dataset(args.dataset, split=args.split, data_dir=args.data_dir, ignore_label=args.ignore_label,
                                data_para=json.loads(args.data_para))
        args.num_classes = dataset.num_classes
        loader = EvalLoader(dataset, max(1, args.batch_size // world), device, num_workers=args.num_workers,
                            rank=rank, world_size=world)
        model = tool.build_model(args)
        model = deploy.build_engine(model).to(device) if args.use_trt else model.to(device)
        palette = [int(v) for v in dataset.cmap_labels.reshape(-1)]
        reverse = ev.reverse_id_table(dataset)
        luts = torch.from_numpy(np.stack([np.arange(256, dtype=np.uint8), reverse])).to(device)
        save_path = output_root(args)
        pred_path, pred_id_path = os.path.join(save_path, "test_pred"), os.path.join(save_path, "test_id")
        for p in (pred_path, pred_id_path):
            os.makedirs(p, exist_ok=True)
        nbatches, images, first = len(loader), 0, None
        start = time.perf_counter()
        with ev.PngWriter() as writer:
            for idx, (image, _, metas) in enumerate(loader):
                with torch.no_grad():
                    pred = tool.predict_batch(model, image, args, scales, args.fused_vote, metas[0]["size"])[0]
                names = [output_names(meta["name"]) for meta in metas]
                if args.device_png:
                    for (pred_name, id_name), files in zip(names, ev.encode_label_pngs(pred, luts, [palette, None])):
                        writer.write(os.path.join(pred_path, pred_name), files[0])
                        writer.write(os.path.join(pred_id_path, id_name), files[1])
                else:
                    seg_pred = pred.cpu().numpy().astype(np.uint8)
                    for (pred_name, id_name), seg in zip(names, seg_pred):
                        Image.fromarray(reverse[seg]).save(os.path.join(pred_id_path, id_name))      # mode L
                        ev.save_palette_png(seg, palette, os.path.join(pred_path, pred_name))
                images += len(metas)
                if first is None:                            # the first batch warms up: rated apart
                    writer.drain()
                    first = (time.perf_counter(), images)
                if rank == 0:
                    print(" Iter%d/%d" % (idx + 1, nbatches), flush=True)
        seconds = time.perf_counter() - start                # the writer is drained: every file is on its way to disk
        if engine.distributed:
            dist.barrier()
            dist.destroy_process_group()
        end = start + seconds
        rate = (images - first[1]) / max(end - first[0], 1e-9) if first and images > first[1] else None
        print(json.dumps({"rank": rank, "images": images, "seconds": seconds, "images_per_s_after_first_batch": rate,
                          "device_png": bool(args.device_png), "outputs": save_path}), flush=True)
        if rank == 0:
            print("end")
        return images


if __name__ == "__main__":
    main()
