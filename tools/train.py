#!/usr/bin/env python
"""Training + scoring driver — the loop of the reference's train.py:140-293 (same flags for
the model / optimiser / loss / pruning options).  Without --dataset it runs over SYNTHETIC Cityscapes-shaped
batches; with --dataset CS|CTX|COCO (and the reference's data flags) it reads a list file through dcfp_amd.datasets,
whose augmentation chain runs on the device (ADE is not built).
`--loss-type ...,kd --teacher-from CKPT` adds the distillation term against a frozen teacher.
`--loss-type gsrl,kdpa` / `gsrl,kd,kdpa` adds the pair-wise similarity term on the backbone's last feature against the same
teacher; `--loss-para '{"pa_weight": 1.0, "pa_pool": 2}'` sets its weight and its pooling window.
`--loss-type ce,lovasz` / `gsrl,lovasz` adds the Lovasz-Softmax term on the main head, the surrogate of the per-class IoU
(DESIGN §18); `--loss-para '{"lovasz_weight": 1.0, "lovasz_bins": 1024}'` sets its weight and its error bins.
`--prune-type taylor | taylor_w` scores by first-order Taylor instead of `dcfp`, `--slim-lambda` adds the Network
Slimming L1 term to the BN weight gradients (the baseline criteria).
`--state-every N` writes the whole training state after every N-th step and `-c/--continue FILE` runs on from such a
file, leaving the bits the uninterrupted run leaves (dcfp_amd/train_state.py); `--log-digest N` prints a
128-bit digest of the parameter arena every N steps, so two runs can be compared from their logs.
One process per GPU: `python -m torch.distributed.run --nproc-per-node N tools/train.py ...`."""
import argparse
import json
import math
import os
import os.path as osp
import sys
import time

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
import torch  # noqa: E402

from dcfp_amd import networks, pruners, train_state  # noqa: E402
from dcfp_amd.engine import Engine  # noqa: E402
from dcfp_amd.loss.criterion import build_criterions  # noqa: E402
from dcfp_amd.optimizer import adjust_learning_rate, build_optimizer  # noqa: E402
from dcfp_amd.utils.pyt_utils import load_model  # noqa: E402


def str2bool(v):
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def get_parser():
    p = argparse.ArgumentParser(description="DCFP")
    p.add_argument("--start-iters", type=int, default=0)
    p.add_argument("--resume", type=str, default=None)
    p.add_argument("--num-steps", type=int, default=40000)
    p.add_argument("--random-seed", type=int, default=12345)
    p.add_argument("--ddp", type=str2bool, default="True")
    p.add_argument("--save-pred-every", type=int, default=10000)
    p.add_argument("--save-steps", type=int, default=0)
    p.add_argument("--snapshot-dir", type=str, default="ckpt")
    p.add_argument("--batch-size", type=int, default=8, help="global batch (split over ranks)")
    p.add_argument("--ignore-label", type=int, default=255)
    p.add_argument("--input-size", type=str, default="769,769")
    p.add_argument("--num-classes", type=int, default=19)
    p.add_argument("--model", type=str, default="deeplabv3")
    p.add_argument("--backbone", type=str, default="resnet50")
    p.add_argument("--backbone-para", type=str, default='{"pretrained": false}')
    p.add_argument("--model-para", type=str, default="{}")
    p.add_argument("--align-corner", type=str2bool, default="True")
    p.add_argument("--no-decay", type=str, default=None)
    p.add_argument("--optim", type=str, default="sgd")
    p.add_argument("--learning-rate", type=float, default=1e-2)
    p.add_argument("--weight-decay", type=float, default=0.0005)
    p.add_argument("--power", type=float, default=0.9)
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--betas", type=str, default="0.9,0.999")
    p.add_argument("--warmup", type=int, default=-1)
    p.add_argument("--deepsup", type=str2bool, default="True")
    p.add_argument("--loss-type", type=str, default="ce",
                   help="ce, ohem, gsrl, kd, kdpa or lovasz, or several joined by commas and summed: ce,kd / gsrl,kd,kdpa / "
                        "gsrl,lovasz")
    p.add_argument("--loss-para", type=str, default="{}",
                   help="JSON of the criteria's keyword arguments: ds_weight, kd_weight, kd_T, kd_mode, pa_weight, pa_pool, lovasz_weight, "
                        "lovasz_bins (a power of two in 64 .. 4096), ...")
    p.add_argument("--prune-type", type=str, default=None,
                   help="score while training and write score.pth: dcfp (the EIC score), taylor (first-order Taylor on "
                        "the BN gate) or taylor_w (on the filters); DESIGN §17")
    p.add_argument("--clip-grad-norm", type=float, default=None,
                   help="clip the global gradient norm to this value inside the optimizer launch (the gradients "
                        "themselves stay unscaled); the log line gains gnorm=")
    p.add_argument("--ema-decay", type=float, default=None,
                   help="keep an exponential moving average of the weights (0.5 < decay < 1) as optimizer state; every "
                        "CS_scenes_<k>.pth gets a CS_scenes_<k>_ema.pth beside it")
    p.add_argument("--slim-lambda", type=float, default=0.0,
                   help="Network Slimming: add lambda * sign(gamma) to the BN weight gradients before every optimizer "
                        "step (0 = off), in any --prune-type")
    p.add_argument("--channel-cfg", type=str, default=None)
    p.add_argument("--teacher-from", type=str, default=None,
                   help="checkpoint of the frozen teacher of --loss-type ...,kd / ...,kdpa: same --model, --backbone and classes as "
                        "the student, built without --channel-cfg (the dense model the student was pruned from)")
    p.add_argument("--teacher-engine", type=str2bool, default="True",
                   help="freeze the teacher into the fp16 deployment engine (default) or keep the fp32 model")
    p.add_argument("--teacher-channel-cfg", type=str, default=None, help="channel_cfg.pth of a teacher that is itself slim")
    p.add_argument("--dataset", type=str, default=None,
                   help="CS, CTX or COCO: read real data through dcfp_amd.datasets (default: synthetic batches)")
    p.add_argument("--data-dir", type=str, default="train", help="name of the data split (kept for the reference's scripts)")
    p.add_argument("--random-mirror", action="store_true")
    p.add_argument("--random-brightness", action="store_true")
    p.add_argument("--random-scale", action="store_true")
    p.add_argument("--balance", type=int, default=0, help="1 / 2: per-crop class-balance weights for the GSRL loss")
    p.add_argument("--longsize", type=int, default=-1)
    p.add_argument("--shortsize", type=int, default=-1)
    p.add_argument("--data-para", type=str, default="{}",
                   help='JSON: "root" and "list_path" of the dataset, further DataSet keywords '
                        '("resample": true for the class-balanced sampler of the fine-tune recipes; "target_class" for '
                        '--balance 2 without it)')
    p.add_argument("--state-every", type=int, default=0,
                   help="after every N-th step write train_state_<k>.pth into --snapshot-dir: everything -c/--continue "
                        "needs to run on bit-identically (0 = off); DESIGN §20")
    p.add_argument("--keep-states", type=int, default=2, help="state files kept after a successful write (0 = all)")
    p.add_argument("--log-digest", type=int, default=0,
                   help="every N steps print `digest it=<k> params=<d0>:<d1>`, the 128-bit digest of the parameter arena")
    p.add_argument("--log-time", type=str2bool, default="False",
                   help="synchronise after every iteration and print its device time (batch synthesis excluded)")
    return p


class SyntheticDataset:
    """Cityscapes-shaped tensors: images N(0,1), labels uniform in [0,num_classes) with 5 % ignore."""

    def __init__(self, num_classes, ignore_label, size, seed):
        self.num_classes, self.ignore_label, self.class_weights = num_classes, ignore_label, None
        self.size, self.gen = size, torch.Generator().manual_seed(seed)

    def batch(self, n, device):
        h, w = self.size
        images = torch.randn(n, 3, h, w, generator=self.gen)
        labels = torch.randint(0, self.num_classes, (n, h, w), generator=self.gen)
        labels[torch.rand(n, h, w, generator=self.gen) < 0.05] = self.ignore_label
        return images.to(device, non_blocking=True), labels.to(device, non_blocking=True)


TEACHER_TERMS = ("kd", "kdpa")      # loss types that read the frozen teacher: its logits / its backbone feature
TAYLOR_TYPES = {"taylor": "gate", "taylor_w": "weight"}      # --prune-type -> pruners.taylor_pruning(mode=...)


def check_args(args):
    """Argument combinations that cannot run, refused before anything is built."""
    for term in TEACHER_TERMS:
        if term in args.loss_type.split(",") and not args.teacher_from:
            raise ValueError("--loss-type %s: the %s term needs a teacher, give --teacher-from CKPT" % (args.loss_type, term))
    if args.prune_type is not None and args.prune_type.startswith("taylor") and args.prune_type not in TAYLOR_TYPES:
        raise ValueError("--prune-type %s: the Taylor scorers are %s" % (args.prune_type, ", ".join(sorted(TAYLOR_TYPES))))
    if not args.slim_lambda >= 0.0:
        raise ValueError("--slim-lambda %r: the sparsity weight is >= 0 (0 = off)" % args.slim_lambda)
    clip, decay = getattr(args, "clip_grad_norm", None), getattr(args, "ema_decay", None)
    if clip is not None and not (math.isfinite(clip) and clip > 0):
        raise ValueError("--clip-grad-norm %r: the largest gradient norm is finite and > 0" % clip)
    if decay is not None and not 0.5 < decay < 1.0:
        raise ValueError("--ema-decay %r: the decay lies in (0.5, 1)" % decay)
    if getattr(args, "continue_fpath", None):
        if args.resume:
            raise ValueError("-c/--continue restores the weights itself: give it without --resume")
        if args.start_iters != 0:
            raise ValueError("-c/--continue takes the step counter from the state file: give it without --start-iters")
    if args.state_every < 0 or args.keep_states < 0 or args.log_digest < 0:
        raise ValueError("--state-every, --keep-states and --log-digest are >= 0")


def build_teacher(args, num_classes, device):
    """The frozen teacher of the kd term (dcfp_amd.distill): the student's architecture at the checkpoint's widths."""
    from dcfp_amd.distill import Teacher
    net = getattr(networks, args.model).Seg_Model(
        backbone=args.backbone, backbone_para=json.loads(args.backbone_para), model_para=json.loads(args.model_para),
        num_classes=num_classes, align_corner=args.align_corner, criterion=None, deepsup=args.deepsup)
    if args.teacher_channel_cfg is not None:
        pruners.init_pruned_model(net, torch.load(args.teacher_channel_cfg, weights_only=False))
    return Teacher.from_checkpoint(net, args.teacher_from, engine=args.teacher_engine).to(device)


def raise_nonfinite_gradient(optimizer, seg_model, gnorm):
    """The gradient norm of the step is not finite: name the first parameter whose squared norm is not."""
    names = {id(p): n for n, p in seg_model.named_parameters()}
    for p, sq in optimizer.grad_sqnorms():
        if not math.isfinite(float(sq)):
            raise FloatingPointError("gradient norm is %r: the gradient of %s is not finite (squared norm %r)"
                                     % (gnorm, names.get(id(p), "<unnamed>"), float(sq)))
    raise FloatingPointError("gradient norm is %r (every per-parameter squared norm is finite)" % gnorm)


def main(argv=None):
    parser = get_parser()
    if argv is not None:
        sys.argv = [sys.argv[0]] + list(argv)
    with Engine(custom_parser=parser) as engine:
        args = parser.parse_args()
        check_args(args)
        main_flag = (not engine.distributed) or engine.local_rank == 0
        if main_flag:
            os.makedirs(args.snapshot_dir, exist_ok=True)
        args.save_steps = min(args.save_steps or args.num_steps, args.num_steps)
        seed = args.random_seed + (engine.local_rank if engine.distributed else 0)
        torch.manual_seed(seed)
        h, w = map(int, args.input_size.split(","))
        if args.dataset is None:
            dataset = SyntheticDataset(args.num_classes, args.ignore_label, (h, w), seed)
        else:
            from dcfp_amd.datasets import build_dataset
            data_para = json.loads(args.data_para)
            target_class = data_para.pop("target_class", None)
            dataset = build_dataset(args.dataset, split="train", data_dir=args.data_dir, crop_size=(h, w),
                                    scale=args.random_scale, mirror=args.random_mirror,
                                    brightness=args.random_brightness, ignore_label=args.ignore_label,
                                    balance=args.balance, longsize=args.longsize, shortsize=args.shortsize,
                                    data_para=data_para)
        criterion = build_criterions(args.loss_type, dataset, json.loads(args.loss_para))
        seg_model = getattr(networks, args.model).Seg_Model(
            backbone=args.backbone, backbone_para=json.loads(args.backbone_para),
            model_para=json.loads(args.model_para), num_classes=dataset.num_classes,
            align_corner=args.align_corner, criterion=criterion, deepsup=args.deepsup)
        if args.channel_cfg is not None:
            channel_cfg = torch.load(args.channel_cfg, weights_only=False)
            pruners.init_pruned_model(seg_model, channel_cfg)
            if main_flag:
                torch.save(channel_cfg, osp.join(args.snapshot_dir, "channel_cfg.pth"))
        if args.resume:
            load_model(seg_model, args.resume)
        wants_state = bool(args.continue_fpath) or args.state_every > 0
        state_fp = train_state.fingerprint(args, seg_model, dataset.num_classes, engine.world_size) if wants_state else None
        state, start_iters = None, args.start_iters
        if args.continue_fpath:
            # the weights go in where --resume puts them: before the move to the device and before the optimizer's arena
            # adopts them, so the permuted copies and kept filters of the first forward are built from the loaded weights
            with train_state.Timer() as t_restore:
                state = train_state.load(args.continue_fpath)
                start_iters = train_state.restore_model(state, seg_model, state_fp)
        device = torch.device("cuda", engine.local_rank)
        seg_model.to(device)
        optimizer = build_optimizer(args, seg_model)
        optimizer.zero_grad()
        # (built after the optimizer and never handed to it: the teacher's parameters stay out of the arenas)
        wants_kd, wants_pa = ("kd" in args.loss_type.split(",")), ("kdpa" in args.loss_type.split(","))
        teacher = build_teacher(args, dataset.num_classes, device) if (wants_kd or wants_pa) else None
        if hasattr(criterion, "attach"):
            criterion.attach(seg_model)            # (the bare model: the tap sits under any data-parallel wrapper)
        train_pruning = pruners.dcfp_pruning(seg_model, 0.999) if args.prune_type == "dcfp" else None
        if args.prune_type in TAYLOR_TYPES:
            train_pruning = pruners.taylor_pruning(seg_model, TAYLOR_TYPES[args.prune_type])
        slimming = pruners.slimming_regularizer(seg_model, args.slim_lambda) if args.slim_lambda > 0 else None
        model = engine.data_parallel(seg_model)
        model.train()
        per_rank = max(1, args.batch_size // engine.world_size)
        batches = None
        if args.dataset is not None:
            from dcfp_amd.datasets import TrainLoader
            with torch.cuda.device(device):
                loader = TrainLoader(dataset, per_rank, device, seed=args.random_seed, target_class=target_class)
            if len(loader) == 0:
                raise ValueError("the list file holds fewer samples than one batch per rank")

            def epochs():
                while True:
                    yield from loader
            batches = epochs()
        source = dataset if batches is None else loader
        if state is not None:
            # (after torch.manual_seed above and after everything that draws while the model is built)
            with train_state.Timer() as t_rest:
                train_state.restore_rest(state, optimizer, train_pruning, device, source,
                                         rank=torch.distributed.get_rank() if engine.distributed else 0)
            if main_flag:
                print("continued from %s at iteration %d (restore %.3f s)"
                      % (args.continue_fpath, start_iters, t_restore.seconds + t_rest.seconds), flush=True)
            state = None
        for it in range(start_iters, args.num_steps):
            if batches is None:
                images, labels = dataset.batch(per_rank, device)
            else:
                with torch.cuda.device(device):
                    images, labels = next(batches)
            if args.log_time:
                torch.cuda.synchronize()
                t_it = time.perf_counter()
            if "gsrl" in args.loss_type and not isinstance(labels, dict):
                if batches is not None:
                    raise ValueError("--loss-type gsrl on --dataset needs --balance 1 or 2 (the per-crop weights)")
                # fine-tune stage: {'ori', 'weight'} labels (datasets/Base.py:73-89); --dataset with --balance brings real ones
                labels = {"ori": labels, "weight": 1.0 + (labels % 3 == 0).float()}
            if teacher is not None:
                labels = dict(labels) if isinstance(labels, dict) else {"ori": labels}
                if wants_pa:                         # one run of the teacher serves both terms
                    logits, labels["teacher_feat"] = teacher(images, feature=True)
                    if wants_kd:
                        labels["teacher"] = logits
                else:
                    labels["teacher"] = teacher(images)
            optimizer.zero_grad()
            lr = adjust_learning_rate(optimizer, args.learning_rate, it, args.num_steps, args.power, args.warmup)
            loss = model(images, labels, deepsup=args.deepsup)
            if not bool(loss["loss"] == loss["loss"]):     # (train.py:260-261 asserts this - a host sync per step, as there)
                from dcfp_amd import syncbn_p2p
                syncbn_p2p.check_all()                     # a SyncBN exchange that gave up on a peer poisons with NaN: say so
                from dcfp_amd import ops as _ops
                _ops.check_fused_status()                  # ... and so does a fused BatchNorm backward that gave up
                raise AssertionError("loss is NaN")
            reduce_loss = engine.all_reduce_tensor(loss["loss"])
            loss["loss"].backward()
            if train_pruning is not None:
                train_pruning.step(seg_model)
            if slimming is not None:
                slimming.step(seg_model)
            optimizer.step()
            if args.log_time:
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t_it) * 1e3
                if main_flag:
                    print("  step %.1f ms  %.2f images/s/GPU" % (ms, per_rank / ms * 1e3), flush=True)
            if main_flag:
                gnorm = ""
                if args.clip_grad_norm is not None:
                    gn = float(optimizer.grad_norm())      # (the loss read below syncs anyway)
                    if not math.isfinite(gn):
                        raise_nonfinite_gradient(optimizer, seg_model, gn)
                    gnorm = " gnorm=%.4e" % gn
                print("Iters%d/%d lr=%.2e loss=%.4f%s" % (it + 1, args.num_steps, lr, reduce_loss.item(), gnorm),
                      flush=True)
                done = it + 1
                if done >= args.save_steps and ((args.num_steps - done) % args.save_pred_every == 0 or done >= args.num_steps):
                    torch.save(seg_model.state_dict(), osp.join(args.snapshot_dir, "CS_scenes_%d.pth" % done))
                    if args.ema_decay is not None:
                        torch.save(optimizer.ema_state_dict(seg_model),
                                   osp.join(args.snapshot_dir, "CS_scenes_%d_ema.pth" % done))
            if args.log_digest > 0 and (it + 1) % args.log_digest == 0 and main_flag:
                from dcfp_amd import ops as _ops
                print("digest it=%d params=%s" % (it + 1, train_state.format_digest(
                    _ops.state_digest(optimizer.arena().flat_param))), flush=True)
            if args.state_every > 0 and (it + 1) % args.state_every == 0:
                with train_state.Timer() as t_save:          # (every rank: the digests are compared across the ranks)
                    snap = train_state.capture(it + 1, seg_model, optimizer, train_pruning, device, source, state_fp)
                    if not engine.distributed or torch.distributed.get_rank() == 0:
                        path = train_state.save(snap, train_state.state_path(args.snapshot_dir, it + 1))
                        train_state.prune_old(args.snapshot_dir, args.keep_states)
                    snap = None
                if not engine.distributed or torch.distributed.get_rank() == 0:
                    print("state %s (save %.3f s)" % (path, t_save.seconds), flush=True)
        if main_flag and train_pruning is not None:
            train_pruning.export_eic(osp.join(args.snapshot_dir, "score.pth"))
        from dcfp_amd import syncbn_p2p, ops as _ops
        _ops.check_fused_status()
        syncbn_p2p.finish()            # DCFP_SYNCBN_P2P=1: no exchange may have given up on a peer


if __name__ == "__main__":
    main()
