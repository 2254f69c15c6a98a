#!/usr/bin/env python
"""What resumable training costs, three numbers on one GPU:

  digest   ops.state_digest on a buffer of the DeepLabv3-R101 arena size (65 M floats, 260 MB) against torch.clone of the
           same buffer, by device events around ten calls of each, the two alternating in one loop (per-call times).
           The clone moves twice the bytes (a read and a write), the digest reads only: a digest slower than the clone
           means the kernel is wrong-shaped.
  save     train_state.capture + train_state.save of DeepLabv3-R101 with FusedSGD and the DCFP scorer after one training
           step (digests, copies to the host, torch.save, fsync, rename), host clock around a device synchronise
  restore  train_state.load + restore_model + restore_rest of that file into a freshly built model (the move of the model
           to the device and the optimizer's construction are the run's own start-up and stay outside the clock)

    python tools/state_bench.py [--reps 20] [--words 65000000] [--dir DIR]

prints one JSON line.  Nothing here asserts a time."""
import argparse
import json
import os
import os.path as osp
import sys
import tempfile
import time

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
import torch  # noqa: E402

from dcfp_amd import networks, ops, pruners, train_state  # noqa: E402
from dcfp_amd.loss.criterion import build_criterions  # noqa: E402
from dcfp_amd.optimizer import build_optimizer  # noqa: E402


def bench_digest(dev, words, reps):
    buf = torch.randn(words, device=dev)
    for _ in range(3):                                   # warm-up: code objects, the workspace, the allocator's blocks
        ops.state_digest_device(buf)
        buf.clone()
    torch.cuda.synchronize()
    times = {"digest": [], "clone": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    inner = 10               # calls per timed window, back to back: the queue stays full and the host's launch path is hidden
    for _ in range(reps):
        ev[0].record()
        for _ in range(inner):
            ops.state_digest_device(buf)
        ev[1].record()
        for _ in range(inner):
            c = buf.clone()
        ev[2].record()
        torch.cuda.synchronize()
        times["digest"].append(ev[0].elapsed_time(ev[1]) / inner)
        times["clone"].append(ev[1].elapsed_time(ev[2]) / inner)
        del c
    out = {"words": words, "reps": reps}
    for k, moved in (("digest", 4 * words), ("clone", 8 * words)):
        t = sorted(times[k])
        med = t[len(t) // 2]
        out[k + "_ms_median"], out[k + "_ms_min"], out[k + "_ms_max"] = round(med, 4), round(t[0], 4), round(t[-1], 4)
        out[k + "_TBps_median"] = round(moved / med * 1e-9, 3)
    return out


class _Args:
    model, backbone, backbone_para, model_para = "deeplabv3", "resnet101", '{"pretrained": false}', "{}"
    optim, momentum, learning_rate, weight_decay, no_decay, betas = "sgd", 0.9, 1e-2, 5e-4, None, "0.9,0.999"
    num_steps, power, warmup, batch_size, loss_type, loss_para = 40000, 0.9, -1, 2, "ce", "{}"
    prune_type, slim_lambda, dataset, input_size, random_seed = "dcfp", 0.0, None, "129,129", 12345


class _Data:
    ignore_label, num_classes, class_weights = 255, 19, None

    def __init__(self):
        self.gen = torch.Generator().manual_seed(1)


def build(dev):
    torch.manual_seed(12345)
    m = networks.deeplabv3.Seg_Model(backbone="resnet101", backbone_para={"pretrained": False}, num_classes=19,
                                     align_corner=True, criterion=build_criterions("ce", _Data(), {}), deepsup=True)
    return m


def bench_state(dev, directory):
    data = _Data()
    m = build(dev)
    fp = train_state.fingerprint(_Args, m, 19, 1)
    m = m.to(dev).train()
    opt = build_optimizer(_Args, m)
    opt.zero_grad()
    scorer = pruners.dcfp_pruning(m, 0.999)
    x = torch.randn(2, 3, 129, 129, generator=data.gen).to(dev)
    lab = torch.randint(0, 19, (2, 129, 129), generator=data.gen).to(dev)
    m(x, lab, deepsup=True)["loss"].backward()
    scorer.step(m)
    opt.step()
    path = train_state.state_path(directory, 1)
    saves = []
    for _ in range(3):
        with train_state.Timer() as t:
            train_state.save(train_state.capture(1, m, opt, scorer, dev, data, fp), path)
        saves.append(t.seconds)
    size = os.path.getsize(path)
    restores = []
    for _ in range(3):
        m2 = build(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = train_state.load(path)
        train_state.restore_model(st, m2, fp)
        t1 = time.perf_counter()
        m2 = m2.to(dev).train()
        opt2 = build_optimizer(_Args, m2)
        opt2.zero_grad()
        sc2 = pruners.dcfp_pruning(m2, 0.999)
        with train_state.Timer() as t:
            train_state.restore_rest(st, opt2, sc2, dev, _Data())
        restores.append((t1 - t0) + t.seconds)
        del m2, opt2, sc2, st
    return {"state_file_MB": round(size / 1e6, 1), "save_s": [round(s, 3) for s in saves],
            "restore_s": [round(s, 3) for s in restores], "params": sum(p.numel() for p in m.parameters())}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--words", type=int, default=65 * 1000 * 1000)
    p.add_argument("--dir", type=str, default=None, help="where the state file is written (default: a temporary directory)")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("state_bench.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    out = {"digest": bench_digest(dev, args.words, args.reps)}
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        out["state"] = bench_state(dev, d)
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
