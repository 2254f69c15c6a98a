#!/usr/bin/env python
"""Times the kernels of the baseline pruning criteria (csrc/score.hip) at the shapes of DeepLabv3-R101 with
19 classes, each against the same formula written with torch ops on the same GPU:

    gate_taylor    pruners.taylor_pruning(mode="gate").step           torch: per layer  s += (gamma*gg + beta*gb)**2
    gate_l1reg     pruners.slimming_regularizer.step                  torch: per layer  gg.add_(sign(gamma), alpha=lam)
    abs_sum, l2    one dcfp_filter_reduce_f32 launch over all convs   torch: per layer  w.abs().sum(1), (w*w).sum(1).sqrt()
    dot_sq_acc     the per-step launch of --prune-type taylor_w       torch: per layer  s += (w*g).sum(1)**2
    fpgm           the two launches of dcfp_fpgm_f32                  torch: per layer  torch.cdist(w, w).sum(1)

The model is built on the device with its random initial weights; the gradients are random tensors (no backward runs:
the kernels' time does not depend on the values).  Protocol: device events around `--calls` back-to-back calls after
`--warmup` calls (10 and 50 by default), per variant; the time is per call and includes the host's enqueue cost
wherever the device finishes first (the per-layer torch loops are ~100 to ~300 launches per call: largely that).  For
the gate kernels `hip_us` is the whole `step` - a walk over the modules and their pointers on the host, then one launch
of a few microseconds - and `abi_us` the launch alone through ctypes.

filter_reduce is also set against a float4 copy: `copy_us` is torch's copy of a flat fp32 buffer as large as what the
kernel reads, timed in the same run the same way.  The copy moves twice its size (read + write), the kernel its reads
plus 4 bytes per row, so the rates compare, not the times: `share_of_copy_rate` = (kernel bytes / kernel time) /
(2 * buffer bytes / copy time).  The R101 weights (~0.24 GB, twice that with gradients) are at or above the 256 MB
Infinity Cache, so the rates are close to HBM rates but not HBM readings.  One JSON line per kernel.  No GPU: an
error, not a CPU timing."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dcfp_amd import _lib, networks, pruners  # noqa: E402
from dcfp_amd.pruners import baseline_pruner as bp  # noqa: E402


def timed(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--backbone", type=str, default="resnet101")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("score_bench: needs the GPU (a CPU run says nothing about the kernels)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = networks.deeplabv3.Seg_Model(backbone=args.backbone, backbone_para={"pretrained": False}, num_classes=19,
                                         align_corner=True, criterion=None, deepsup=True).to(dev)
    names = bp.scored_bn_names(model)
    mods = dict(model.named_modules())
    convs = bp.linked_convs(model, names)
    for n in names:
        for prm in (mods[n].weight, mods[n].bias, mods[convs[n]].weight):
            prm.grad = torch.randn_like(prm) * 1e-3
    bns = [mods[n] for n in names]
    ws = [mods[convs[n]].weight.detach() for n in names]
    gs = [mods[convs[n]].weight.grad for n in names]
    w2 = [w.flatten(1) for w in ws]
    g2 = [g.flatten(1) for g in gs]
    channels = sum(b.weight.numel() for b in bns)
    wbytes = 4 * sum(w.numel() for w in ws)
    shape = {"model": "deeplabv3-" + args.backbone, "layers": len(names), "channels": channels, "weight_bytes": wbytes}
    lam = 1e-4

    def report(name, hip_us, torch_us, **extra):
        rec = dict(kernel=name, hip_us=round(hip_us, 2), torch_us=round(torch_us, 2),
                   torch_over_hip=round(torch_us / hip_us, 2), warmup=args.warmup, calls=args.calls, **shape, **extra)
        print(json.dumps(rec), flush=True)

    # ---- gate kernels
    tp = pruners.taylor_pruning(model, "gate")
    sums = [torch.zeros_like(b.weight) for b in bns]

    def torch_taylor():
        for s, b in zip(sums, bns):
            s += (b.weight * b.weight.grad + b.bias * b.bias.grad) ** 2
    L, stream = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def abi(fn, table, *more):
        """the launch alone through ctypes: what is left of `step` without its walk over the modules and their pointers"""
        ptr = C.c_void_p(table.data_ptr())
        return round(timed(lambda: _lib.check(fn(ptr, len(names), *more, stream), "gate"), args.warmup, args.calls), 2)
    with torch.no_grad():
        report("gate_taylor", timed(lambda: tp.step(model), args.warmup, args.calls),
               timed(torch_taylor, args.warmup, args.calls), bytes=5 * 4 * channels,
               abi_us=abi(L.dcfp_gate_taylor_f32, tp._table))
        reg = pruners.slimming_regularizer(model, lam)

        def torch_l1():
            for b in bns:
                b.weight.grad.add_(torch.sign(b.weight), alpha=lam)
        report("gate_l1reg", timed(lambda: reg.step(model), args.warmup, args.calls),
               timed(torch_l1, args.warmup, args.calls), bytes=3 * 4 * channels,
               abi_us=abi(L.dcfp_gate_l1reg_f32, reg._table, lam))

        # ---- filter_reduce, and the copy of the same bytes
        outs = [torch.zeros(w.shape[0], device=dev) for w in ws]
        acc = [torch.zeros(w.shape[0], device=dev) for w in ws]
        table_w = bp.filter_reduce_table([(w, None, o) for w, o in zip(ws, outs)])
        table_wg = bp.filter_reduce_table([(w, g, o) for w, g, o in zip(ws, gs, outs)])
        src1, dst1 = torch.empty(wbytes // 4, device=dev), torch.empty(wbytes // 4, device=dev)
        src2, dst2 = torch.empty(wbytes // 2, device=dev), torch.empty(wbytes // 2, device=dev)
        copy1 = timed(lambda: dst1.copy_(src1), args.warmup, args.calls)
        copy2 = timed(lambda: dst2.copy_(src2), args.warmup, args.calls)

        def torch_abs():
            for o, w in zip(acc, w2):
                torch.sum(w.abs(), 1, out=o)

        def torch_l2():
            for o, w in zip(acc, w2):
                o.copy_((w * w).sum(1).sqrt())

        def torch_dot():
            for o, w, g in zip(acc, w2, g2):
                o += (w * g).sum(1) ** 2
        for name, op, table, ref, read, copy_us in (
                ("filter_abs_sum", _lib.FILTER_ABS_SUM, table_w, torch_abs, wbytes, copy1),
                ("filter_l2", _lib.FILTER_L2, table_w, torch_l2, wbytes, copy1),
                ("filter_dot_sq_acc", _lib.FILTER_DOT_SQ_ACC, table_wg, torch_dot, 2 * wbytes, copy2)):
            hip_us = timed(lambda: bp.filter_reduce(*table, op), args.warmup, args.calls)
            kbytes = read + 4 * channels * (2 if op == _lib.FILTER_DOT_SQ_ACC else 1)
            rate, copy_rate = kbytes / (hip_us * 1e-6), 2 * read / (copy_us * 1e-6)
            report(name, hip_us, timed(ref, args.warmup, args.calls), bytes=kbytes, units=table[2],
                   TB_per_s=round(rate / 1e12, 3), copy_us=round(copy_us, 2), copy_TB_per_s=round(copy_rate / 1e12, 3),
                   share_of_copy_rate=round(rate / copy_rate, 3))

        # ---- fpgm
        plan = bp.fpgm_table(list(zip(ws, outs)))

        def hip_fpgm():
            bp.fpgm(*plan)

        def torch_fpgm():
            for o, w in zip(acc, w2):
                o.copy_(torch.cdist(w, w).sum(1))
        pair_elems = sum(w.shape[0] ** 2 * w.shape[1] for w in w2)
        hip_us = timed(hip_fpgm, args.warmup, args.calls)
        report("fpgm", hip_us, timed(torch_fpgm, args.warmup, args.calls), pair_elements=pair_elems,
               G_pair_elements_per_s=round(pair_elems / (hip_us * 1e-6) / 1e9, 1))


if __name__ == "__main__":
    main()
