#!/usr/bin/env python
"""One optimizer step on the parameter shapes of DeepLabv3-R101 (65 M parameters in some hundred tensors), random
gradients, no model run:

  fused_sgd     FusedSGD.step()      one launch per param group + one weight-copy refresh launch
  fused_adamw   FusedAdamW.step()    one launch per param group + one weight-copy refresh launch
  torch_adamw   torch.optim.AdamW(foreach=True).step() - what `--optim adamw` ran before FusedAdamW - and, in the
                second phase, the permuted weight copy every conv then rebuilds for itself: one single-entry launch of
                the refresh kernel per conv and pass

Two phases per optimizer: "update" with no kept weight copies registered (the update kernels alone), then "step" after
a forward and a dgrad copy of every conv weight has been registered the way a training step registers them (at a
nominal 2 x Cin x 64 x 64 activation: the copy's size is the weight's, not the activation's).  bench.py's discipline:
warm-up steps, a synchronise, the wall clock around K steps ending in a synchronise; the median of the per-step device
events is printed beside it.  A bare loop of steps is paced by the host (a step's Python work is of the order of its
device time; in training it hides behind the backward pass), so each phase is also timed with the queue kept full:
a few large matrix products are enqueued first, the steps are queued behind them, and two device events bracket the
steps ("device" ms; `ahead` says that the host had queued every step before the first one started).  GB/s =
algorithmic bytes of the update (AdamW 28 B/element: p, g, m, v read, p, m, v written; SGD 20 B/element) over the
device time of the "update" phase.

Then gradient-norm clipping and the weight EMA, "update" phase only, device time with the queue
kept full:

  fused_sgd+clip, fused_adamw+clip           max_grad_norm set: the two norm launches, then the step launches
  fused_sgd+clip+ema, fused_adamw+clip+ema   ... and ema_decay set (8 B/element more in the step launch)
  grad_norm                                  the two norm launches alone (4 B/element), beside ops.state_digest_device
                                             over the same gradient arena (the read-only pass it is modelled on)
  torch_sgd+clip+ema, torch_adamw+clip+ema   clip_grad_norm_(foreach=True), the foreach optimizer, torch._foreach_lerp_"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch import nn  # noqa: E402
from dcfp_amd import _lib, networks, ops  # noqa: E402
from dcfp_amd.optimizer import FusedAdamW, FusedSGD  # noqa: E402

BYTES = {"fused_sgd": 20, "fused_adamw": 28, "torch_adamw": 28}


def model_layout(backbone):
    """[(shape, conv geometry or None, decays)] of every trainable parameter, from the model built on the CPU."""
    bb = {"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128, "pretrained": False}
    m = networks.deeplabv3.Seg_Model(backbone=backbone, backbone_para=bb, num_classes=19, align_corner=True, deepsup=True)
    geom = {}
    for mod in m.modules():
        if isinstance(mod, nn.Conv2d) and mod.groups == 1:
            geom[id(mod.weight)] = (mod.stride[0], mod.padding[0], mod.dilation[0])
    return [(tuple(p.shape), geom.get(id(p)), p.dim() > 1) for p in m.parameters() if p.requires_grad]


def make_params(layout, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    params = []
    for shape, _, _ in layout:
        p = nn.Parameter(torch.randn(shape, device=device, generator=g) * 0.05)
        p.grad = torch.randn(shape, device=device, generator=g) * 0.01
        params.append(p)
    groups = [{"params": [p for p, (_, _, decays) in zip(params, layout) if decays]},
              {"params": [p for p, (_, _, decays) in zip(params, layout) if not decays], "weight_decay": 0.0}]
    return params, groups


def register_copies(params, layout):
    """A forward and a dgrad kept copy for every conv weight the refresh kernel has a layout for; returns the
    single-entry tables (one per copy) of the on-demand rebuilds."""
    L = _lib.lib()
    recs = []
    for p, (shape, geom, _) in zip(params, layout):
        if geom is None:
            continue
        stride, pad, dil = geom
        d = ops._desc((2, shape[1], 64, 64), shape, stride, pad, dil)
        for which in (_lib.CONV_FWD, _lib.CONV_DGRAD):
            e = _lib.WpEntry()
            if L.dcfp_conv2d_workspace_is_scratch(C.byref(d), which) or L.dcfp_conv2d_wp_layout(C.byref(d), which, C.byref(e)) != 0:
                continue
            buf, _ = ops._conv_workspace(p, which, d)
            e.w, e.wp, e.first_block = p.data_ptr(), buf.data_ptr(), 0
            recs.append(e)
    arr = (_lib.WpEntry * len(recs))(*recs)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(params[0].device)
    return table, [int(e.n_blocks) for e in recs]


def on_demand_copies(table, blocks):
    """What every conv does for itself when nobody refreshed its copy: one launch per conv and pass."""
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    size = C.sizeof(_lib.WpEntry)
    for i, nb in enumerate(blocks):
        _lib.check(L.dcfp_conv2d_permute_weights_multi_f32(C.c_void_p(table.data_ptr() + i * size), 1, nb, stream),
                   "permute_weights")


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for k in range(steps):
        fn()
        marks[k + 1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    per = sorted(marks[k].elapsed_time(marks[k + 1]) for k in range(steps))
    median = per[len(per) // 2] if len(per) % 2 else 0.5 * (per[len(per) // 2 - 1] + per[len(per) // 2])
    return wall, median


def device_ms(fn, steps, busy):
    """Device time per call of `fn` with the queue kept full behind `busy()`; (ms, host stayed ahead)."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    busy()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    ahead = not e0.query()               # the device had not reached the first step when the last one was queued
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, ahead


def clip_ema_rows(result, layout, dev, args, busy):
    """The rows of the module docstring's second table.  max_grad_norm is small enough that the coefficient is < 1."""
    CLIP, DECAY = 1e-2, 0.999

    def torch_step(make):
        def build(groups):
            opt = make(groups)
            params = [p for g in groups for p in g["params"]]
            emas = [p.detach().clone() for p in params]

            def step():
                torch.nn.utils.clip_grad_norm_(params, CLIP, foreach=True)
                opt.step()
                torch._foreach_lerp_(emas, [p.detach() for p in params], 1.0 - DECAY)
            return opt, step
        return build

    def fused(make, **kw):
        def build(groups):
            opt = make(groups, **kw)
            return opt, opt.step
        return build
    sgd = lambda g, **kw: FusedSGD(g, lr=0.01, momentum=0.9, weight_decay=5e-4, **kw)          # noqa: E731
    adamw = lambda g, **kw: FusedAdamW(g, lr=1e-3, weight_decay=1e-2, **kw)                    # noqa: E731
    rows = {
        "fused_sgd+clip": (fused(sgd, max_grad_norm=CLIP), 24),
        "fused_sgd+clip+ema": (fused(sgd, max_grad_norm=CLIP, ema_decay=DECAY), 32),
        "fused_adamw+clip": (fused(adamw, max_grad_norm=CLIP), 32),
        "fused_adamw+clip+ema": (fused(adamw, max_grad_norm=CLIP, ema_decay=DECAY), 40),
        "torch_sgd+clip+ema": (torch_step(lambda g: torch.optim.SGD(g, lr=0.01, momentum=0.9, weight_decay=5e-4,
                                                                    foreach=True)), None),
        "torch_adamw+clip+ema": (torch_step(lambda g: torch.optim.AdamW(g, lr=1e-3, weight_decay=1e-2, foreach=True)),
                                 None),
    }
    numel = result["elements"]
    for seed, (name, (build, nbytes)) in enumerate(rows.items()):
        params, groups = make_params(layout, dev, 100 + seed)
        opt, step = build(groups)
        wall, med = timed(step, args.warmup, args.steps)
        dms, ahead = device_ms(step, args.device_steps, busy)
        row = {"update_ms": wall, "update_median_ms": med, "update_device_ms": dms, "ahead": bool(ahead),
               "bytes_per_element": nbytes, "table_rebuilds": getattr(opt, "table_rebuilds", None)}
        if nbytes:
            row["update_GBps"] = nbytes * numel / (dms * 1e-3) / 1e9
        if name == "fused_sgd+clip":              # the norm launches alone, and the digest of the same arena beside them
            row["grad_norm"] = float(opt.grad_norm())
            n_ms, n_ahead = device_ms(opt._clip, args.device_steps, busy)
            flat = opt.arena().flat_grad
            ops.state_digest_device(flat)
            d_ms, d_ahead = device_ms(lambda: ops.state_digest_device(flat), args.device_steps, busy)
            result["rows"]["grad_norm"] = {
                "device_ms": n_ms, "GBps": 4 * numel / (n_ms * 1e-3) / 1e9, "ahead": bool(n_ahead),
                "digest_device_ms": d_ms, "digest_GBps": 4 * flat.numel() / (d_ms * 1e-3) / 1e9,
                "digest_ahead": bool(d_ahead), "arena_elements": flat.numel()}
            print("%-22s device %.3f ms = %.0f GB/s over %.1f M elements | state digest of the gradient arena "
                  "(%.1f M elements) %.3f ms = %.0f GB/s" % ("grad_norm", n_ms, result["rows"]["grad_norm"]["GBps"],
                                                            numel / 1e6, flat.numel() / 1e6, d_ms,
                                                            result["rows"]["grad_norm"]["digest_GBps"]))
        result["rows"][name] = row
        print("%-22s update: loop %.3f ms (median %.3f), device %.3f ms%s%s"
              % (name, wall, med, dms, (" = %.0f GB/s at %d B/element" % (row["update_GBps"], nbytes)) if nbytes else "",
                 "" if ahead else "  [host did not stay ahead: device figures include host gaps]"))
        del opt, step, params, groups
        gc.collect()
        ops._WP_TABLE["version"] += 1
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="resnet101")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device-steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_bench.py needs a GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    layout = model_layout(args.backbone)
    numel = sum(int(torch.Size(s).numel()) for s, _, _ in layout)
    makers = {
        "fused_sgd": lambda g: FusedSGD(g, lr=0.01, momentum=0.9, weight_decay=5e-4),
        "fused_adamw": lambda g: FusedAdamW(g, lr=1e-3, weight_decay=1e-2),
        "torch_adamw": lambda g: torch.optim.AdamW(g, lr=1e-3, weight_decay=1e-2, foreach=True),
    }
    result = {"tool": "optim_bench", "backbone": args.backbone, "tensors": len(layout), "elements": numel,
              "steps": args.steps, "warmup": args.warmup, "rows": {}}
    print("%d tensors, %.1f M elements; AdamW moves %.2f GB per step" % (len(layout), numel / 1e6, 28 * numel / 1e9))
    a = torch.randn(8192, 8192, device=dev)

    def busy():                                  # ~0.1 s of device work for the host to queue steps behind
        for _ in range(16):
            torch.mm(a, a)
    busy()
    for seed, (name, make) in enumerate(makers.items()):
        params, groups = make_params(layout, dev, seed)
        opt = make(groups)
        wall_u, med_u = timed(opt.step, args.warmup, args.steps)            # no kept copies yet: the update alone
        dev_u, ahead_u = device_ms(opt.step, args.device_steps, busy)
        table, blocks = register_copies(params, layout)
        if name == "torch_adamw":
            def step():
                opt.step()
                on_demand_copies(table, blocks)
        else:
            step = opt.step
        wall_s, med_s = timed(step, args.warmup, args.steps)
        dev_s, ahead_s = device_ms(step, args.device_steps, busy)
        gbs = BYTES[name] * numel / (dev_u * 1e-3) / 1e9
        row = {"update_ms": wall_u, "update_median_ms": med_u, "update_device_ms": dev_u, "update_GBps": gbs,
               "bytes_per_element": BYTES[name], "step_ms": wall_s, "step_median_ms": med_s, "step_device_ms": dev_s,
               "ahead": bool(ahead_u and ahead_s), "kept_copies": len(blocks),
               "table_rebuilds": getattr(opt, "table_rebuilds", None)}
        result["rows"][name] = row
        print("%-12s update: loop %.3f ms (median %.3f), device %.3f ms = %.0f GB/s at %d B/element | with %d kept weight "
              "copies, step: loop %.3f ms (median %.3f), device %.3f ms%s"
              % (name, wall_u, med_u, dev_u, gbs, BYTES[name], len(blocks), wall_s, med_s, dev_s,
                 "" if row["ahead"] else "  [host did not stay ahead: device figures include host gaps]"))
        del opt, params, groups, table, step
        gc.collect()
        ops._WP_TABLE["version"] += 1
        torch.cuda.empty_cache()
    clip_ema_rows(result, layout, dev, args, busy)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
