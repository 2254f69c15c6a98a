#!/usr/bin/env python
"""Times the Lovasz-Softmax loss (ops.lovasz_softmax, dcfp_amd/csrc/lovasz.hip) against the sort-based
formula of the paper written with torch ops, at the main head's logits of three recipes:

    8 x 19 x 97 x 97    -> 769 x 769    Cityscapes crops of the fine-tune stage
    8 x 59 x 61 x 61    -> 481 x 481    Pascal-Context
    8 x 171 x 65 x 65   -> 513 x 513    COCO-Stuff

Labels are the prediction's argmax at 60 % of the pixels, a random class elsewhere, 10 % ignored.  Per shape, in one
process, the variants interleaved round by round after a warm-up, by device events around `--reps` back-to-back calls
(the protocol of tools/kd_bench.py):

    hip      forward + backward of ops.lovasz_softmax through autograd
    torch    forward + backward of the sort formula in torch ops: F.interpolate, softmax, one descending sort of the
             [C, valid pixels] errors, gather, cumsum - it materialises the N x C x H x W probabilities
    hist / scan / bwd   the three C entries alone (dcfp_lovasz_hist_f32, _scan_f32, _bwd_f32) through ctypes: an upper
             bound on their kernels; for the kernels alone run this tool under `rocprofv3 --kernel-trace --stats`

`peak_bytes` is torch.cuda.max_memory_allocated over one forward + backward above what was allocated before it.
`hist_bytes` = 12 N H W - the labels read and the log-sum-exp written once, the logits being cache resident - and
`hist_TB_per_s` is that over the `hist` time.  `loss_gap` = torch - hip (the bound is [-2^-21, 1/bins + 2^-21] plus fp32
rounding), `grad_nrel` the norm-relative distance of the two gradients.  One JSON line per shape.  No GPU: an error."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dcfp_amd import _lib, ops  # noqa: E402

SHAPES = [((8, 19, 97, 97), (769, 769)), ((8, 59, 61, 61), (481, 481)), ((8, 171, 65, 65), (513, 513))]
IGNORE = 255


def torch_lovasz(logits, labels, size, align_corners, ignore_index):
    p = torch.softmax(F.interpolate(logits, size=size, mode="bilinear", align_corners=align_corners), dim=1)
    Cc = p.shape[1]
    valid = (labels >= 0) & (labels < Cc) & (labels != ignore_index)
    pv = p.permute(1, 0, 2, 3)[:, valid]                                         # [C, M]
    fg = (labels[valid].unsqueeze(0) == torch.arange(Cc, device=p.device).unsqueeze(1)).to(p.dtype)
    es, order = torch.sort((fg - pv).abs(), dim=1, descending=True)
    fs = torch.gather(fg, 1, order)
    G = fg.sum(1, keepdim=True)
    jac = 1 - (G - fs.cumsum(1)) / (G + (1 - fs).cumsum(1))
    grad = torch.cat([jac[:, :1], jac[:, 1:] - jac[:, :-1]], dim=1)
    present = (G[:, 0] > 0).to(p.dtype)
    return ((es * grad).sum(1) * present).sum() / present.sum().clamp(min=1)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # microseconds per call


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--shapes", type=str, default="0,1,2", help="indices into the three recipe shapes")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lovasz_bench: needs the GPU (a CPU run says nothing about the kernels)")
    dev = torch.device("cuda:0")
    L, B = _lib.lib(), args.bins
    p = lambda t: C.c_void_p(t.data_ptr())
    for k in (int(v) for v in args.shapes.split(",")):
        shape, size = SHAPES[k]
        N, Cc, h, w = shape
        H, W = size
        g = torch.Generator().manual_seed(sum(shape))
        x = (torch.randn(*shape, generator=g) * 3.0).to(dev).requires_grad_(True)
        with torch.no_grad():
            pred = F.interpolate(x, size=size, mode="bilinear", align_corners=True).argmax(1)
        lab = torch.randint(0, Cc, (N, H, W), generator=g).to(dev)
        take = (torch.rand(N, H, W, generator=g) < 0.6).to(dev)
        lab[take] = pred[take]
        lab[(torch.rand(N, H, W, generator=g) < 0.1).to(dev)] = IGNORE
        del pred, take
        ws = torch.empty(L.dcfp_lovasz_workspace_bytes(Cc, B), dtype=torch.uint8, device=dev)
        lse, asum = torch.empty(N, H, W, device=dev), torch.empty(N, H, W, device=dev)
        out, one = torch.empty(1, device=dev), torch.ones(1, device=dev)
        table, dl = torch.empty(Cc, B, 2, device=dev), torch.empty(shape, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        xd = x.detach()

        def hip():
            x.grad = None
            ops.lovasz_softmax(x, lab, size, True, IGNORE, B).backward()

        def eager():
            x.grad = None
            torch_lovasz(x, lab, size, True, IGNORE).backward()

        def hist():
            _lib.check(L.dcfp_lovasz_hist_f32(p(xd), p(lab), IGNORE, N, Cc, h, w, H, W, 1, B, p(lse), p(ws), ws.numel(),
                                              stream), "lovasz_hist")

        def scan():
            _lib.check(L.dcfp_lovasz_scan_f32(Cc, B, p(ws), ws.numel(), p(out), p(table), stream), "lovasz_scan")

        def bwd():
            _lib.check(L.dcfp_lovasz_bwd_f32(p(xd), p(lab), IGNORE, N, Cc, h, w, H, W, 1, B, p(lse), p(table), p(one),
                                             p(asum), p(dl), stream), "lovasz_bwd")

        variants = {"hip": hip, "torch": eager, "hist": hist, "scan": scan, "bwd": bwd}
        for _ in range(args.warmup):
            for fn in variants.values():
                timed(fn, args.reps)
        hip()
        mine, mine_g = ops.lovasz_softmax(x, lab, size, True, IGNORE, B).item(), x.grad.clone()
        eager()
        agree = {"loss_gap": torch_lovasz(x, lab, size, True, IGNORE).item() - mine,
                 "grad_nrel": float((mine_g - x.grad).norm() / x.grad.norm())}
        del mine_g
        x.grad = None
        mem = {"hip": peak(hip), "torch": peak(eager)}
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                times[name].append(timed(fn, args.reps))
        rec = {"shape": list(shape), "size": list(size), "bins": B, "rounds": args.rounds, "reps": args.reps}
        for name, v in times.items():
            rec[name + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1),
                                 "max": round(max(v), 1)}
        rec["torch_over_hip"] = round(rec["torch_us"]["median"] / rec["hip_us"]["median"], 2)
        rec["peak_bytes"] = mem
        rec["probabilities_bytes"] = 4 * N * Cc * H * W
        rec["hist_bytes"] = 12 * N * H * W
        rec["hist_TB_per_s"] = round(rec["hist_bytes"] / (rec["hist_us"]["median"] * 1e-6) / 1e12, 3)
        rec["hip_vs_torch"] = agree
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
