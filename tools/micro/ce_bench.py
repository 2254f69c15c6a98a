"""Times of the fused upsample+CE forward and backward, separately, at one shape (default: the bench shape
4x19x128x256 -> 1024x2048, align_corners, unweighted), and the kernel the backward takes (ops.ce_backward_plan).

    python tools/micro/ce_bench.py --classes 171 --batch 2 --lowres 64,64 --size 512,512 --align 0 --weighted 1

Each figure is the median of --repeats windows of --iters calls between two device events (min and max beside it: the
run-to-run spread of this process).  DCFP_CE_BWD_CELLS=0 in the environment times the per-output kernels."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def get_parser():
    pair = lambda s: tuple(int(v) for v in s.split(","))
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--classes", type=int, default=19)
    p.add_argument("--batch", type=int, default=4)
    p.add_argument("--lowres", type=pair, default=(128, 256), help="h,w of the logits")
    p.add_argument("--size", type=pair, default=(1024, 2048), help="H,W of the labels")
    p.add_argument("--align", type=int, default=1, help="align_corners")
    p.add_argument("--weighted", type=int, default=0, help="1: the per-pixel-weighted CE of the GSRL loss")
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--repeats", type=int, default=5)
    return p


def timed(fn, iters, repeats):
    """-> (median, min, max) ms per call over `repeats` windows of `iters` calls"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main(argv=None):
    from dcfp_amd import _lib, ops
    a = get_parser().parse_args(argv)
    dev = torch.device("cuda:0")
    N, Cc, (h, w), (H, W), align = a.batch, a.classes, a.lowres, a.size, int(bool(a.align))
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(N, Cc, h, w, generator=g) * 2).to(dev)
    lab = torch.randint(0, Cc, (N, H, W), generator=g)
    lab[torch.rand(N, H, W, generator=g) < 0.05] = 255
    lab = lab.to(dev)
    L = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lse = torch.empty((N, H, W), dtype=torch.float32, device=dev)
    dl = torch.empty_like(z)
    if a.weighted:
        pw = (torch.rand(N, H, W, generator=g) * 2).to(dev)
        pw[lab == 255] = 0.0
        ws = torch.empty(L.dcfp_upsample_wce_workspace_bytes(N, H, W), dtype=torch.uint8, device=dev)
        out = torch.empty((N, 2), dtype=torch.float32, device=dev)
        gs = torch.full((N,), 1e-4, dtype=torch.float32, device=dev)

        def fwd():
            _lib.check(L.dcfp_upsample_wce_fwd_f32(p(z), p(lab), p(pw), 255, N, Cc, h, w, H, W, align, p(lse), p(out),
                                                   p(ws), ws.numel(), st()), "wce_fwd")

        def bwd():
            _lib.check(L.dcfp_upsample_wce_bwd_f32(p(z), p(lab), p(pw), 255, N, Cc, h, w, H, W, align, p(lse), p(gs),
                                                   p(dl), st()), "wce_bwd")
    else:
        ws = torch.empty(L.dcfp_upsample_ce_workspace_bytes(N, H, W), dtype=torch.uint8, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        gs = torch.full((1,), 1e-6, dtype=torch.float32, device=dev)

        def fwd():
            _lib.check(L.dcfp_upsample_ce_fwd_f32(p(z), p(lab), None, 255, N, Cc, h, w, H, W, align, p(lse), None,
                                                  p(out), p(ws), ws.numel(), st()), "ce_fwd")

        def bwd():
            _lib.check(L.dcfp_upsample_ce_bwd_f32(p(z), p(lab), None, 255, N, Cc, h, w, H, W, align, p(lse), p(gs),
                                                  p(dl), st()), "ce_bwd")
    plan = ops.ce_backward_plan(N, Cc, h, w, H, W)
    tf = timed(fwd, a.iters, a.repeats)
    tb = timed(bwd, a.iters, a.repeats)
    shape = "%dx%dx%dx%d -> %dx%d align %d %s" % (N, Cc, h, w, H, W, align, "weighted" if a.weighted else "plain")
    print("upsample+CE %s: plan %s chunk_width %d chunks %d" % ((shape,) + plan))
    print("upsample+CE fwd ms %.4f (min %.4f max %.4f)" % tf)
    print("upsample+CE bwd ms %.4f (min %.4f max %.4f)" % tb)
    print("upsample+CE fwd+bwd ms %.4f" % (tf[0] + tb[0]))
    print("CE_BENCH " + json.dumps({"N": N, "C": Cc, "h": h, "w": w, "H": H, "W": W, "align": align,
                                    "weighted": int(bool(a.weighted)), "plan": list(plan), "fwd_ms": tf, "bwd_ms": tb,
                                    "checksum": float(dl.double().abs().sum())}))


if __name__ == "__main__":
    main()
