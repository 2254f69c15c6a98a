#!/usr/bin/env python
"""Times the pair-wise similarity distillation (ops.pairwise_kd_loss, dcfp_amd/csrc/pairwise.hip) against
the same formula written with torch ops, at the backbone output of two recipes:

    8 x 2048 x 97 x 97    769 x 769 crops, pool 2 and 4  (P = 2401 / 625 nodes)
    4 x 2048 x 129 x 257  1025 x 2049 crops, pool 4      (P = 2145)

Per (shape, pool), in one process, the variants taking turns round by round after a warm-up, by device events around
`--reps` back-to-back calls:

    hip      forward + backward of ops.pairwise_kd_loss through autograd, fp32 NCHW teacher
    hip_f16  the same with the teacher as the engine holds it: fp16 NHWC
    torch    forward + backward of the formula in torch ops (avg_pool2d, normalisation, bmm and their autograd)
    abi      dcfp_pairwise_fwd_f32 + dcfp_pairwise_bwd_f32 alone (loss and gradient, their ten launches) through ctypes

Peak memory: torch.cuda.max_memory_allocated over one forward + backward of `hip` and of `torch`, above what is
allocated before the call (the inputs); the op's workspace belongs to the graph and is allocated inside that window.

Rate: the MFMA FLOPs the kernels execute - the two Grams over the upper triangle of 128-node tiles and the gradient
GEMM, on the padded sizes - over the `abi` time, as a share of the 157.3 TF fp32 matrix peak.  `abi` also holds the
node, dot, scatter and final launches, so this is a lower bound on the matrix kernels' own rate; for those alone run
this tool under `rocprofv3 --kernel-trace --stats`.

`--step-time` instead times whole training steps as DESIGN §16 does: tools/train.py --log-time True as a child process,
the slim DeepLabv3-R101 of tools/data/channel_cfg_r101_p60_synthetic.pth against the dense R101 (random weights) as an
fp16 engine teacher, 8 x 769 x 769 synthetic batches, once per --loss-type, median of the last steps.
One JSON line per measurement.  No GPU: an error, not a CPU timing."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from dcfp_amd import _lib, ops  # noqa: E402

CASES = [((8, 2048, 97, 97), 2), ((8, 2048, 97, 97), 4), ((4, 2048, 129, 257), 4)]
F32_MATRIX_PEAK = 157.3e12


def torch_pa(s, t, pool):
    def gram(x):
        u = F.avg_pool2d(x, pool, pool, ceil_mode=True, count_include_pad=False).flatten(2)
        r2 = (u * u).sum(dim=1, keepdim=True)
        f = u * torch.where(r2 > 1e-12, torch.rsqrt(r2.clamp_min(1e-30)), torch.zeros_like(r2))
        return torch.bmm(f.transpose(1, 2), f)
    d = gram(s) - gram(t)
    return (d * d).mean()


def mfma_flops(N, Cs, Ct, h, w, pool):
    P = -(-h // pool) * -(-w // pool)
    Pp = -(-P // 128) * 128
    nt = Pp // 128
    cs, ct = -(-Cs // 32) * 32, -(-Ct // 32) * 32
    gram = nt * (nt + 1) // 2 * 128 * 128 * 2 * (cs + ct)
    grad = -(-cs // 128) * 128 * Pp * Pp * 2
    return N * (gram + grad), P


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # microseconds per call


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench_op(args):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    for shape, pool in CASES:
        N, Cc, h, w = shape
        g = torch.Generator().manual_seed(sum(shape) + pool)
        s = torch.relu(torch.randn(*shape, generator=g)).to(dev).requires_grad_(True)
        t = torch.relu(torch.randn(*shape, generator=g)).to(dev)
        t16 = t.permute(0, 2, 3, 1).contiguous().half()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def hip():
            s.grad = None
            ops.pairwise_kd_loss(s, t, pool).backward()

        def hip_f16():
            s.grad = None
            ops.pairwise_kd_loss(s, t16, pool).backward()

        def eager():
            s.grad = None
            torch_pa(s, t, pool).backward()

        peak_hip = peak_of(hip)
        s.grad = None
        peak_torch = peak_of(eager)
        s.grad = None
        nbytes = L.dcfp_pairwise_workspace_bytes(N, Cc, Cc, h, w, pool, 1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out, ds = torch.empty(1, device=dev), torch.empty_like(s)

        def abi():
            _lib.check(L.dcfp_pairwise_fwd_f32(C.c_void_p(s.data_ptr()), C.c_void_p(t.data_ptr()), ops.PA_F32_NCHW, 0, N,
                                               Cc, Cc, h, w, pool, C.c_void_p(ws.data_ptr()), ws.numel(),
                                               C.c_void_p(out.data_ptr()), 1, stream), "pairwise_fwd")
            _lib.check(L.dcfp_pairwise_bwd_f32(N, Cc, Cc, h, w, pool, C.c_void_p(ws.data_ptr()), ws.numel(), None,
                                               C.c_void_p(ds.data_ptr()), stream), "pairwise_bwd")

        variants = {"hip": hip, "hip_f16": hip_f16, "torch": eager, "abi": abi}
        for _ in range(args.warmup):
            for fn in variants.values():
                timed(fn, args.reps)
        hip()
        mine, mine_g = ops.pairwise_kd_loss(s, t, pool).item(), s.grad.clone()
        eager()
        agree = {"loss_rel": abs(mine - torch_pa(s, t, pool).item()) / max(1.0, abs(mine)),
                 "grad_nrel": float((mine_g - s.grad).norm() / s.grad.norm())}
        del mine_g
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn, args.reps))
        flops, P = mfma_flops(N, Cc, Cc, h, w, pool)
        rec = {"shape": list(shape), "pool": pool, "nodes": P, "rounds": args.rounds, "reps": args.reps,
               "mfma_gflop": round(flops / 1e9, 1), "workspace_MB": round(nbytes / 1e6, 1)}
        for k, v in times.items():
            rec[k + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1)}
        rec["torch_over_hip"] = round(rec["torch_us"]["median"] / rec["hip_us"]["median"], 2)
        rec["peak_MB"] = {"hip": round(peak_hip / 1e6, 1), "torch": round(peak_torch / 1e6, 1)}
        rate = flops / (rec["abi_us"]["median"] * 1e-6)
        rec["abi_TF"] = round(rate / 1e12, 1)
        rec["matrix_peak_fraction"] = round(rate / F32_MATRIX_PEAK, 3)
        rec["hip_vs_torch"] = agree
        print(json.dumps(rec), flush=True)
        del s, t, t16, ws, ds
        torch.cuda.empty_cache()


def bench_step(args):
    from dcfp_amd import networks
    with tempfile.TemporaryDirectory() as tmp:
        torch.manual_seed(0)
        dense = networks.deeplabv3.Seg_Model(backbone="resnet101", backbone_para={"pretrained": False}, num_classes=19,
                                             align_corner=True, criterion=None, deepsup=True)
        ckpt = os.path.join(tmp, "dense.pth")
        torch.save(dense.state_dict(), ckpt)
        del dense
        cfg = os.path.join(ROOT, "tools", "data", "channel_cfg_r101_p60_synthetic.pth")
        for loss_type in args.loss_types.split(";"):
            cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--ddp", "False", "--backbone", "resnet101",
                   "--loss-type", loss_type, "--channel-cfg", cfg, "--num-steps", str(args.steps), "--batch-size", "8",
                   "--input-size", "769,769", "--log-time", "True", "--snapshot-dir", os.path.join(tmp, "snap"),
                   "--save-steps", str(10 ** 9), "--save-pred-every", str(10 ** 9)]
            if any(k in loss_type.split(",") for k in ("kd", "kdpa")):
                cmd += ["--teacher-from", ckpt]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=args.step_timeout)
            if r.returncode != 0:
                raise SystemExit(f"pa_bench: train.py --loss-type {loss_type} failed\n{r.stderr[-3000:]}")
            ms = [float(l.split("step")[1].split("ms")[0]) for l in r.stdout.splitlines() if l.strip().startswith("step ")]
            tail = ms[-args.last:]
            print(json.dumps({"loss_type": loss_type, "steps": len(ms), "median_ms_last": round(statistics.median(tail), 1),
                              "min_ms_last": round(min(tail), 1), "max_ms_last": round(max(tail), 1)}), flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--step-time", action="store_true")
    p.add_argument("--loss-types", type=str, default="gsrl;gsrl,kdpa")
    p.add_argument("--steps", type=int, default=14)
    p.add_argument("--last", type=int, default=8)
    p.add_argument("--step-timeout", type=int, default=500)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pa_bench: needs the GPU (a CPU run says nothing about the kernels)")
    if args.step_time:
        bench_step(args)
    else:
        bench_op(args)


if __name__ == "__main__":
    main()
