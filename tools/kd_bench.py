#!/usr/bin/env python
"""Times the distillation losses (ops.kd_loss, dcfp_amd/csrc/kd.hip) against the same formula written with torch ops,
both modes, at the low-resolution logits of three recipes:

    4 x 19 x 129 x 257   Cityscapes, 1025 x 2049 crops (the flagship step)
    8 x 59 x 61 x 61     Pascal-Context, 481 x 481
    8 x 171 x 65 x 65    COCO-Stuff, 513 x 513

Per (shape, mode), in one process, the variants interleaved round by round after a warm-up, by device events around
`--reps` back-to-back calls (one call is tens of microseconds: a single one would time the event pair):

    hip    forward + backward of ops.kd_loss through autograd
    torch  forward + backward of the formula in torch ops (log_softmax, exp, mul, sum and their autograd)
    abi    dcfp_kd_fwd_f32 alone, loss and gradient in its two launches, called through ctypes

All three include the host's enqueue cost wherever the device finishes first; `abi` is the closest to device time a
run without a profiler gets, an upper bound on the two kernels.  For the kernels alone run this tool under
`rocprofv3 --kernel-trace --stats` (kd_pixel_reg_kernel, kd_pixel_stream_kernel, kd_channel_kernel, kd_final_kernel).

bytes = 3 * 4 * N*C*h*w: s and t read once, dlogits written once - what the algorithm needs.  `hbm_fraction` is that
over the `abi` time, as a share of 6.29 TB/s (the float4-copy rate measured on an MI355X; the data sheet says 8.0).
The shapes are 8 - 31 MB and live in the 256 MB Infinity Cache between calls, so this is a rate, not an HBM reading.
One JSON line per (shape, mode).  No GPU: an error, not a CPU timing."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dcfp_amd import _lib, ops  # noqa: E402

SHAPES = [(4, 19, 129, 257), (8, 59, 61, 61), (8, 171, 65, 65)]
HBM_MEASURED = 6.29e12


def torch_kd(s, t, T, mode):
    N, Cc, h, w = s.shape
    if mode == "pixel":
        ls, lt, count = torch.log_softmax(s / T, dim=1), torch.log_softmax(t / T, dim=1), N * h * w
    else:
        ls = torch.log_softmax(s.reshape(N, Cc, h * w) / T, dim=2)
        lt = torch.log_softmax(t.reshape(N, Cc, h * w) / T, dim=2)
        count = N * Cc
    return (lt.exp() * (lt - ls)).sum() * (T * T / count)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # microseconds per call


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--temperature", type=float, default=2.0)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("kd_bench: needs the GPU (a CPU run says nothing about the kernels)")
    dev = torch.device("cuda:0")
    L, T = _lib.lib(), args.temperature
    for shape in SHAPES:
        g = torch.Generator().manual_seed(sum(shape))
        s = (torch.randn(*shape, generator=g) * 2.5).to(dev).requires_grad_(True)
        t = (torch.randn(*shape, generator=g) * 2.5).to(dev)
        N, Cc, h, w = shape
        nbytes = 3 * 4 * N * Cc * h * w
        for mode in ("pixel", "channel"):
            ws = torch.empty(max(L.dcfp_kd_workspace_bytes(ops.KD_MODES[mode], N, Cc, h, w), 256), dtype=torch.uint8,
                             device=dev)
            out, dl = torch.empty(1, device=dev), torch.empty_like(s)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def hip():
                s.grad = None
                ops.kd_loss(s, t, T, mode).backward()

            def eager():
                s.grad = None
                torch_kd(s, t, T, mode).backward()

            def abi():
                _lib.check(L.dcfp_kd_fwd_f32(C.c_void_p(s.data_ptr()), C.c_void_p(t.data_ptr()), ops.KD_MODES[mode], N,
                                             Cc, h, w, T, C.c_void_p(ws.data_ptr()), ws.numel(),
                                             C.c_void_p(out.data_ptr()), C.c_void_p(dl.data_ptr()), stream), "kd_fwd")

            variants = {"hip": hip, "torch": eager, "abi": abi}
            for _ in range(args.warmup):
                for fn in variants.values():
                    timed(fn, args.reps)
            hip()
            mine, mine_g = ops.kd_loss(s, t, T, mode).item(), s.grad.clone()
            eager()
            agree = {"loss_rel": abs(mine - torch_kd(s, t, T, mode).item()) / max(1.0, abs(mine)),
                     "grad_nrel": float((mine_g - s.grad).norm() / s.grad.norm())}
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    times[k].append(timed(fn, args.reps))
            rec = {"shape": list(shape), "mode": mode, "T": T, "rounds": args.rounds, "reps": args.reps, "bytes": nbytes}
            for k, v in times.items():
                rec[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2)}
            rec["torch_over_hip"] = round(rec["torch_us"]["median"] / rec["hip_us"]["median"], 2)
            rate = nbytes / (rec["abi_us"]["median"] * 1e-6)
            rec["abi_TB_per_s"] = round(rate / 1e12, 3)
            rec["hbm_fraction"] = round(rate / HBM_MEASURED, 3)
            rec["hip_vs_torch"] = agree
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
