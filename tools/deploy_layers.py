#!/usr/bin/env python
"""Per-layer-family kernel table of the fp16 engine or, with --precision fp8 (deeplabv3 and simple), of
the fp8 engine (§11a; the matrix peak is then the block-scaled e4m3 rate, 5 PF dense).  Two steps:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/deploy_layers.py --plan OUT/plan.json
  python tools/deploy_layers.py --report OUT --plan OUT/plan.json

The first runs the frozen model (--model, default deeplabv3) a few times under the profiler and writes the launch list of one call (one entry
per kernel launch, in order, with the FLOPs and the least bytes the layer needs, computed from its shapes).  The second
matches the trace's engine kernels to that list by launch order (the last --iters calls; median per launch) and prints,
per family: kernel time, achieved TF/s, the time at the fp16 matrix peak (2.5 PF dense) and at the measured HBM copy
rate (6.29 TB/s), and which of the two bounds the family."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F16, PEAK_F8, HBM = 2.5e15, 5.0e15, 6.29e12
ENGINE_KERNELS = re.compile(r"conv_f16_kernel|maxpool_nhwc_f16|avgpool_partial|avgpool_final|broadcast_nhwc_f16|"
                            r"nchw_f32_to_nhwc_f16|resize_bilinear_kernel|pyramid_partial|pyramid_final|"
                            r"conv_f8_kernel|cast_nhwc_f16_to_f8|maxpool_nhwc_f8|avgpool_f8_partial|avgpool_f8_final|"
                            r"broadcast_nhwc_f16_to_f8")


def family(name):
    m = re.match(r"backbone\.(layer\d)\.\d+\.(conv\d|downsample)", name)
    if m:
        return f"{m.group(1)} {m.group(2)}"
    if name.startswith("backbone.conv1") and not name.endswith(".cast"):
        return "stem 3x3"
    if re.match(r"aspp\.aspp[234]", name):
        return "aspp dilated 3x3"
    if name in ("last_conv.0", "last_conv.3"):
        return "head 3x3"
    if name == "last_conv.6":
        return "classifier (fp32 NCHW)"
    if name == "ppm.stages.pool":
        return "pyramid pool (4 levels, one sweep)"
    if re.match(r"ppm\.stages\.\d\.up", name):
        return "pyramid prior resizes"
    if re.match(r"ppm\.stages\.\d\.1", name):
        return "pyramid stage 1x1 (s x s maps)"
    if name == "ppm.bottleneck.0":
        return "pyramid bottleneck 3x3"
    if name == "decoder.up":
        return "decoder resize"
    if name == "decoder.conv1":
        return "decoder 1x1 (layer1 tap)"
    if name in ("decoder.last_conv.0", "decoder.last_conv.3"):
        return "decoder 3x3"
    if name in ("decoder.last_conv.6", "last_conv"):
        return "classifier (fp32 NCHW)"
    if name.startswith("aspp.global_avg_pool") or name == "backbone.maxpool" or name == "input" or name.endswith(".cast"):
        return "pools / convert / broadcast"
    return name


def launches(engine, N, H, W):
    """One entry per kernel launch of a call: (name, flops, least bytes)."""
    hw = engine.buffer_shapes(H, W)
    out = [("input", 0, N * H * W * (3 * 4 + 8 * 2))]
    es = lambda b: 1 if engine.buffer_fmt[b] == "f8" else 2     # noqa: E731  bytes per element of a buffer
    for r in engine.plan:
        h, w = hw[r["src"]]
        ho, wo = hw[r["dst"]]
        if r["op"] == "conv":
            e = es(r["src"])
            flops = 2 * N * ho * wo * r["cout"] * r["cin"] * r["k"] ** 2
            byts = e * (N * h * w * r["cin8"] // (r["stride"] ** 2 if r["k"] == 1 else 1)
                        + engine.tensors[r["w"]].numel()) + N * ho * wo * r["cout"] * (4 if r["f32"] else e)
            if r["res"] >= 0:
                byts += e * N * ho * wo * r["cout"]
            out.append((r["name"], flops, byts))
        elif r["op"] == "cast":
            out.append((r["name"], 0, 3 * N * h * w * r["c"]))
        elif r["op"] == "avgpool":
            out.append((r["name"], 0, es(r["src"]) * N * h * w * engine.buffers[r["src"]]))
            out.append((r["name"], 0, 0))
        elif r["op"] == "pyramid":                      # two launches: the sweep over the features, then the bins
            out.append((r["name"], 0, 2 * N * h * w * r["c8"]))
            out.append((r["name"], 0, 0))
        elif r["op"] == "resize":                       # store-bound: the bytes written
            out.append((r["name"], 0, 2 * engine.buffers[r["src"]] * N * ho * wo))
        else:
            c8, e = engine.buffers[r["src"]], es(r["dst"])
            out.append((r["name"], 0, e * c8 * N * (h * w + ho * wo) if r["op"] == "maxpool" else e * c8 * N * ho * wo))
    return out


def run(a):
    import torch
    from dcfp_amd import deploy, networks
    h, w = [int(v) for v in a.size.split(",")]
    bb = {"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128, "pretrained": False}
    m = getattr(networks, a.model).Seg_Model(backbone=a.backbone, backbone_para=bb, num_classes=19, align_corner=True,
                                             deepsup=False).eval()
    eng = deploy.build_engine(m).to("cuda:0")
    x = torch.randn(a.batch, 3, h, w, device="cuda:0")
    calib = 0
    if a.precision == "fp8":                  # (the calibration call's fp16 launches precede the fp8 engine's in the trace)
        calib = len(launches(eng, a.batch, h, w))
        eng = deploy.build_engine(m, precision="fp8", amax=deploy.calibrate(eng, [x])).to("cuda:0")
    for _ in range(3 + a.iters):
        eng.lowres_logits(x)
    torch.cuda.synchronize()
    with open(a.plan, "w") as f:
        json.dump({"iters": a.iters, "launches": launches(eng, a.batch, h, w),
                   "what": f"{a.model}-{a.backbone} {a.batch}x3x{h}x{w} {a.precision}", "precision": a.precision,
                   "calib_launches": calib}, f)


def report(a):
    plan = json.load(open(a.plan))
    L, iters = plan["launches"], plan["iters"]
    peak = PEAK_F8 if plan.get("precision") == "fp8" else PEAK_F16
    rows = []
    for path in glob.glob(os.path.join(a.report, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if ENGINE_KERNELS.search(r["Kernel_Name"]):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    assert len(rows) >= iters * len(L) and (len(rows) - plan.get("calib_launches", 0)) % len(L) == 0, (len(rows), len(L))
    rows = rows[-iters * len(L):]
    ns = [statistics.median(rows[c * len(L) + i][1] for c in range(iters)) for i in range(len(L))]
    fam = {}
    for (name, flops, byts), t in zip(L, ns):
        f = fam.setdefault(family(name), [0, 0.0, 0.0, 0.0])
        f[0] += 1; f[1] += t * 1e-9; f[2] += flops; f[3] += byts
    total = sum(f[1] for f in fam.values())
    print(f"{plan['what']}: {len(L)} launches, kernel time {total * 1e3:.2f} ms per call "
          f"(median of {iters} calls per launch)")
    print(f"{'family':30s} {'n':>3s} {'ms':>7s} {'GFLOP':>8s} {'TF/s':>7s} {'ms@' + ('5PF' if peak == PEAK_F8 else '2.5PF'):>9s} {'MB':>7s} {'ms@HBM':>7s} bound")
    for k, (n, t, fl, by) in fam.items():
        tp, tb = fl / peak, by / HBM
        print(f"{k:30s} {n:3d} {t * 1e3:7.3f} {fl / 1e9:8.1f} {fl / t / 1e12:7.1f} {tp * 1e3:9.3f} {by / 1e6:7.1f} "
              f"{tb * 1e3:7.3f} {'matrix' if tp > tb else 'HBM'} ({max(tp, tb) / t:.2f} of it)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="deeplabv3", choices=("simple", "deeplabv3", "deeplabv3p", "psp"))
    ap.add_argument("--backbone", default="resnet101")
    ap.add_argument("--size", default="1024,2048")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--precision", default="fp16", choices=("fp16", "fp8"))
    ap.add_argument("--plan", default="plan.json")
    ap.add_argument("--report", default=None, help="directory of the rocprofv3 output to read")
    a = ap.parse_args()
    (report if a.report else run)(a)


if __name__ == "__main__":
    main()
