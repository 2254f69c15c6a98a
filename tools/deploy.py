#!/usr/bin/env python
"""Deployment driver — the command line and protocol of the reference's totrt.py (scripts/cs/trt.sh): build the
(optionally slimmed) model, freeze it into an fp16 engine (dcfp_amd/deploy.py) - or, with --precision fp8, calibrate that engine on
--calib-batches batches and build the e4m3 engine - save the engine, reload it, and time
it as totrt.benchmark does: 10 warm-up calls, 50 timed calls, each timed call synchronised; prints the average batch
time.  Without --restore-from the model keeps its initial weights (synthetic, as tools/train.py starts from).

--save-flat PATH also writes the engine as a flat engine file, what dcfp_engine_open and
tools/engine_run.cpp load.  --runtime c times deploy.CEngine - the same plan launched by the library's C runtime - in the
same run with the same protocol and prints three lines: the Python engine, the C runtime on the same fp32 batch, and the C
runtime on a uint8 frame with the host -> device copy of the frame included; then the uint8 input kernel's own time
(device events around a chain of launches) next to its byte bound, 3 B read + 2 * 8 B written per pixel at the measured
float4-copy rate of an MI355X."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dcfp_amd import deploy, networks  # noqa: E402
from dcfp_amd.pruners import init_pruned_model  # noqa: E402
from dcfp_amd.utils.pyt_utils import load_model  # noqa: E402


def str2bool(v):
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def get_parser():
    p = argparse.ArgumentParser(description="DCFP")
    p.add_argument("--input-size", type=str, default="1025,2049")
    p.add_argument("--batch-size", type=int, default=1)
    p.add_argument("--model", type=str, default="deeplabv3")
    p.add_argument("--backbone", type=str, default="resnet101")
    p.add_argument("--backbone-para", type=str, default='{"pretrained": false}')
    p.add_argument("--model-para", type=str, default="{}")
    p.add_argument("--align-corner", type=str2bool, default="True")
    p.add_argument("--dataset", type=str, default="CS")
    p.add_argument("--restore-from", type=str, default=None)
    p.add_argument("--channel-cfg", type=str, default=None)
    p.add_argument("--save-dir", type=str, default="./ckpt")
    p.add_argument("--precision", type=str, default="fp16", choices=("fp16", "fp8"),
                   help="fp8: the calibrated e4m3 engine (opt-in; accuracy on trained weights is unmeasured)")
    p.add_argument("--calib-batches", type=int, default=2,
                   help="fp8: batches the activation maxima are taken over (synthetic images without --data-para)")
    p.add_argument("--data-para", type=str, default=None,
                   help='fp8: JSON {"root": ..., "list_path": ...}: calibrate on the first batches of --dataset')
    p.add_argument("--save-flat", type=str, default=None,
                   help="also write the flat engine file (with the uint8 input table) that the C runtime loads")
    p.add_argument("--runtime", type=str, default="python", choices=("python", "c"),
                   help="c: also time deploy.CEngine (fp32 and uint8 input) in the same run")
    p.add_argument("--seed", type=int, default=12345)
    return p


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)      # the datasets' normalisation (datasets/base.py)
HBM_MEASURED = 6.29e12                                        # float4-copy rate measured on an MI355X (8.0e12 on the sheet)


def time_u8_kernel(ce, frame, launches=200):
    """Seconds per launch of dcfp_image_u8_hwc_to_nhwc_f16 on `frame` (uint8 [N,H,W,3] on the device): device events
    around `launches` back-to-back launches, after a warm-up."""
    import ctypes as C
    from dcfp_amd import _lib, ops
    L = _lib.lib()
    N, H, W, _ = frame.shape
    table = deploy.input_table(MEAN, STD).to(frame.device)
    dst = torch.empty((N, H, W, 8), dtype=torch.float16, device=frame.device)
    order = (C.c_int * 3)(2, 1, 0)

    def launch():
        _lib.check(L.dcfp_image_u8_hwc_to_nhwc_f16(C.c_void_p(frame.data_ptr()), 3 * W, N, H, W,
                                                   C.c_void_p(table.data_ptr()), order, C.c_void_p(dst.data_ptr()), 8,
                                                   ops._stream()), "uint8 input kernel")
    for _ in range(10):
        launch()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        launch()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / launches


def benchmark_c_runtime(args, flat_path, x, dev, h, w):
    """The C runtime's two lines and the uint8 kernel's own line."""
    from dcfp_amd import ops
    ce = deploy.CEngine(flat_path, dev)
    what = f"{args.model}-{args.backbone} {h}x{w} batch {args.batch_size} {args.precision} engine"
    avg_c = benchmark(ce, x)
    print(f"Average batch time: {avg_c * 1e3:.2f} ms ({args.batch_size / avg_c:.2f} images/s) {what}, C runtime, "
          f"fp32 input")
    gen = torch.Generator().manual_seed(args.seed)
    host = torch.randint(0, 256, (args.batch_size, h, w, 3), generator=gen, dtype=torch.uint8).pin_memory()
    frame = torch.empty_like(host, device=dev)

    def from_frame(_):                               # the frame crosses to the device inside the timed call
        frame.copy_(host, non_blocking=True)
        return [ops.upsample_bilinear(z, (h, w), ce.align_corner) for z in ce.run_u8(frame)]
    avg_u8 = benchmark(from_frame, None)
    print(f"Average batch time: {avg_u8 * 1e3:.2f} ms ({args.batch_size / avg_u8:.2f} images/s) {what}, C runtime, "
          f"uint8 input (host -> device copy of the frame included)")
    t = time_u8_kernel(ce, frame)
    nbytes = args.batch_size * h * w * (3 + 2 * 8)
    print(f"uint8 input kernel: {t * 1e6:.1f} us for {nbytes / 1e6:.1f} MB ({nbytes / t / 1e12:.2f} TB/s); byte bound "
          f"{nbytes / HBM_MEASURED * 1e6:.1f} us at {HBM_MEASURED / 1e12:.2f} TB/s")
    return avg_c, avg_u8, t


def get_num_classes(dataset):
    for prefix, n in (("CS", 19), ("CTX", 59), ("ADE", 150), ("COCO", 171)):
        if dataset.startswith(prefix):
            return n
    raise ValueError(dataset)


def benchmark(engine, x, nwarmup=10, nruns=50):
    """totrt.benchmark: warm-up, then nruns calls timed one by one with a synchronise around each."""
    for _ in range(nwarmup):
        engine(x)
    torch.cuda.synchronize()
    times = []
    for _ in range(nruns):
        t0 = time.perf_counter()
        engine(x)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return sum(times) / len(times)


def calibration_batches(args, h, w, dev):
    """--calib-batches float32 batches: the first of the dataset's validation list with --data-para, else seeded
    N(0,1) images of the timed shape."""
    if args.data_para:
        from dcfp_amd.datasets import EvalLoader, build_dataset
        dataset = build_dataset(args.dataset, split="val", data_para=json.loads(args.data_para))
        for i, (image, _, _) in enumerate(EvalLoader(dataset, args.batch_size, dev, num_workers=2)):
            if i >= args.calib_batches:
                break
            yield image
        return
    gen = torch.Generator().manual_seed(args.seed)
    for _ in range(args.calib_batches):
        yield torch.randn(args.batch_size, 3, h, w, generator=gen).to(dev)


def main(argv=None):
    args = get_parser().parse_args(argv)
    h, w = map(int, args.input_size.split(","))
    model = getattr(networks, args.model).Seg_Model(
        backbone=args.backbone, backbone_para=json.loads(args.backbone_para), model_para=json.loads(args.model_para),
        num_classes=get_num_classes(args.dataset), align_corner=args.align_corner, criterion=None, deepsup=False)
    if args.channel_cfg:
        init_pruned_model(model, torch.load(args.channel_cfg, weights_only=False))
    if args.restore_from:
        load_model(model, args.restore_from)
    dev = torch.device("cuda:0")
    engine = deploy.build_engine(model.eval())
    if args.precision == "fp8":
        amax = deploy.calibrate(engine.to(dev), calibration_batches(args, h, w, dev))
        engine = deploy.build_engine(model, precision="fp8", amax=amax)
    os.makedirs(args.save_dir, exist_ok=True)
    path = os.path.join(args.save_dir, f"engine_{args.precision}.pth")
    torch.save(engine.state_dict(), path)
    print(f"saved {path}: {len(engine.plan)} layer records, "
          f"{sum(t.numel() * t.element_size() for t in engine.tensors) / 2 ** 20:.1f} MiB")
    engine = deploy.load_engine(path, dev)
    x = torch.randn(args.batch_size, 3, h, w, device=dev)
    avg = benchmark(engine, x)
    print(f"Average batch time: {avg * 1e3:.2f} ms ({args.batch_size / avg:.2f} images/s) "
          f"{args.model}-{args.backbone} {h}x{w} batch {args.batch_size} {args.precision} engine")
    if args.save_flat or args.runtime == "c":
        flat_path = args.save_flat or os.path.join(args.save_dir, f"engine_{args.precision}.bin")
        size = deploy.save_flat(engine, flat_path, MEAN, STD)
        print(f"saved {flat_path}: flat engine file version {deploy.FLAT_VERSION}, {size / 2 ** 20:.1f} MiB")
        if args.runtime == "c":
            benchmark_c_runtime(args, flat_path, x, dev, h, w)
    return avg


if __name__ == "__main__":
    main()
