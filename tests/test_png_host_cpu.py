"""CPU: the host half of the label-PNG export - the stream format's restatement (tests/_png_ref.py) against
zlib and PIL, evaluate.png_container, the size bound, evaluate.reverse_id_table, the encoder's descriptor checks, and
the command line and file names of tools/evaluate_test.py."""
import ctypes
import importlib.util
import io
import os
import zlib

import numpy as np
import pytest

import _png_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (3, 2), (2, 257), (5, 259), (7, 263), (9, 520), (16, 2049), (3, 4099), (8, 300)]


def label_map(rng, H, W, classes=19, rects=6):
    m = np.full((H, W), rng.randint(0, classes), dtype=np.uint8)
    for _ in range(rects):
        y, x = rng.randint(0, H), rng.randint(0, W)
        m[y:y + rng.randint(1, H + 1), x:x + rng.randint(1, W + 1)] = rng.randint(0, classes)
    return m


def maps():
    rng = np.random.RandomState(11)
    out = [label_map(rng, H, W) for H, W in SHAPES]
    out.append(rng.randint(0, 256, (8, 300)).astype(np.uint8))           # all literals: the worst case of the bound
    out.append(rng.randint(0, 256, (3, 4099)).astype(np.uint8))
    return out


def evaluate_test_tool():
    spec = importlib.util.spec_from_file_location("evaluate_test_tool", os.path.join(ROOT, "tools", "evaluate_test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("image", maps(), ids=lambda m: "%dx%d_%d" % (m.shape + (int(m.max()),)))
def test_restatement_round_trips_and_stays_under_the_bound(image):
    from PIL import Image
    from dcfp_amd import _lib, evaluate
    H, W = image.shape
    stream = R.deflate_labels(image)
    assert zlib.decompress(stream) == R.filtered_rows(image).tobytes()
    bound = _lib.lib().dcfp_png_deflate_bound(H, W)
    assert bound == R.bound(H, W) and len(stream) <= bound
    palette = [int(v) for v in np.random.RandomState(5).randint(0, 256, 3 * 256)]
    with Image.open(io.BytesIO(evaluate.png_container(stream, H, W, palette))) as im:
        im.load()
        assert im.mode == "P" and im.size == (W, H)
        assert im.getpalette() == palette
        assert np.array_equal(np.asarray(im), image)
    with Image.open(io.BytesIO(evaluate.png_container(stream, H, W))) as im:
        im.load()
        assert im.mode == "L" and im.size == (W, H)
        assert np.array_equal(np.asarray(im), image)


def test_bound_is_met_by_nothing_but_literals():
    """9-bit literals only (bytes 144 .. 255, no two neighbours equal in the filtered row): the bound's own case."""
    for H, W in ((1, 1), (8, 300), (16, 2049)):
        y, x = np.mgrid[0:H, 0:W]
        f = (144 + (37 * x + y) % 112).astype(np.uint8)                    # neighbours differ by 37 mod 112
        assert not (f[:, 1:] == f[:, :-1]).any()
        image = np.cumsum(f.astype(np.int64), axis=0).astype(np.uint8)     # Up-filtered, it is f again
        assert np.array_equal(R.filtered_rows(image)[:, 1:], f)
        n = len(R.deflate_labels(image))
        # the filter byte 2 is an 8-bit literal: one bit per row short of the bound's all-9-bit rows
        assert R.bound(H, W) - H <= n <= R.bound(H, W)


def test_reverse_id_table_of_cityscapes_and_pascal_context(tmp_path):
    from dcfp_amd import evaluate
    from dcfp_amd.datasets import cs, ctx
    lst = tmp_path / "test.lst"
    lst.write_text("a_leftImg8bit.png\n")
    table = evaluate.reverse_id_table(cs.DataSet(str(tmp_path), str(lst), split="test"))
    want = np.arange(256, dtype=np.uint8)
    for raw, train in cs._TRAIN_IDS.items():
        want[train] = raw
    want[255] = 30
    assert table.dtype == np.uint8 and np.array_equal(table, want)
    names = tmp_path / "val.txt"
    names.write_text("2008_000002\n")
    table = evaluate.reverse_id_table(ctx.DataSet(str(tmp_path), str(names), split="val"))
    want = np.arange(256, dtype=np.int64) + 1                              # class k is raw k + 1 ...
    want[255] = 0                                                          # ... and ignore is raw 0
    assert np.array_equal(table, want.astype(np.uint8))


def test_png_descriptor_errors_do_not_need_a_gpu():
    """Bad descriptors are rejected on the host side with the documented negative codes, before any HIP call."""
    from dcfp_amd import _lib
    L = _lib.lib()
    H, W, N, P = 4, 6, 2, 2
    pred = (ctypes.c_int32 * (N * H * W))()
    luts = (ctypes.c_uint8 * (4 * 256))()
    bound = L.dcfp_png_deflate_bound(H, W)
    out = (ctypes.c_uint8 * (N * P * bound))()
    meta = (ctypes.c_int64 * (2 * N * P))()
    ws_bytes = L.dcfp_png_deflate_workspace_bytes(N, H, W, P)
    assert bound == R.bound(H, W) and ws_bytes > 0
    ws = (ctypes.c_uint32 * (ws_bytes // 4 + 1))()
    offsets, lengths = ctypes.byref(meta), ctypes.byref(meta, 8 * N * P)

    def call(pred=pred, N=N, H=H, W=W, P=P, out_bytes=N * P * bound, ws_bytes=ws_bytes):
        return L.dcfp_png_deflate_labels_i32(pred, N, H, W, luts, P, out, out_bytes, offsets, lengths, ws, ws_bytes, None)
    assert call(pred=None) == _lib.E_BADDESC
    assert call(P=0) == _lib.E_BADDESC
    assert call(P=5) == _lib.E_BADDESC
    assert call(W=0) == _lib.E_BADDESC
    assert call(H=0) == _lib.E_BADDESC and call(N=0) == _lib.E_BADDESC
    assert call(out_bytes=N * P * bound - 1) == _lib.E_BADDESC
    assert call(ws_bytes=ws_bytes - 1) == _lib.E_WORKSPACE
    assert call(H=4097, out_bytes=1 << 40, ws_bytes=1 << 40) == _lib.E_UNSUPPORTED
    assert call(W=8193, out_bytes=1 << 40, ws_bytes=1 << 40) == _lib.E_UNSUPPORTED
    assert L.dcfp_png_deflate_bound(4096, 8192) == R.bound(4096, 8192)
    assert L.dcfp_png_deflate_bound(4097, 8) == 0 and L.dcfp_png_deflate_bound(8, 8193) == 0
    assert L.dcfp_png_deflate_bound(0, 8) == 0
    assert L.dcfp_png_deflate_workspace_bytes(1, 8, 8, 0) == 0 and L.dcfp_png_deflate_workspace_bytes(1, 8, 8, 5) == 0
    assert L.dcfp_png_deflate_workspace_bytes(4, 4096, 8192, 4) >= 4 * 4 * R.bound(4096, 8192) - 16 * 8
    assert L.dcfp_abi_version() == 2


def test_png_container_rejects_bad_arguments():
    from dcfp_amd import evaluate
    with pytest.raises(ValueError):
        evaluate.png_container(b"", 0, 4)
    with pytest.raises(ValueError):
        evaluate.png_container(b"", 4, 4, palette=[1, 2])
    with pytest.raises(ValueError):
        evaluate.png_container(b"", 4, 4, palette=[0] * 771)


def test_writer_writes_and_reraises(tmp_path):
    from dcfp_amd import evaluate
    with evaluate.PngWriter() as w:
        assert w.pool._max_workers <= 4
        for i in range(9):
            w.write(str(tmp_path / ("f%d.bin" % i)), bytes([i]) * (i + 1))
    for i in range(9):
        assert (tmp_path / ("f%d.bin" % i)).read_bytes() == bytes([i]) * (i + 1)
    w = evaluate.PngWriter(threads=64)
    assert w.pool._max_workers == 4
    w.write(str(tmp_path / "no_such_dir" / "f.bin"), b"x")
    w.write(str(tmp_path / "late.bin"), b"y")
    with pytest.raises(OSError):
        w.close()
    assert (tmp_path / "late.bin").read_bytes() == b"y"                     # the error waited for the other writes


def test_parser_accepts_the_reference_command_line():
    """The evaluation line of the reference's scripts/cs/finetune.sh (multi-scale test), values filled in."""
    tool = evaluate_test_tool()
    line = ["--dataset", "CS", "--model", "deeplabv3", "--backbone", "resnet101", "--batch-size", "4", "--whole", "True",
            "--flip", "True", "--input-size", "769,769", "--align-corner", "True", "--ms", "0.5,0.75,1,1.25,1.5,1.75",
            "--num-workers", "8", "--restore-from", "snapshots_deeplabv3/CS_scenes_40000.pth", "--save-predict", "False",
            "--channel-cfg", "snapshots/channel_cfg.pth"]
    args = tool.get_parser().parse_args(line)
    assert args.dataset == "CS" and args.whole and args.flip and args.align_corner and args.batch_size == 4
    assert args.ms == "0.5,0.75,1,1.25,1.5,1.75" and args.channel_cfg == "snapshots/channel_cfg.pth"
    assert args.split == "test" and args.longsize == -1 and args.shortsize == -1 and args.ddp
    assert tool.output_root(args) == os.path.join("snapshots_deeplabv3", "outputs")
    # every option of the reference's evaluate_test.py parser, and this project's own
    more = ["--ignore-label", "255", "--longsize", "2048", "--shortsize", "-1", "--ddp", "False", "--backbone-para", "{}",
            "--model-para", "{}", "--data-para", "{}", "--data-dir", "test", "--use-trt", "True", "--seed", "1",
            "--dist-backend", "gloo", "--fused-vote", "False", "--snapshot-dir", "out", "--split", "val",
            "--device-png", "True"]
    args = tool.get_parser().parse_args(line + more)
    assert args.device_png is True and args.use_trt is True and args.split == "val" and args.longsize == 2048
    assert tool.output_root(args) == os.path.join("out", "outputs")
    assert isinstance(tool.get_parser().parse_args([]).device_png, bool)


def test_output_file_names():
    tool = evaluate_test_tool()
    assert tool.output_names("berlin_000000_000019_leftImg8bit") == ("berlin_000000_000019_leftImg8bit.png",
                                                                     "berlin_000000_000019.png")
    assert tool.output_names("2008_000002") == ("2008_000002.png", "2008_000002.png")


def test_evaluate_tool_keeps_its_default():
    spec = importlib.util.spec_from_file_location("evaluate_tool_for_png", os.path.join(ROOT, "tools", "evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.get_parser().parse_args([]).device_png is False
