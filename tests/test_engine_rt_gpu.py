"""GPU: the C engine runtime (csrc/engine_rt.hip, deploy.CEngine) and the uint8 input kernel (csrc/image_u8.hip).

The runtime launches the kernels the Python engine launches, with the same arguments in the same order, so every
comparison with deploy.Engine is torch.equal - anything else is a bug in the port.  The uint8 kernel is a lookup and is
compared exactly against numpy.  R50 with the closed-form weights; every case takes seconds."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _model_cases as mc  # noqa: E402
from oracle import fill  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# tag: (head, align_corner, slimmed, fp8, input N x H x W)
CASES = {
    "simple_2x65x65": ("simple", True, False, False, (2, 65, 65)),
    "v3_align_2x65x65": ("deeplabv3", True, False, False, (2, 65, 65)),
    "v3_noalign_2x65x65": ("deeplabv3", False, False, False, (2, 65, 65)),
    "v3p_2x65x65": ("deeplabv3p", True, False, False, (2, 65, 65)),
    "psp_2x65x65": ("psp", True, False, False, (2, 65, 65)),
    "psp_1x33x41": ("psp", True, False, False, (1, 33, 41)),          # a 6x6 prior meets a 5x6 map
    "v3p_slim_2x65x65": ("deeplabv3p", True, True, False, (2, 65, 65)),   # ragged widths
    "simple_f8_2x65x65": ("simple", True, False, True, (2, 65, 65)),
    "v3_f8_2x65x65": ("deeplabv3", True, False, True, (2, 65, 65)),
}
_engines = {}


def _pair(head, align, slim, fp8, tmp_path_factory, table=False):
    """(Python engine on the GPU, CEngine of the flat file written from that very engine), one per session."""
    key = (head, align, slim, fp8, table)
    if key not in _engines:
        from dcfp_amd import deploy
        if slim:
            import test_deploy_heads_gpu as heads
            m = heads._slim(head, str(tmp_path_factory.mktemp("slim")))
        else:
            m = mc.build_model(head, "resnet50", align, torch.device("cpu"), criterion=False, deepsup=False).eval()
        eng = deploy.build_engine(m).to("cuda:0")
        if fp8:                       # calibrate once; the flat file is written from the calibrated engine itself
            amax = deploy.calibrate(eng, [fill.closed_form_input(2, 65, 65)])
            eng = deploy.build_engine(m, precision="fp8", amax=amax).to("cuda:0")
        data = deploy.flat_bytes(eng, MEAN, STD) if table else deploy.flat_bytes(eng)
        _engines[key] = (eng, deploy.CEngine(data, "cuda:0"), data)
    return _engines[key]


def _v3(tmp_path_factory, table=False):
    return _pair("deeplabv3", True, False, False, tmp_path_factory, table)


@pytest.mark.parametrize("tag", list(CASES))
def test_bit_identical_to_the_python_engine(tag, tmp_path_factory, cuda):
    head, align, slim, fp8, size = CASES[tag]
    eng, ce, _ = _pair(head, align, slim, fp8, tmp_path_factory)
    assert ce.format == (2 if fp8 else 1) and ce.align_corner is align and ce.num_classes == 19 and ce.eval() is ce
    assert ce.meta == eng.meta
    x = fill.closed_form_input(*size).to(cuda)
    want = eng.lowres_logits(x)[0]
    got = ce.lowres_logits(x)
    assert isinstance(got, list) and got[0].dtype == torch.float32 and got[0].shape == want.shape
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    assert torch.equal(got[0], want), float((got[0] - want).abs().max())
    assert ce.buffer_shapes(size[1], size[2]) == eng.buffer_shapes(size[1], size[2])


def test_no_dependence_on_stale_bytes(tmp_path_factory, cuda):
    """The workspace is filled with 0xFF before every call; shape A, the larger shape B, then A again."""
    eng, ce, _ = _pair("psp", True, False, False, tmp_path_factory)
    for size in ((1, 33, 41), (2, 65, 65), (1, 33, 41)):
        x = fill.closed_form_input(*size).to(cuda)
        ce.workspace(*size).fill_(0xFF)
        got = ce.lowres_logits(x)[0]
        assert torch.equal(got, eng.lowres_logits(x)[0]), size
    eng, ce, _ = _v3(tmp_path_factory)
    for size in ((1, 33, 41), (2, 65, 65), (1, 33, 41)):
        x = fill.closed_form_input(*size).to(cuda)
        ce.workspace(*size).fill_(0xFF)
        assert torch.equal(ce.lowres_logits(x)[0], eng.lowres_logits(x)[0]), size


def _lookup(img, table, order, c8):
    """numpy: dst[n][y][x][c] = table[c][src[n][y][x][order[c]]], zeros in the padding channels (fp16 bits)."""
    t = table.view(np.uint16)
    out = np.zeros(img.shape[:3] + (c8,), dtype=np.uint16)
    for c in range(3):
        out[..., c] = t[c][img[..., order[c]]]
    return out


# (N, H, W, row pitch - 3 W, byte offset of the image in its allocation, C8)
U8_SHAPES = [(1, 5, 7, 0, 0, 8), (2, 33, 41, 5, 0, 8), (1, 64, 64, 0, 0, 8),
             (1, 3, 1100, 1, 3, 8),      # two blocks per row, rows and base at odd addresses
             (2, 4, 37, 0, 0, 16)]       # a second all-zero chunk per pixel


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
@pytest.mark.parametrize("shape", U8_SHAPES)
def test_uint8_input_kernel_is_the_lookup(shape, order, cuda):
    from dcfp_amd import _lib, deploy
    L = _lib.lib()
    N, H, W, extra, base, c8 = shape
    pitch = 3 * W + extra
    rng = np.random.default_rng(W)
    store = rng.integers(0, 256, size=base + N * H * pitch, dtype=np.uint8)
    store[base:base + 512] = np.arange(512, dtype=np.uint8)[:min(512, store.size - base)]     # every byte value occurs
    img = store[base:].reshape(N, H, pitch)[:, :, :3 * W].reshape(N, H, W, 3)
    table = deploy.input_table(MEAN, STD)
    assert table.dtype == torch.float16 and tuple(table.shape) == (3, 256)
    want = _lookup(img, table.numpy(), order, c8)
    src = torch.from_numpy(store).to(cuda)
    dst = torch.full((N, H, W, c8), -1, dtype=torch.int16, device=cuda)          # 0xFFFF everywhere
    tab = table.to(cuda)
    st = L.dcfp_image_u8_hwc_to_nhwc_f16(C.c_void_p(src.data_ptr() + base), pitch, N, H, W, C.c_void_p(tab.data_ptr()),
                                         (C.c_int * 3)(*order), C.c_void_p(dst.data_ptr()), c8, None)
    assert st == 0
    got = dst.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want)
    assert not got[..., 3:].any()                                               # the padding channels: exact zeros


def test_uint8_input_kernel_refuses_bad_arguments(cuda):
    from dcfp_amd import _lib
    L = _lib.lib()
    p, order = C.c_void_p(4096), (C.c_int * 3)(0, 1, 2)
    call = L.dcfp_image_u8_hwc_to_nhwc_f16
    assert call(None, 21, 1, 5, 7, p, order, p, 8, None) == _lib.E_BADDESC
    assert call(p, 20, 1, 5, 7, p, order, p, 8, None) == _lib.E_BADDESC          # row pitch < 3 W
    assert call(p, 21, 1, 5, 7, p, order, p, 12, None) == _lib.E_BADDESC         # C8 no multiple of 8
    assert call(p, 21, 1, 5, 7, p, (C.c_int * 3)(0, 1, 3), p, 8, None) == _lib.E_BADDESC
    assert call(p, 21, 1, 5, 7, p, order, C.c_void_p(4104), 8, None) == _lib.E_BADDESC   # dst not 16-byte aligned


def test_input_table_is_rounded_once_from_fp64():
    from dcfp_amd import deploy
    t = deploy.input_table(MEAN, STD)
    v = np.arange(256, dtype=np.float64)
    for c in range(3):
        want = ((v / 255.0 - MEAN[c]) / STD[c]).astype(np.float16)
        assert np.array_equal(t[c].numpy().view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("bgr", [True, False])
def test_run_u8_equals_run_f32_on_the_table_values(bgr, tmp_path_factory, cuda):
    """The fp32 image made of the table's own values converts to fp16 without rounding, so the logits are bit-equal."""
    from dcfp_amd import deploy
    eng, ce, _ = _v3(tmp_path_factory, table=True)
    if not bgr:
        ce = deploy.CEngine(deploy.flat_bytes(eng, MEAN, STD, bgr=False), cuda)
    assert ce.has_input_table
    N, H, W = 2, 33, 41
    gen = torch.Generator().manual_seed(3)
    wide = torch.randint(0, 256, (N, H, W + 2, 3), generator=gen, dtype=torch.uint8).to(cuda)
    img = wide[:, :, :W]                                                         # rows 3 (W + 2) bytes apart
    order = [2, 1, 0] if bgr else [0, 1, 2]
    table = deploy.input_table(MEAN, STD).to(cuda)
    x = torch.stack([table[c][img[..., order[c]].long()] for c in range(3)], dim=1).float().contiguous()
    want = ce.lowres_logits(x)[0]
    assert torch.equal(want, eng.lowres_logits(x)[0])
    assert torch.equal(ce.run_u8(img)[0], want)
    assert torch.equal(ce.run_u8(img.contiguous())[0], want)


def test_error_paths_launch_nothing(tmp_path_factory, cuda):
    from dcfp_amd import _lib
    L = _lib.lib()
    eng, ce, _ = _v3(tmp_path_factory)
    N, H, W = 1, 33, 41
    x = fill.closed_form_input(N, H, W).to(cuda)
    need = ce.workspace_bytes(N, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    out = torch.full(ce.output_shape(N, H, W), 7.0, device=cuda)
    args = (ce.handle, C.c_void_p(ce.weights.data_ptr()), C.c_void_p(x.data_ptr()), N, H, W, C.c_void_p(ws.data_ptr()))
    assert L.dcfp_engine_run_f32(*args, need - 1, C.c_void_p(out.data_ptr()), None) == _lib.E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                              # untouched
    assert L.dcfp_engine_run_f32(*args, need, C.c_void_p(out.data_ptr()), None) == 0
    assert torch.equal(out, eng.lowres_logits(x)[0])
    assert not ce.has_input_table
    u8 = torch.zeros((N, H, W, 3), dtype=torch.uint8, device=cuda)
    out.fill_(7.0)
    assert L.dcfp_engine_run_u8(ce.handle, C.c_void_p(ce.weights.data_ptr()), C.c_void_p(u8.data_ptr()), 3 * W, N, H, W,
                                C.c_void_p(ws.data_ptr()), need, C.c_void_p(out.data_ptr()), None) == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(RuntimeError, match="input table"):
        ce.run_u8(u8)
    with pytest.raises(ValueError, match="magic"):
        from dcfp_amd import deploy
        deploy.CEngine(b"x" * 4096, cuda)


def test_evaluation_driver_takes_a_cengine(tmp_path_factory, cuda):
    from dcfp_amd import evaluate as ev
    eng, ce, _ = _v3(tmp_path_factory)
    x = fill.closed_form_input(2, 65, 65).to(cuda)
    want = ev.predict_labels(eng, x)
    got = ev.predict_labels(ce, x)
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert torch.equal(ce(x)[0], eng(x)[0])


def test_standalone_program_writes_the_engines_logits(tmp_path, tmp_path_factory, cuda):
    """tools/engine_run.cpp: no Python, one run in a fresh child process.  (Last in this file: a non-zero exit ends the
    test here and nothing further is started on the GPU.)"""
    eng, _, data = _v3(tmp_path_factory, table=True)
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dcfp_amd", "csrc"), "engine_run"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(ROOT, "dcfp_amd", "csrc", "build", "engine_run")
    N, H, W = 2, 65, 65
    x = fill.closed_form_input(N, H, W)
    want = eng.lowres_logits(x.to(cuda))[0].cpu()
    (tmp_path / "engine.bin").write_bytes(data)
    x.numpy().tofile(str(tmp_path / "in.raw"))
    cmd = ["timeout", "-k", "10", "120", exe, str(tmp_path / "engine.bin"), str(N), str(H), str(W),
           str(tmp_path / "in.raw"), str(tmp_path / "out.raw")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got = np.fromfile(str(tmp_path / "out.raw"), dtype=np.float32)
    assert got.size == want.numel() and np.array_equal(got.view(np.uint32), want.numpy().reshape(-1).view(np.uint32))
