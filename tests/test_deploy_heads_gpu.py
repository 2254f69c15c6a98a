"""GPU: the frozen fp16 engines of DeepLabv3+ and PSPNet (deploy.build_engine) as whole models.

Acceptance is that of tests/test_deploy_gpu.py, unchanged.  The yardstick is computed here on the CPU and never uses
the code under test (tests/_deploy_heads_ref.py): the fp64 eval-mode logits, and an fp16-storage emulation of the same
forward run twice (sums in fp64 and in fp32); e / r = the larger of the two emulations' max-abs / relative-L2 distances
to the fp64 logits.  The engine's low-resolution logits against fp64: relative L2 <= 1.5 r, max-abs <= 3 e.  Labels
(where the align_corners grid of the full-resolution map coincides with the low-resolution pixels):
predict_labels(engine, x) equals the fp64 argmax wherever the fp64 top-2 margin is >= 6 e, and at most 10 % of the
pixels may be left out.

The yardstick is recomputed by the test, never hard-coded; its values (e, r, pixels left out) per case are in the table
of DESIGN.md §11.  Each case prints the yardstick and the engine's max-abs / relative L2 before it asserts."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _deploy_heads_ref as href  # noqa: E402
import _model_cases as mc  # noqa: E402
from oracle import fill, model as omodel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# tag: (head, align_corner, slimmed, input N x H x W, low-resolution map, labels checked)
CASES = {
    "psp_align_2x65x65": ("psp", True, False, (2, 65, 65), (9, 9), True),
    "v3p_align_2x65x65": ("deeplabv3p", True, False, (2, 65, 65), (17, 17), True),
    "psp_noalign_2x64x64": ("psp", False, False, (2, 64, 64), (8, 8), False),
    "v3p_noalign_2x64x64": ("deeplabv3p", False, False, (2, 64, 64), (16, 16), False),
    "psp_align_1x33x41": ("psp", True, False, (1, 33, 41), (5, 6), False),     # a 6x6 prior on a 5x6 map
    "psp_slim_2x65x65": ("psp", True, True, (2, 65, 65), (9, 9), True),
    "v3p_slim_2x65x65": ("deeplabv3p", True, True, (2, 65, 65), (17, 17), True),
}
_models, _cache = {}, {}


def _slim(head, tmp):
    """The R50 slimmed as mc.slim_model_logits_check does: global_percent 0.5 on the head's prune fixture's scores."""
    from dcfp_amd import pruners
    tag = {"psp": "pspr50", "deeplabv3p": "v3pr50"}[head]
    g = np.load(os.path.join(mc.G, f"prune_{tag}_gp50.npz"))
    cpu = torch.device("cpu")
    m = mc.build_model(head, "resnet50", True, cpu, criterion=False)
    _, pruned, cfg = mc._prune_gp50(m, os.path.join(tmp, "score.pth"))
    assert list(cfg.keys()) == g["names"].tolist()
    slim = mc.build_model(head, "resnet50", True, cpu, criterion=False)
    pruners.init_pruned_model(slim, cfg)
    slim.load_state_dict(pruned.state_dict())
    return slim.eval()


def _model(head, align, slim, tmp_path_factory):
    """(eval-mode model on the CPU with closed-form weights, its engine on the GPU), one per session."""
    key = (head, align, slim)
    if key not in _models:
        from dcfp_amd import deploy
        if slim:
            m = _slim(head, str(tmp_path_factory.mktemp("slim")))
        else:
            m = mc.build_model(head, "resnet50", align, torch.device("cpu"), criterion=False, deepsup=False).eval()
        _models[key] = (m, deploy.build_engine(m).to("cuda:0"))
    return _models[key]


def _setup(tag, tmp_path_factory):
    if tag not in _cache:
        head, align, slim, size, _, _ = CASES[tag]
        m, eng = _model(head, align, slim, tmp_path_factory)
        x = fill.closed_form_input(*size)
        cfg = omodel.Cfg(head, "resnet50", align_corner=align, deepsup=False)
        ref, e, r = href.yardstick(m.state_dict(), x, cfg)
        _cache[tag] = (m, x, ref, e, r, eng)
    return _cache[tag]


def _compare(tag, tmp_path_factory, cuda):
    from dcfp_amd import evaluate as ev
    head, align, slim, size, low_hw, labelled = CASES[tag]
    m, x, ref, e, r, eng = _setup(tag, tmp_path_factory)
    assert tuple(ref.shape) == (size[0], 19) + low_hw
    xd = x.to(cuda)
    low = eng.lowres_logits(xd)[0]
    assert low.dtype == torch.float32 and tuple(low.shape) == tuple(ref.shape)
    got = low.double().cpu()
    rel = float((got - ref).norm() / ref.norm())
    err = float((got - ref).abs().max())
    print(f"deploy {tag}: yardstick e {e:.4g} r {r:.3e} (|logits| <= {float(ref.abs().max()):.4g}); "
          f"engine max-abs {err:.4g} rel-L2 {rel:.3e}")
    assert torch.isfinite(got).all()
    assert rel <= 1.5 * r, (rel, r)
    assert err <= 3 * e, (err, e)
    H, W = x.shape[2:]
    full = eng(xd)
    assert isinstance(full, list) and tuple(full[0].shape) == (x.shape[0], 19, H, W) and full[0].dtype == torch.float32
    assert eng.align_corner is align
    if not labelled:
        return
    labels = ev.predict_labels(eng, xd)
    h, w = ref.shape[2:]
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (x.shape[0], H, W)
    assert (H - 1) % (h - 1) == 0 and (W - 1) % (w - 1) == 0
    sub = labels[:, ::(H - 1) // (h - 1), ::(W - 1) // (w - 1)].cpu().long()
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) >= 6 * e
    left_out = 1.0 - float(sure.double().mean())
    print(f"deploy {tag}: {100 * left_out:.1f} % of the low-resolution pixels have an fp64 top-2 margin below 6 e")
    assert left_out <= 0.10, left_out
    assert torch.equal(sub[sure], ref.argmax(dim=1)[sure])


@pytest.mark.parametrize("tag", list(CASES))
def test_engine_logits_and_labels_against_fp64(tag, tmp_path_factory, cuda, capsys):
    if CASES[tag][2]:
        m = _setup(tag, tmp_path_factory)[0]
        widths = [c.out_channels for c in m.modules() if isinstance(c, torch.nn.Conv2d)]
        assert sum(1 for c in widths if c % 8) >= 50, widths      # 50 (PSP) / 52 (v3+) ragged widths
    with capsys.disabled():
        _compare(tag, tmp_path_factory, cuda)


@pytest.mark.parametrize("tag", ["psp_align_2x65x65", "v3p_align_2x65x65"])
def test_saved_engine_gives_bit_identical_logits(tag, tmp_path_factory, tmp_path, cuda):
    from dcfp_amd import deploy
    _, x, _, _, _, eng = _setup(tag, tmp_path_factory)
    xd = x.to(cuda)
    a = eng.lowres_logits(xd)[0].clone()
    assert torch.equal(deploy.load_engine(eng.state_dict(), cuda).lowres_logits(xd)[0], a)
    path = str(tmp_path / "engine.pth")
    torch.save(eng.state_dict(), path)
    assert torch.equal(deploy.load_engine(path, cuda).lowres_logits(xd)[0], a)
    assert torch.equal(eng.lowres_logits(xd)[0], a)              # buffers reused across calls: same bits


def test_another_shape_and_back_gives_the_same_bits(tmp_path_factory, cuda):
    """PSP 2x65x65 -> 1x33x41 -> 2x65x65 on a fresh engine."""
    from dcfp_amd import deploy
    _, x, _, _, _, eng0 = _setup("psp_align_2x65x65", tmp_path_factory)
    eng = deploy.load_engine(eng0.state_dict(), cuda)
    xd = x.to(cuda)
    a = eng.lowres_logits(xd)[0].clone()
    assert torch.equal(a, eng0.lowres_logits(xd)[0])
    small = eng.lowres_logits(xd[:1, :, :33, :41].contiguous())[0].clone()
    assert tuple(small.shape) == (1, 19, 5, 6)
    assert torch.equal(eng.lowres_logits(xd)[0], a)
    assert torch.equal(eng.lowres_logits(xd[:1, :, :33, :41].contiguous())[0], small)


def test_returning_to_a_shape_after_the_pyramid_workspace_grew(tmp_path_factory, cuda):
    """2x89x89 pools two 12x12 maps (1, 2, 3 and 6 all divide 12: 6 x 6 cells between the window boundaries each);
    2x65x65 pools two 9x9 maps (9 x 9 cells each, every row and column its own).  The batch is the same and every map
    smaller, the s x s pooled maps equal, so no slot grows, but the pyramid workspace does (2 x 81 > 2 x 36 cells).
    The launch list of the first shape must not keep the old workspace: same bits on return, and memory handed back
    to the allocator (re-allocated here and filled with a pattern) stays untouched."""
    from dcfp_amd import deploy
    _, x, _, _, _, eng0 = _setup("psp_align_2x65x65", tmp_path_factory)
    eng = deploy.load_engine(eng0.state_dict(), cuda)          # a fresh engine: nothing allocated yet
    big = fill.closed_form_input(2, 89, 89).to(cuda)
    two = x.to(cuda)
    a = eng.lowres_logits(big)[0].clone()
    slots = [s.data_ptr() for s in eng._slots]
    b = eng.lowres_logits(two)[0].clone()
    assert [s.data_ptr() for s in eng._slots] == slots          # no slot grew ...
    assert torch.equal(b, eng0.lowres_logits(two)[0])
    torch.cuda.synchronize()
    ws_bytes = 2 * 36 * 2048 * 4                                # ... but the first shape's workspace went back
    guards = [torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device=cuda) for _ in range(8)]
    assert torch.equal(eng.lowres_logits(big)[0], a)
    assert torch.equal(eng.lowres_logits(two)[0], b)
    torch.cuda.synchronize()
    assert all(bool((g == 0x5A).all()) for g in guards)


@pytest.mark.parametrize("tag", ["psp_align_2x65x65", "v3p_align_2x65x65"])
def test_evaluation_drivers_run_on_an_engine(tag, tmp_path_factory, cuda):
    from dcfp_amd import evaluate as ev
    _, x, _, _, _, eng = _setup(tag, tmp_path_factory)
    xd = x.to(cuda)
    N, _, H, W = x.shape
    whole = ev.predict_whole(eng, xd)
    assert tuple(whole.shape) == (N, 19, H, W)
    slid = ev.predict_sliding(eng, xd, (49, 49), 19)
    assert tuple(slid.shape) == (N, 19, H, W) and torch.isfinite(slid).all()
    ms = ev.predict_multiscale(eng, xd, (49, 49), [0.75, 1.0], 19, True, eng.align_corner)
    assert tuple(ms.shape) == (N, 19, H, W) and torch.isfinite(ms).all()
    labels = ev.predict_labels(eng, xd)
    conf = ev.get_confusion_matrix(fill.closed_form_labels(N, H, W).to(cuda), labels, 19)
    assert tuple(conf.shape) == (19, 19) and int(conf.sum()) > 0


@pytest.mark.parametrize("model", ["psp", "deeplabv3p"])
def test_evaluate_tool_through_the_engine(model, tmp_path):
    snap = str(tmp_path / "snap")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), "--model", model, "--backbone", "resnet50",
           "--input-size", "65,65", "--whole", "True", "--batch-size", "2", "--num-images", "4", "--use-trt", "True",
           "--snapshot-dir", snap]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    recs = [json.loads(l) for l in open(os.path.join(snap, "result.txt")).read().splitlines() if l.startswith("{")]
    iou = recs[0]
    assert math.isfinite(iou["meanIU"]) and 0.0 <= iou["meanIU"] <= 1.0
    assert len(iou["IU_array"]) == 19 and all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in iou["IU_array"])
    assert recs[-1]["images"] == 2 and recs[-1]["FPS"] > 0
