"""GPU: the frozen fp16 engine (dcfp_amd/deploy.py) as a whole model.

The yardstick is computed here on the CPU and never uses the code under test (tests/_deploy_ref.py): the fp64
eval-mode logits of the oracle, and an fp16-storage emulation of the same forward run twice (convolutions summed in
fp64 and in fp32).  e / r = the larger of the two emulations' max-abs / relative-L2 distances to the fp64 logits.
Acceptance of the engine's low-resolution logits against fp64: relative L2 <= 1.5 r, max-abs <= 3 e (the two
summation orders already differ by about e and the GPU's order is a third; relative L2 is the stable statistic and gets
the narrow margin).  Labels: predict_labels(engine, x) equals the fp64 argmax at every pixel whose low-resolution fp64
top-2 margin is at least 6 e - compared where the align_corners grid of the full-resolution map coincides with a
low-resolution pixel - and at most 10 % of the pixels may be left out."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _deploy_ref as dref  # noqa: E402
import _model_cases as mc  # noqa: E402
from oracle import fill, model as omodel  # noqa: E402

pytestmark = pytest.mark.gpu

_SIZES = {"v3_r50_2x65x65": (2, 65, 65), "simple_r50_4x64x64": (4, 64, 64)}
_cache = {}


def _full(tag):
    """(eval-mode model on the CPU, input, oracle Cfg) of a whole-model case: closed-form weights and input."""
    case = mc.CASES[tag]
    m = mc.build_model(case.model, case.backbone, True, torch.device("cpu"), criterion=False).eval()
    return m, fill.closed_form_input(*_SIZES[tag]), omodel.Cfg(case.model, case.backbone, align_corner=True, deepsup=False)


def _slim(tmp):
    """The v3-R50 slimmed as slim_model_logits_check does: global_percent 0.5 on the prune_v3r50_gp50 scores."""
    from dcfp_amd import pruners
    g = np.load(os.path.join(mc.G, "prune_v3r50_gp50.npz"))
    cpu = torch.device("cpu")
    m = mc.build_model("deeplabv3", "resnet50", True, cpu, criterion=False)
    _, pruned, cfg = mc._prune_gp50(m, os.path.join(tmp, "score.pth"))
    assert list(cfg.keys()) == g["names"].tolist()
    slim = mc.build_model("deeplabv3", "resnet50", True, cpu, criterion=False)
    pruners.init_pruned_model(slim, cfg)
    slim.load_state_dict(pruned.state_dict())
    return slim.eval(), fill.closed_form_input(2, 65, 65), omodel.Cfg("deeplabv3", "resnet50", align_corner=True, deepsup=False)


def _setup(tag, tmp_path_factory):
    """Per case, once: model, input, the CPU yardstick (ref64, e, r) and the engine on the GPU."""
    if tag not in _cache:
        from dcfp_amd import deploy
        m, x, cfg = _slim(str(tmp_path_factory.mktemp("slim"))) if tag == "slim" else _full(tag)
        ref, e, r = dref.yardstick(m.state_dict(), x, cfg)
        eng = deploy.freeze(m).to("cuda:0")
        _cache[tag] = (m, x, ref, e, r, eng)
    return _cache[tag]


def _compare(tag, tmp_path_factory, cuda):
    from dcfp_amd import evaluate as ev
    m, x, ref, e, r, eng = _setup(tag, tmp_path_factory)
    xd = x.to(cuda)
    low = eng.lowres_logits(xd)[0]
    assert low.dtype == torch.float32 and tuple(low.shape) == tuple(ref.shape)
    got = low.double().cpu()
    rel = float((got - ref).norm() / ref.norm())
    err = float((got - ref).abs().max())
    print(f"deploy {tag}: yardstick e {e:.4f} r {r:.3e} (|logits| <= {float(ref.abs().max()):.0f}); "
          f"engine max-abs {err:.4f} rel-L2 {rel:.3e}")
    assert torch.isfinite(got).all()
    assert rel <= 1.5 * r, (rel, r)
    assert err <= 3 * e, (err, e)

    labels = ev.predict_labels(eng, xd)
    H, W = x.shape[2:]
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
    full = eng(xd)
    assert isinstance(full, list) and tuple(full[0].shape) == (x.shape[0], 19, H, W) and full[0].dtype == torch.float32


@pytest.mark.parametrize("tag", list(_SIZES))
def test_engine_logits_and_labels_against_fp64(tag, tmp_path_factory, cuda, capsys):
    with capsys.disabled():
        _compare(tag, tmp_path_factory, cuda)


def test_slim_engine_logits_and_labels_against_fp64(tmp_path_factory, cuda, capsys):
    m = _setup("slim", tmp_path_factory)[0]
    widths = [c.out_channels for c in m.modules() if isinstance(c, torch.nn.Conv2d)]
    assert any(c % 8 for c in widths), widths
    with capsys.disabled():
        _compare("slim", tmp_path_factory, cuda)


def test_saved_engine_gives_bit_identical_logits(tmp_path_factory, tmp_path, cuda):
    from dcfp_amd import deploy
    _, x, _, _, _, eng = _setup("v3_r50_2x65x65", tmp_path_factory)
    xd = x.to(cuda)
    a = eng.lowres_logits(xd)[0].clone()
    again = deploy.load_engine(eng.state_dict(), cuda)
    assert torch.equal(again.lowres_logits(xd)[0], a)
    path = str(tmp_path / "engine.pth")
    torch.save(eng.state_dict(), path)
    assert torch.equal(deploy.load_engine(path, cuda).lowres_logits(xd)[0], a)
    assert torch.equal(eng.lowres_logits(xd)[0], a)              # buffers reused across calls: same bits
    small = eng.lowres_logits(xd[:1, :, :33, :41])[0]             # another input shape, then the first one again
    assert tuple(small.shape) == (1, 19, 5, 6)
    assert torch.equal(eng.lowres_logits(xd)[0], a)


def test_evaluation_drivers_run_on_an_engine(tmp_path_factory, cuda):
    from dcfp_amd import evaluate as ev
    _, x, _, _, _, eng = _setup("v3_r50_2x65x65", tmp_path_factory)
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


def test_returning_to_a_shape_after_the_workspace_grew(tmp_path_factory, cuda):
    """More images on a smaller map need a larger average-pool workspace while no activation slot grows.  The launch
    list of the first shape must not keep the old workspace: same bits on return, and memory handed back to the
    allocator (re-allocated here and filled with a pattern) stays untouched."""
    from dcfp_amd import deploy
    _, x, _, _, _, eng0 = _setup("v3_r50_2x65x65", tmp_path_factory)
    eng = deploy.load_engine(eng0.state_dict(), cuda)          # a fresh engine: nothing allocated yet
    xd = x.to(cuda)
    one = xd[:1].contiguous()                                   # 1 x 65 x 65
    a = eng.lowres_logits(one)[0].clone()
    slots = [s.data_ptr() for s in eng._slots]
    two = xd[:, :, :41, :41].contiguous()                       # 2 x 41 x 41: fewer pixels in every buffer, N doubled
    b = eng.lowres_logits(two)[0].clone()
    assert [s.data_ptr() for s in eng._slots] == slots          # no slot grew ...
    torch.cuda.synchronize()
    ws_bytes = 1 * 2048 * 4                                     # ... but the first shape's workspace went back
    guards = [torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device=cuda) for _ in range(16)]
    assert torch.equal(eng.lowres_logits(one)[0], a)
    assert torch.equal(eng.lowres_logits(two)[0], b)
    torch.cuda.synchronize()
    assert all(bool((g == 0x5A).all()) for g in guards)
    assert torch.equal(eng0.lowres_logits(one)[0], a)


def test_engine_refuses_an_image_on_another_device(tmp_path_factory, cuda):
    _, x, _, _, _, eng = _setup("v3_r50_2x65x65", tmp_path_factory)
    with pytest.raises(RuntimeError):
        eng.lowres_logits(x)                                    # a CPU image
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="cuda:1"):
            eng.lowres_logits(x.to("cuda:1"))
