"""Host side of the distillation fine-tune, no GPU: the reference formulas of tests/_kd_ref.py against an
independent statement, the `kd` criterion's construction and errors, the C-ABI's argument checks, the driver's flag
check and the random pruner's mask rule."""
import copy
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kd_ref as kr  # noqa: E402


class _DS:
    ignore_label = 255
    num_classes = 19
    class_weights = None


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("mode", kr.MODES)
@pytest.mark.parametrize("T", [1.0, 4.0])
def test_reference_agrees_with_kl_div(mode, T):
    from dcfp_amd import ops
    assert set(kr.MODES) == set(ops.KD_MODES)          # the reference states every mode the product offers
    N, Cc, h, w = 2, 5, 3, 7
    s, t = kr.logits((N, Cc, h, w), 11)
    loss, grad = kr.kd_ref(s, t, T, mode, torch.float64)
    s64, t64 = s.double(), t.double()
    if mode == "pixel":
        dim, count = 1, N * h * w
    else:
        s64, t64, dim, count = s64.reshape(N, Cc, -1), t64.reshape(N, Cc, -1), 2, N * Cc
    want = F.kl_div(F.log_softmax(s64 / T, dim=dim), F.softmax(t64 / T, dim=dim), reduction="sum") * T * T / count
    assert abs(float(loss) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    # dL/ds = T / count * (softmax(s/T) - softmax(t/T))
    gwant = (F.softmax(s64 / T, dim=dim) - F.softmax(t64 / T, dim=dim)).reshape(N, Cc, h, w) * T / count
    assert float((grad - gwant).abs().max()) <= 1e-14
    assert float(loss) > 0


def test_reference_degenerate_cases_are_zero():
    from dcfp_amd import ops
    assert set(kr.MODES) == set(ops.KD_MODES)
    s, t = kr.logits((2, 1, 3, 5), 3)
    loss, grad = kr.kd_ref(s, t, 1.0, "pixel", torch.float64)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    s, t = kr.logits((2, 3, 1, 1), 3)
    loss, grad = kr.kd_ref(s, t, 2.0, "channel", torch.float64)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the criterion
def test_combined_criterion_builds():
    from dcfp_amd.loss.criterion import CombinedCriterion, CriterionDSN, CriterionGsrlDSN, CriterionKD, build_criterions
    para = {"ds_weight": 0.4, "kd_weight": 0.5, "kd_T": 2.0, "kd_mode": "channel"}
    crit = build_criterions("ce,kd", _DS(), para)
    assert isinstance(crit, CombinedCriterion)
    assert [type(c) for c in crit.criterions] == [CriterionDSN, CriterionKD]
    kd = crit.criterions[1]
    assert (kd.kd_weight, kd.kd_T, kd.kd_mode) == (0.5, 2.0, "channel")
    assert [type(c) for c in build_criterions("gsrl,kd", _DS(), {}).criterions] == [CriterionGsrlDSN, CriterionKD]
    alone = build_criterions("kd", _DS(), {})
    assert isinstance(alone, CriterionKD) and (alone.kd_weight, alone.kd_T, alone.kd_mode) == (1.0, 1.0, "pixel")
    with pytest.raises(ValueError, match="kd_mode"):
        build_criterions("kd", _DS(), {"kd_mode": "spatial"})
    with pytest.raises(ValueError, match="kd_T"):
        build_criterions("kd", _DS(), {"kd_T": 0.0})


def test_criterion_errors_name_the_teacher_and_the_shapes():
    from dcfp_amd.loss.criterion import build_criterions
    kd = build_criterions("kd", _DS(), {})
    z = torch.zeros(2, 19, 9, 9)
    lab = torch.zeros(2, 65, 65, dtype=torch.int64)
    for labels in (lab, {"ori": lab}):
        with pytest.raises(ValueError, match="teacher"):
            kd.forward_lowres([z], labels, (65, 65), True)
        with pytest.raises(ValueError, match="teacher"):
            kd([z], labels)
    bad = {"ori": lab, "teacher": torch.zeros(2, 19, 9, 17)}
    for call in (lambda: kd.forward_lowres([z], bad, (65, 65), True), lambda: kd([z], bad)):
        with pytest.raises(ValueError) as e:
            call()
        assert "(2, 19, 9, 17)" in str(e.value) and "(2, 19, 9, 9)" in str(e.value)


def test_kd_loss_has_no_cpu_path():
    from dcfp_amd import ops
    s, t = kr.logits((1, 3, 2, 2), 0)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.kd_loss(s, t)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.kd_loss(s.requires_grad_(True), t, T=2.0, mode="channel")


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_abi_argument_errors_need_no_gpu():
    from dcfp_amd import _lib
    L = _lib.lib()
    BAD, WS = _lib.E_BADDESC, _lib.E_WORKSPACE
    p = C.c_void_p(4096)                     # never dereferenced: every call below returns before any HIP call

    def call(s=p, t=p, mode=0, N=2, Cc=19, h=9, w=9, T=1.0, ws=p, nbytes=1 << 20, out=p, dl=None):
        return L.dcfp_kd_fwd_f32(s, t, mode, N, Cc, h, w, T, ws, nbytes, out, dl, None)

    assert call(s=None) == BAD and call(t=None) == BAD and call(out=None) == BAD
    for key in ("N", "Cc", "h", "w"):
        assert call(**{key: 0}) == BAD and call(**{key: -3}) == BAD
    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert call(T=T) == BAD
    assert call(mode=2) == BAD and call(mode=-1) == BAD
    for mode, need in ((0, 4 * ((2 * 9 * 9 + 63) // 64)), (1, 4 * 2 * 19)):
        assert L.dcfp_kd_workspace_bytes(mode, 2, 19, 9, 9) == need
        assert call(mode=mode, nbytes=need - 1) == WS
        assert call(mode=mode, ws=None, nbytes=need) == WS
    assert L.dcfp_kd_workspace_bytes(0, 0, 19, 9, 9) == 0 and L.dcfp_kd_workspace_bytes(5, 2, 19, 9, 9) == 0


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_refuses_kd_without_a_teacher(monkeypatch, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    built = []
    monkeypatch.setattr(train, "build_criterions", lambda *a, **k: built.append(a))
    with pytest.raises(ValueError, match="--teacher-from"):
        train.main(["--loss-type", "ce,kd", "--ddp", "False", "--snapshot-dir", str(tmp_path / "snap")])
    assert built == [] and not (tmp_path / "snap").exists()      # refused before anything was built or written
    args = train.get_parser().parse_args(["--loss-type", "gsrl,kd", "--teacher-from", "dense.pth"])
    train.check_args(args)
    assert args.teacher_engine is True and args.teacher_channel_cfg is None
    train.check_args(train.get_parser().parse_args(["--loss-type", "ce"]))


# ------------------------------------------------------------------------------------------------ the random pruner
def test_random_mask_rule():
    from dcfp_amd.pruners.random_pruner import random_out_masks
    links = {"a.bn": "a.conv", "b.bn": "b.conv", "c.bn": "c.conv", "d.bn": "d.conv"}
    channels = {"a.bn": 64, "b.bn": 300, "c.bn": 7, "d.bn": 40}
    gen = torch.Generator().manual_seed(5)
    masks = random_out_masks(links, ["c.conv"], channels, 0.6, 0.02, gen)
    assert list(masks) == ["a.conv", "b.conv", "d.conv"]                  # the excepted layer gets no mask
    gen = torch.Generator().manual_seed(5)
    for bn, conv in links.items():
        if conv == "c.conv":
            continue
        want = (torch.rand(channels[bn], generator=gen) > 0.6).float()    # keep rand > global_percent
        assert torch.equal(masks[conv], want) and 0 < int(want.sum()) < channels[bn]
    # nothing survives the draw: the first max(1, int(C * layer_keep)) channels stay
    masks = random_out_masks(links, [], channels, 1.0, 0.02, torch.Generator().manual_seed(5))
    for bn, conv in links.items():
        n = channels[bn]
        keep = max(1, int(n * 0.02))
        assert keep == {64: 1, 300: 6, 7: 1, 40: 1}[n]
        assert int(masks[conv].sum()) == keep and bool((masks[conv][:keep] == 1).all())


def test_random_pruner_prunes_a_model():
    from dcfp_amd import networks, pruners
    BB = {"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128, "pretrained": False}

    def bare():
        torch.manual_seed(0)
        return networks.deeplabv3.Seg_Model(backbone="resnet50", backbone_para=dict(BB), num_classes=19,
                                            align_corner=True, deepsup=True)
    m = bare()
    cfgs = []
    for seed in (3, 3, 4):
        pruner = pruners.RandomChannelPruner(global_percent=0.5, layer_keep=0.02, seed=seed)
        pruned, cfg = pruner.prune_model(copy.deepcopy(m), except_start_keys=["conv_deepsup"])
        cfgs.append(cfg)
    for name in pruner.except_layers:                                     # excepted layers keep every output channel
        assert cfg[name]["out_channels"] == cfg[name]["raw_out_channels"], name
    assert "aspp.conv1" in pruner.except_layers and "conv_deepsup.0" in pruner.except_layers
    c = cfg["backbone.layer1.0.conv1"]                                    # a conv outside every residual group
    assert 0.25 * c["raw_out_channels"] < c["out_channels"] < 0.75 * c["raw_out_channels"]
    same = [all((cfgs[0][k]["out_mask"] == cfgs[i][k]["out_mask"]).all() for k in cfgs[0]) for i in (1, 2)]
    assert same == [True, False]                                          # a seed repeats the cut, another changes it
    slim = bare()
    pruners.init_pruned_model(slim, cfg)
    slim.load_state_dict(pruned.state_dict())
