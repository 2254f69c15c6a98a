"""Host side of the baseline pruning criteria (dcfp_amd/pruners/baseline_pruner.py), no GPU:
normalize_scores against hand values, ScorePruner against DCFPPruner on one score file, the score-file format with its
extra keys, the host-side refusals of the new C entry points and of tools/train.py's arguments."""
import ctypes
import importlib
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dcfp_amd import _lib, networks, pruners  # noqa: E402
from dcfp_amd.pruners.baseline_pruner import linked_convs, scored_bn_names  # noqa: E402


def test_normalize_scores_hand_values():
    eic = {"a": torch.tensor([3.0, 4.0]), "z": torch.zeros(3), "m": torch.tensor([1.0, 2.0, 3.0, 6.0])}
    none = pruners.normalize_scores(eic, "none")
    assert set(none) == set(eic) and all(torch.equal(none[k], eic[k]) for k in eic)
    l2 = pruners.normalize_scores(eic, "l2")
    assert torch.equal(l2["a"], torch.tensor([3.0 / 5.0, 4.0 / 5.0], dtype=torch.float64).float())
    assert torch.equal(l2["z"], torch.zeros(3)) and l2["z"].dtype == torch.float32
    want = torch.tensor([1.0, 2.0, 3.0, 6.0], dtype=torch.float64) / 50.0 ** 0.5
    assert torch.equal(l2["m"], want.float())
    mean = pruners.normalize_scores(eic, "mean")
    assert torch.equal(mean["a"], torch.tensor([3.0 / 3.5, 4.0 / 3.5], dtype=torch.float64).float())
    assert torch.equal(mean["m"], torch.tensor([1.0 / 3.0, 2.0 / 3.0, 1.0, 2.0], dtype=torch.float64).float())
    assert torch.equal(mean["z"], torch.zeros(3))
    assert all(v.dtype == torch.float32 for d in (l2, mean) for v in d.values())
    assert torch.equal(eic["a"], torch.tensor([3.0, 4.0]))                  # the input is left alone
    with pytest.raises(ValueError):
        pruners.normalize_scores(eic, "max")


@pytest.fixture(scope="module")
def model_and_scores(tmp_path_factory):
    """networks.simple R50 on the CPU with a seeded random score per scored BN channel, saved with the extra keys."""
    torch.manual_seed(7)
    m = networks.simple.Seg_Model(backbone="resnet50", backbone_para={"pretrained": False}, num_classes=19, deepsup=True)
    mods = dict(m.named_modules())
    g = torch.Generator().manual_seed(11)
    eic = {n: torch.rand(mods[n].weight.numel(), generator=g) for n in scored_bn_names(m)}
    d = tmp_path_factory.mktemp("score")
    plain, extra = str(d / "plain.pth"), str(d / "extra.pth")
    torch.save({"eic": eic}, plain)
    torch.save({"eic": eic, "criterion": "taylor", "steps": 2}, extra)
    return m, eic, plain, extra


def test_scored_layers_are_linked_to_a_conv(model_and_scores):
    m, eic, _, _ = model_and_scores
    assert list(eic) == list(pruners.dcfp_pruning(m).state_dict["eic"])
    convs = linked_convs(m, list(eic))
    mods = dict(m.named_modules())
    assert all(mods[convs[n]].weight.shape[0] == eic[n].numel() for n in eic)


def _masks(pruner, model):
    import copy
    sub, cfg = pruner.prune_model(copy.deepcopy(model), except_start_keys=["conv_deepsup"])
    return {k: v["out_mask"] for k, v in cfg.items() if "out_mask" in v}


def test_score_pruner_none_equals_dcfp_pruner_and_extra_keys_load(model_and_scores):
    m, eic, plain, extra = model_and_scores
    ref = _masks(pruners.DCFPPruner(global_percent=0.5, layer_keep=0.02, score_file=plain), m)
    mine = _masks(pruners.ScorePruner(global_percent=0.5, layer_keep=0.02, score_file=plain, score_norm="none"), m)
    assert set(ref) == set(mine) and all((ref[k] == mine[k]).all() for k in ref)
    assert any(v.sum() < v.size for v in ref.values())                       # something was cut
    loaded = _masks(pruners.DCFPPruner(global_percent=0.5, layer_keep=0.02, score_file=extra), m)   # reads "eic" alone
    assert all((ref[k] == loaded[k]).all() for k in ref)
    # a per-layer norm changes the cut: the thresholds are global, the layers have different widths
    l2 = _masks(pruners.ScorePruner(global_percent=0.5, layer_keep=0.02, score_file=plain, score_norm="l2"), m)
    assert any((ref[k] != l2[k]).any() for k in ref)


def test_new_entry_points_reject_a_null_table_on_the_host():
    L = _lib.lib()
    bad, ok = _lib.E_BADDESC, 0
    assert L.dcfp_gate_taylor_f32(None, 3, None) == bad and L.dcfp_gate_taylor_f32(None, 0, None) == ok
    assert L.dcfp_gate_taylor_f32(None, -1, None) == bad
    assert L.dcfp_gate_l1reg_f32(None, 3, 1e-4, None) == bad and L.dcfp_gate_l1reg_f32(None, 0, 1e-4, None) == ok
    assert L.dcfp_filter_reduce_f32(None, 2, 5, _lib.FILTER_L2, None) == bad
    assert L.dcfp_filter_reduce_f32(None, 0, 0, _lib.FILTER_L2, None) == ok
    dummy = ctypes.c_void_p(256)                                             # never dereferenced: refused before any launch
    assert L.dcfp_filter_reduce_f32(dummy, 1, 1, 3, None) == bad             # unknown op
    assert L.dcfp_filter_reduce_f32(dummy, 1, -1, 0, None) == bad
    assert L.dcfp_fpgm_f32(None, 2, 4, None, 0, None) == bad and L.dcfp_fpgm_f32(None, 0, 0, None, 0, None) == ok
    assert L.dcfp_fpgm_f32(dummy, 1, 1, None, 0, None) == _lib.E_WORKSPACE
    # the host-side halves of the split rule and of the workspace
    units = L.dcfp_filter_reduce_units
    assert [units(64, 27), units(3, 64), units(3, 65), units(7, 576), units(2, 2304), units(1, 18432)] == [2, 1, 1, 2, 2, 1]
    assert units(33, 32) == 2 and units(17, 128) == 2 and units(5, 1024) == 2 and units(5, 1025) == 5
    assert units(0, 8) == 0 and units(8, 0) == 0
    assert L.dcfp_fpgm_workspace_bytes(0) == 0 and L.dcfp_fpgm_workspace_bytes(1) == 256
    assert L.dcfp_fpgm_workspace_bytes(130) == 3 * 130 * 4 + (256 - 3 * 130 * 4 % 256)


def test_train_tool_refuses_bad_scoring_arguments_before_building():
    train = importlib.import_module("train")
    parse = train.get_parser().parse_args
    for good in (["--prune-type", "taylor"], ["--prune-type", "taylor_w"], ["--prune-type", "dcfp"], [],
                 ["--slim-lambda", "1e-4"]):
        train.check_args(parse(good))
    with pytest.raises(ValueError, match="taylor"):
        train.check_args(parse(["--prune-type", "taylor_x"]))
    with pytest.raises(ValueError, match="slim-lambda"):
        train.check_args(parse(["--slim-lambda", "-1"]))
    with pytest.raises(ValueError):
        pruners.taylor_pruning(None, mode="filter")                          # refused before the model is looked at


def test_scorers_need_the_device(model_and_scores):
    m = model_and_scores[0]
    with pytest.raises(RuntimeError):
        pruners.weight_scores(m, "l1")
    with pytest.raises(ValueError):
        pruners.weight_scores(m, "l3")
    tp = pruners.taylor_pruning(m, "gate")
    with pytest.raises(RuntimeError):
        tp.step(m)
    with pytest.raises(RuntimeError):
        pruners.slimming_regularizer(m, 1e-4).step(m)
