"""CPU: the shared whole-model comparison (tests/_model_cases.py compare_to_golden) really asserts.  For every
whole-model fixture the reference's own fp32 record passes it - the bounds are multiples of exactly that run's distance
to fp64 - and each of five single-field corruptions (six where the fixture holds eval-mode logits) makes it raise.
The same for the summaries-only comparison of a second input draw, and the input draws themselves."""
import copy
import json
import math

import pytest
import torch

from oracle import fill
from _model_cases import CASES, RECIPES, SECOND_DRAWS, compare_summaries_to_golden, compare_to_golden, load_golden, \
    module_tree_check


def _fp32_record(gold, case):
    g = gold
    evals = ("logits_eval", "logits_eval_ds") if case.eval_logits else ()
    return {"loss": float(g["loss32"]), "out_shapes": [(g.N, case.classes, g.H, g.W)] * 2,
            "logits": g.f32("logits"), "logits_ds": g.f32("logits_ds"), **{k: g.f32(k) for k in evals},
            "bgrad": g.f32(f"bgrad:{case.classifier}:"),
            "bn_wgrad": g.f32("bn_wgrad"), "bn_bgrad": g.f32("bn_bgrad"),
            "grad_l2": g["grad_l2:32"].copy(), "grad_proj": g["grad_proj:32"].copy(),
            "wgrad": {k: g.f32(f"wgrad:{k}:") for k in case.convs},
            "rm": {bn: g.f32(f"rm:{bn}:") for bn in case.running},
            "rv": {bn: g.f32(f"rv:{bn}:") for bn in case.running}}


def _corrupt_loss(rec, gold, case):
    l64, l32 = float(gold["loss64"]), float(gold["loss32"])
    rec["loss"] += 10 * max(1e-5 * abs(l64), 3 * abs(l32 - l64))


def _corrupt_logit(rec, gold, case):
    rec["logits"][0, 3, 1, 2] += 1.0


def _corrupt_norm(rec, gold, case):
    rec["grad_l2"][0] *= 2.0


def _corrupt_wgrad(rec, gold, case):
    rec["wgrad"][case.convs[-1]] *= -1.0


def _corrupt_running_mean(rec, gold, case):
    rec["rm"][case.running[-1]][0] += 1e-3


def _corrupt_eval_logit(rec, gold, case):
    rec["logits_eval_ds"][1, case.classes - 1, 2, 1] += 1.0


def _corrupt_bias_gradient(rec, gold, case):
    rec["bgrad"] = rec["bgrad"][::-1].copy()


@pytest.mark.parametrize("tag", list(CASES))
def test_comparator_accepts_the_reference_fp32_run_and_rejects_corruptions(tag):
    case, gold = CASES[tag], load_golden(tag)
    good = _fp32_record(gold, case)
    compare_to_golden(copy.deepcopy(good), gold, case)
    corruptions = (_corrupt_loss, _corrupt_logit, _corrupt_norm, _corrupt_wgrad, _corrupt_running_mean,
                   _corrupt_bias_gradient) + ((_corrupt_eval_logit,) if case.eval_logits else ())
    for corrupt in corruptions:
        rec = copy.deepcopy(good)
        corrupt(rec, gold, case)
        with pytest.raises(AssertionError):
            compare_to_golden(rec, gold, case)
    # (the corruptions left the good record as it was: it still passes)
    compare_to_golden(good, gold, case)


def test_running_statistics_rule_is_per_case():
    """Only PSPNet's fixture gets the relative rule; a 2e-5 slip of backbone.bn1's running mean fails everywhere else."""
    assert [t for t, c in CASES.items() if c.running_rel] == ["psp_r50_2x65x65"]
    for tag in ("v3_r50_2x65x65", "v3p_r50_2x65x65"):
        case, gold = CASES[tag], load_golden(tag)
        rec = _fp32_record(gold, case)
        rec["rm"]["backbone.bn1"] = gold["rm:backbone.bn1:64"] + 2e-5
        with pytest.raises(AssertionError):
            compare_to_golden(rec, gold, case)


@pytest.mark.parametrize("tag", list(SECOND_DRAWS))
def test_summaries_comparator_accepts_the_reference_fp32_run_and_rejects_corruptions(tag):
    gold = load_golden(tag)
    assert gold.phase == 1.0 and "logits32" not in gold.g.files
    good = {"loss": float(gold["loss32"]), "bn_wgrad": gold.f32("bn_wgrad"), "bn_bgrad": gold.f32("bn_bgrad"),
            "grad_l2": gold["grad_l2:32"].copy(), "grad_proj": gold["grad_proj:32"].copy()}
    compare_summaries_to_golden(copy.deepcopy(good), gold)

    def flip_bn(rec, gold, case):
        rec["bn_bgrad"] *= -1.0

    def swap_projections(rec, gold, case):
        rec["grad_proj"] = rec["grad_proj"][::-1].copy()
    for corrupt in (_corrupt_loss, _corrupt_norm, flip_bn, swap_projections):
        rec = copy.deepcopy(good)
        corrupt(rec, gold, None)
        with pytest.raises(AssertionError):
            compare_summaries_to_golden(rec, gold)
    # the second draw is another input: the first draw's record (same model, same labels) does not pass it
    first = load_golden(SECOND_DRAWS[tag])
    with pytest.raises(AssertionError):
        compare_summaries_to_golden(dict(good, loss=float(first["loss32"]), grad_l2=first["grad_l2:32"].copy(),
                                         grad_proj=first["grad_proj:32"].copy()), gold)


def test_input_phase_zero_is_the_input_of_every_earlier_fixture():
    """fill.closed_form_input(phase=0) bit for bit what it was before it took a phase (restated here), in both
    dtypes; phase 1 is another draw of the same distribution."""
    for (N, H, W), dtype in (((2, 65, 65), torch.float32), ((2, 96, 128), torch.float64), ((4, 64, 64), torch.float32)):
        n = N * 3 * H * W
        i = torch.arange(n, dtype=torch.float64)
        u = torch.sin((4.1414 * i + 0.77) % 6.283185307179586) * 43758.5453123
        u = u - torch.floor(u)
        was = (0.7 * torch.cos(0.0137 * i + 0.3).to(torch.float64)
               + 0.9 * ((u - 0.5) * (2.0 * math.sqrt(3.0)))).reshape(N, 3, H, W).to(dtype)
        assert torch.equal(fill.closed_form_input(N, H, W, dtype), was)
        assert torch.equal(fill.closed_form_input(N, H, W, dtype, phase=0.0), was)
        other = fill.closed_form_input(N, H, W, dtype, phase=1.0)
        assert other.shape == was.shape and other.dtype == dtype
        assert (other - was).abs().mean() > 0.5 and abs(float(other.std() / was.std()) - 1.0) < 0.05


@pytest.mark.parametrize("key", list(RECIPES))
def test_recipe_labels_hold_every_class(key):
    """The many-class CE backward runs its last, ragged chunk of classes on real labels: every class of the recipe
    occurs in the fixture's label map, and some pixels are ignored."""
    classes = RECIPES[key][0]
    gold = load_golden(f"v3_r50_{key}_2x96x128")
    lab = fill.closed_form_labels(gold.N, gold.H, gold.W, num_classes=classes)
    assert sorted(lab.unique().tolist()) == list(range(classes)) + [255]
    assert 0.01 < float((lab == 255).float().mean()) < 0.1
    assert int(gold["num_classes"]) == classes and gold["logits_eval32"].shape[:2] == (gold.N, classes)


def test_module_tree_of_a_recipe_case():
    """The product module tree at mg_unit [1, 1, 1] and 59 classes against the reference's (names, shapes, BatchNorm and
    parameter order): three layer4 blocks at dilation 4, both classifiers 59 wide."""
    m, g = module_tree_check("v3_r50_ctx_2x96x128")
    assert [b.conv2.dilation[0] for b in m.backbone.layer4] == [4, 4, 4]
    assert m.last_conv[6].out_channels == m.conv_deepsup[4].out_channels == int(g["num_classes"]) == 59
    assert json.loads(str(g["backbone_para"])) == CASES["v3_r50_ctx_2x96x128"].backbone_para
    assert [int(v) for v in g["meta"]] == [2, 96, 128, 0]
