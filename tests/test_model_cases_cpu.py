"""CPU: the shared whole-model comparison (tests/_model_cases.py compare_to_golden) really asserts.  For every
whole-model fixture the reference's own fp32 record passes it - the bounds are multiples of exactly that run's distance
to fp64 - and each of five single-field corruptions makes it raise."""
import copy

import pytest

from _model_cases import CASES, compare_to_golden, load_golden


def _fp32_record(gold, case):
    g = gold
    return {"loss": float(g["loss32"]), "out_shapes": [(g.N, 19, g.H, g.W)] * 2,
            "logits": g.f32("logits"), "logits_ds": g.f32("logits_ds"),
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


@pytest.mark.parametrize("tag", list(CASES))
def test_comparator_accepts_the_reference_fp32_run_and_rejects_corruptions(tag):
    case, gold = CASES[tag], load_golden(tag)
    good = _fp32_record(gold, case)
    compare_to_golden(copy.deepcopy(good), gold, case)
    for corrupt in (_corrupt_loss, _corrupt_logit, _corrupt_norm, _corrupt_wgrad, _corrupt_running_mean):
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
