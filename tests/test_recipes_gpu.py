"""GPU: the ADE20K, COCO-Stuff and Pascal-Context recipes as whole models.  DeepLabv3-R50 with align_corner False,
mg_unit [1, 1, 1] and 150 / 171 / 59 classes at 2 x 3 x 96 x 128 (even, not square; a 12 x 16 feature map) against
fixtures made from the reference itself (oracle/make_golden.py `ade` / `coco` / `ctx` / `ade:p1`), by the rules of the
Cityscapes cases (tests/_model_cases.py compare_to_golden, tests/_parity.py).  What composes differently here than
in every other whole-model case: align_corner False at the ASPP image-pool broadcast and at both heads' fused
upsample + CE, the chunked many-class CE backward with a ragged last chunk inside a real backward pass, classifier convs
and their dgrads 59 / 150 / 171 wide, three layer4 blocks at dilation 4 through the fused Bottleneck node, even sizes
through the stride-2 stem, the max-pool and the stride-2 stage, and the fp32 inference epilogue (eval-mode logits) at
those class counts."""
import pytest

import _model_cases as mc
from dcfp_amd import ops

pytestmark = pytest.mark.gpu
# key -> (chunks, classes in the last chunk) of the CE backward at a chunk width of 20
CE_CHUNKS = {"ade": (8, 10), "coco": (9, 11), "ctx": (3, 19)}


def _tag(key):
    return f"v3_r50_{key}_2x96x128"


def _is_the_recipe(key):
    """The assertions on the model about to run: it is the configuration the case claims to be."""
    case = mc.CASES[_tag(key)]
    chunks, tail = CE_CHUNKS[key]
    assert case.classes == mc.RECIPES[key][0] == 20 * (chunks - 1) + tail and 0 < tail < 20
    assert "cells_chunked" in ops.CE_BACKWARD_VARIANTS
    assert ops.ce_backward_plan(2, case.classes, 12, 16, 96, 128) == ("cells_chunked", 20, chunks)

    def check(m):
        assert [b.conv2.dilation[0] for b in m.backbone.layer4] == [4, 4, 4]
        assert m.align_corner is False and m.aspp.align_corner is False
        assert m.last_conv[6].out_channels == m.conv_deepsup[4].out_channels == case.classes
    return check


@pytest.mark.parametrize("key", list(mc.RECIPES))
def test_forward_backward_vs_reference_golden(cuda, capsys, key):
    """Loss, both heads' logits in training and in eval mode, every parameter gradient by norm (per tensor) and by
    projection (rank-wise), the stored weight gradients and the classifier's bias gradient, the BatchNorm gamma / beta
    gradients and backbone.bn1's running statistics."""
    mc.forward_backward_vs_golden(_tag(key), cuda, capsys, before=_is_the_recipe(key))


@pytest.mark.parametrize("key", ["ade_p1"])
def test_second_input_draw(cuda, capsys, key):
    """Every other whole-model case runs one draw of the input; ADE20K's recipe on a second one (phase 1 of
    fill.closed_form_input): loss, BatchNorm gradients, every parameter gradient by norm and by projection."""
    tag = _tag(key)
    assert mc.SECOND_DRAWS[tag] == _tag("ade") and mc.load_golden(tag).phase == 1.0
    mc.second_draw_vs_golden(tag, cuda, capsys)


@pytest.mark.parametrize("trait", ["align_corner", "mg_unit"])
def test_fixture_tells_the_recipes_apart(cuda, capsys, trait):
    """The product model with Cityscapes' align_corner True, or its mg_unit [1, 2, 4], forced on fails ADE20K's
    fixture: if it passed, the fixture could not tell whether the flag reaches the three bilinear sites, or which
    dilations layer4 runs at."""
    def check(m):
        if trait == "align_corner":
            assert m.align_corner is True and m.aspp.align_corner is True
        else:
            assert [b.conv2.dilation[0] for b in m.backbone.layer4] == [4, 8, 16] and m.align_corner is False
    other = {"align": True} if trait == "align_corner" else {"backbone_para": mc.BB}
    rec, gold, case = mc.golden_record(_tag("ade"), cuda, before=check, **other)
    assert gold.align == 0 and case.backbone_para["mg_unit"] == [1, 1, 1]
    with pytest.raises(AssertionError) as failure:
        mc.compare_to_golden(rec, gold, case)
    with capsys.disabled():
        print("\n[%s with Cityscapes' %s] rejected: %s" % (gold.tag, trait, str(failure.value).splitlines()[0][:200]))
