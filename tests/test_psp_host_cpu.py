"""CPU: PSPNet (networks.psp) host side against the reference's own records (tests/golden/*psp*.npz): module tree and
state_dict, ignore_prune_layer, the static pruning graph (the pyramid concat whose last item is the layer4 residual
sum) and every mask bit of prune_model, the pruned weights, init_pruned_model's slim shapes, the complexity counter
(full and global_percent 0.5), and the header's pyramid pooling entry points."""
import os

import torch

import _model_cases as mc
from _model_cases import BB

TAG = "psp_r50_2x65x65"


def test_module_tree_matches_reference():
    m, g = mc.module_tree_check(TAG)
    assert m.ignore_prune_layer == ["backbone.layer4.2.bn3"]
    assert not hasattr(m, "get_prune_params")                    # (the reference's PSPNet has none)
    # the constructor's defaults (psp.py:14-24, ppm.py:15-25)
    assert m.backbone.out_index == [3, 4]
    assert tuple(m.ppm.bottleneck[0].weight.shape) == (512, 4096, 3, 3)
    assert isinstance(m.last_conv, torch.nn.Conv2d) and m.last_conv.bias is not None
    assert [st[0].output_size for st in m.ppm.stages] == [(1, 1), (2, 2), (3, 3), (6, 6)]
    para = dict(BB)
    build_args = dict(backbone="resnet50", backbone_para=para, num_classes=19)
    from dcfp_amd import networks
    networks.psp.Seg_Model(**build_args)
    assert para == BB                                            # the caller's dict is not mutated


def test_prune_model_matches_reference(tmp_path):
    cfg = mc.prune_model_check("psp", "pspr50", tmp_path)
    # the ragged pyramid widths the issue's reference run reports: 319 + 318 + 318 + 324 + the 2048 of layer4
    assert [cfg[f"ppm.stages.{k}.1"]["out_channels"] for k in range(4)] == [319, 318, 318, 324]
    assert cfg["ppm.bottleneck.0"]["in_channels"] == 3327 and cfg["ppm.bottleneck.0"]["raw_in_channels"] == 4096


def test_pruning_graph_concat_of_a_residual_sum():
    """The pyramid concat's last item is the layer4 residual sum: an item node of its own whose convs share one group
    (the reference's concat_*_item_* node), and the bottleneck conv's input space lists it after the four stages."""
    from dcfp_amd.pruners.channel_pruner import build_graph
    g = build_graph(mc.host_model("psp"))
    cat = g.node2parents["ppm.bottleneck.0"]
    assert len(cat) == 1 and cat[0].startswith("concat_")
    parents = g.node2parents[cat[0]]
    assert parents[:4] == [f"ppm.stages.{k}.1" for k in range(4)]
    assert parents[4] == cat[0] + "_item_4"
    assert sorted(g.node2parents[parents[4]]) == sorted(["backbone.layer4.2.conv3", "backbone.layer4.1.conv3",
                                                         "backbone.layer4.0.conv3", "backbone.layer4.0.downsample.0"])
    assert g.node2parents["last_conv"] == ["ppm.bottleneck.0"]


def test_flops_counter_matches_reference(tmp_path):
    mc.flops_counter_check("psp", "flops_psp.npz", "psp_r50", tmp_path)


def test_abi_declares_the_pyramid_pooling_entry_points():
    from dcfp_amd import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dcfp_hip.h")).read()
    for name in ("dcfp_ppm_pool_f32", "dcfp_ppm_pool_adjoint_f32", "dcfp_ppm_resize_adjoint_f32"):
        assert name in _lib.SIGNATURES
        assert name + "(" in src


def test_run_sequential_rejects_a_none_pool_size():
    import pytest
    from dcfp_amd.networks import _exec
    seq = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d((None, 3)))
    with pytest.raises(RuntimeError):
        _exec.run_sequential(seq, torch.zeros(1, 2, 5, 5))
