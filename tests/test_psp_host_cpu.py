"""CPU: PSPNet (networks.psp) host side against the reference's own records (tests/golden/*psp*.npz): module tree and
state_dict, ignore_prune_layer, the static pruning graph (the pyramid concat whose last item is the layer4 residual
sum) and every mask bit of prune_model, the pruned weights, init_pruned_model's slim shapes, the complexity counter
(full and global_percent 0.5), and the header's pyramid pooling entry points."""
import copy
import os
import tempfile

import numpy as np
import torch

from oracle import fill
from oracle.make_scores import synthetic_scores

G = os.path.join(os.path.dirname(__file__), "golden")
BB = {"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128, "pretrained": False}


def build(deepsup=True):
    from dcfp_amd import networks
    m = networks.psp.Seg_Model(backbone="resnet50", backbone_para=dict(BB), num_classes=19, align_corner=True,
                               deepsup=deepsup)
    m.load_state_dict(fill.closed_form_state(m.state_dict()))
    return m


def test_module_tree_matches_reference():
    g = np.load(os.path.join(G, "model_psp_r50_2x65x65.npz"))
    m = build()
    sd = m.state_dict()
    assert list(sd.keys()) == g["state_keys"].tolist()
    assert [str(tuple(v.shape)) for v in sd.values()] == g["state_shapes"].tolist()
    assert m.ignore_prune_layer == g["ignore_prune_layer"].tolist() == ["backbone.layer4.2.bn3"]
    assert [n for n, p in m.named_parameters()] == g["param_names"].tolist()
    bns = [n for n, mod in m.named_modules() if isinstance(mod, torch.nn.BatchNorm2d)]
    assert bns == g["bn_names"].tolist()
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
    g = np.load(os.path.join(G, "prune_pspr50_gp50.npz"))
    from dcfp_amd import pruners
    from dcfp_amd.pruners.dcfp_pruner import DCFPPruner
    m = build()
    score = str(tmp_path / "score.pth")
    torch.save({"eic": synthetic_scores(m)}, score)
    pruner = DCFPPruner(global_percent=0.5, layer_keep=0.02, score_file=score)
    pruned, cfg = pruner.prune_model(copy.deepcopy(m), except_start_keys=["conv_deepsup"])

    assert dict(zip(g["norm_conv_bn"].tolist(), g["norm_conv_conv"].tolist())) == pruner.norm_conv_links
    assert sorted(g["except_layers"].tolist()) == sorted(pruner.except_layers)
    assert sorted(g["groups"].tolist()) == sorted(",".join(sorted(v)) for v in pruner.same_out_channel_groups.values())
    th = pruner.get_thresh()
    assert np.array_equal(np.array([float(th[0]), float(th[1])], dtype=np.float32), g["thresh"])

    assert list(cfg.keys()) == g["names"].tolist()
    for name, c in cfg.items():
        for kind in ("in", "out"):
            if kind + "_mask" in c:
                ref = np.unpackbits(g[f"{kind}:{name}"])[:c[f"raw_{kind}_channels"]]
                assert np.array_equal(c[kind + "_mask"].reshape(-1).astype(np.uint8), ref), (name, kind)
                assert [c[kind + "_channels"], c[f"raw_{kind}_channels"]] == g[f"{kind}_n:{name}"].tolist()
    # the ragged pyramid widths the issue's reference run reports: 319 + 318 + 318 + 324 + the 2048 of layer4
    assert [cfg[f"ppm.stages.{k}.1"]["out_channels"] for k in range(4)] == [319, 318, 318, 324]
    assert cfg["ppm.bottleneck.0"]["in_channels"] == 3327 and cfg["ppm.bottleneck.0"]["raw_in_channels"] == 4096

    sd = pruned.state_dict()
    assert list(sd.keys()) == g["pruned_keys"].tolist()
    assert [str(tuple(v.shape)) for v in sd.values()] == g["pruned_shapes"].tolist()
    sums = np.array([float(v.double().sum()) for v in sd.values()])
    abss = np.array([float(v.double().abs().sum()) for v in sd.values()])
    assert np.allclose(sums, g["pruned_sum"], rtol=1e-9, atol=1e-9)
    assert np.allclose(abss, g["pruned_abs"], rtol=1e-9, atol=1e-9)

    slim = build()
    pruners.init_pruned_model(slim, cfg)
    assert [str(tuple(v.shape)) for v in slim.state_dict().values()] == g["slim_shapes"].tolist()
    slim.load_state_dict(sd)


def test_pruning_graph_concat_of_a_residual_sum():
    """The pyramid concat's last item is the layer4 residual sum: an item node of its own whose convs share one group
    (the reference's concat_*_item_* node), and the bottleneck conv's input space lists it after the four stages."""
    from dcfp_amd.pruners.channel_pruner import build_graph
    g = build_graph(build())
    cat = g.node2parents["ppm.bottleneck.0"]
    assert len(cat) == 1 and cat[0].startswith("concat_")
    parents = g.node2parents[cat[0]]
    assert parents[:4] == [f"ppm.stages.{k}.1" for k in range(4)]
    assert parents[4] == cat[0] + "_item_4"
    assert sorted(g.node2parents[parents[4]]) == sorted(["backbone.layer4.2.conv3", "backbone.layer4.1.conv3",
                                                         "backbone.layer4.0.conv3", "backbone.layer4.0.downsample.0"])
    assert g.node2parents["last_conv"] == ["ppm.bottleneck.0"]


def test_flops_counter_matches_reference():
    g = np.load(os.path.join(G, "flops_psp.npz"))
    from dcfp_amd import networks, pruners
    from dcfp_amd.pruners.dcfp_pruner import DCFPPruner
    from dcfp_amd.utils.flops_counter import get_model_complexity_info
    m = networks.psp.Seg_Model(backbone="resnet50", backbone_para=dict(BB), num_classes=19, align_corner=True,
                               deepsup=False)
    f, p = get_model_complexity_info(m, (3, 257, 257), print_per_layer_stat=False, as_strings=False)
    assert float(f) == float(g["flops:psp_r50"]) and float(p) == float(g["params:psp_r50"])
    assert list(get_model_complexity_info(m, (3, 257, 257), print_per_layer_stat=False)) == g["str:psp_r50"].tolist()
    m = build()
    with tempfile.TemporaryDirectory() as d:
        torch.save({"eic": synthetic_scores(m)}, d + "/score.pth")
        pr = DCFPPruner(global_percent=0.5, layer_keep=0.02, score_file=d + "/score.pth")
        _, cfg = pr.prune_model(copy.deepcopy(m), except_start_keys=["conv_deepsup"])
    slim = networks.psp.Seg_Model(backbone="resnet50", backbone_para=dict(BB), num_classes=19, align_corner=True,
                                  deepsup=False)
    pruners.init_pruned_model(slim, cfg)
    f, p = get_model_complexity_info(slim, (3, 257, 257), print_per_layer_stat=False, as_strings=False)
    assert float(f) == float(g["flops:psp_r50_gp50"]) and float(p) == float(g["params:psp_r50_gp50"])


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
