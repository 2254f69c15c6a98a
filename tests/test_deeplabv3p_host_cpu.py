"""CPU: DeepLabv3+ (networks.deeplabv3p) host side against the reference's own records (tests/golden/*v3p*.npz):
module tree and state_dict, ignore_prune_layer, the static pruning graph and every mask bit of prune_model, the pruned
weights, init_pruned_model's slim shapes, and the complexity counter (full and global_percent 0.5)."""
import _model_cases as mc

TAG = "v3p_r50_2x65x65"


def test_module_tree_matches_reference():
    m, g = mc.module_tree_check(TAG)
    bns = g["bn_names"].tolist()
    prunable = [p for p in m.get_prune_params()]
    mods = dict(m.named_modules())
    assert [id(p) for p in prunable] == [id(mods[n].weight) for n in bns if n not in m.ignore_prune_layer]
    # the constructor's defaults (deeplabv3p.py:56-62): the layer1 tap and the 1x1 256 -> 48 conv that reads it
    assert m.backbone.out_index == [1, 3, 4]
    assert tuple(m.decoder.conv1.weight.shape) == (48, 256, 1, 1)
    assert tuple(m.decoder.last_conv[0].weight.shape) == (256, 560, 3, 3)


def test_prune_model_matches_reference(tmp_path):
    cfg = mc.prune_model_check("deeplabv3p", "v3pr50", tmp_path)
    assert len(cfg) == 132
    # the ragged decoder widths the issue's reference run reports
    assert cfg["decoder.conv1"]["in_channels"] == 175
    assert cfg["decoder.last_conv.0"]["out_channels"] == 146 and cfg["decoder.last_conv.3"]["out_channels"] == 147


def test_flops_counter_matches_reference(tmp_path):
    mc.flops_counter_check("deeplabv3p", "flops_v3p.npz", "v3p_r50", tmp_path)


def test_abi_declares_the_resize_entry_points():
    from dcfp_amd import _lib
    for name in ("dcfp_resize_bilinear_into_f32", "dcfp_resize_bilinear_adjoint_f32"):
        assert name in _lib.SIGNATURES
