"""CPU: dcfp_amd.deploy plans and packs without a device - record count, packed weights against fp16(w * scale) with
zero padding, what is refused, the saved form - and the fp16 launchers reject bad descriptors on the host."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(__file__))
import _model_cases as mc  # noqa: E402


def _eval_model(name, deepsup=True):
    return mc.host_model(name, deepsup=deepsup).eval()


def _convs_outside_deepsup(m):
    return [(n, mod) for n, mod in m.named_modules() if isinstance(mod, nn.Conv2d) and not n.startswith("conv_deepsup")]


@pytest.mark.parametrize("name,extra", [("deeplabv3", 3), ("simple", 1)])
def test_freeze_plans_on_the_cpu(name, extra):
    """One record per conv outside conv_deepsup, plus the pool (maxpool, ASPP average pool) and broadcast nodes."""
    from dcfp_amd import deploy
    m = _eval_model(name)
    eng = deploy.freeze(m)
    convs = _convs_outside_deepsup(m)
    assert len(eng.plan) == len(convs) + extra
    assert sorted(r["name"] for r in eng.conv_records()) == sorted(n for n, _ in convs)
    pools = [r["op"] for r in eng.plan if r["op"] != "conv"]
    assert pools == (["maxpool", "avgpool", "broadcast"] if name == "deeplabv3" else ["maxpool"])
    assert not any(r["name"].startswith("conv_deepsup") for r in eng.plan)
    assert all(t.device.type == "cpu" for t in eng.tensors)
    assert eng.align_corner is True and eng.num_classes == 19
    # every buffer pitch is a multiple of 8; the stem reads 3 channels padded to 8; the concat is written in slices
    assert all(p % 8 == 0 for p in eng.buffers) and eng.buffers[0] == 8
    if name == "deeplabv3":
        offs = [r["y_off"] for r in eng.plan if r["name"].startswith("aspp.aspp") or r["op"] == "broadcast"]
        assert offs == [0, 256, 512, 768, 1024]
        assert eng.plan[-4]["name"] == "aspp.conv1" and eng.plan[-4]["cin8"] == 1280


def _folded_fp16(m, rec):
    """fp16(w * scale) of a record's conv, restated from the module (fp64 fold, one rounding)."""
    mods = dict(m.named_modules())
    conv = mods[rec["name"]]
    w = conv.weight.detach().double()
    bn_name = {"backbone.conv1.6": "backbone.bn1"}.get(rec["name"])
    if bn_name is None:
        parent, leaf = rec["name"].rsplit(".", 1)
        if leaf.isdigit():
            bn_name = f"{parent}.{int(leaf) + 1}"
        elif leaf == "atrous_conv":
            bn_name = parent + ".bn"
        else:
            bn_name = f"{parent}.bn{leaf[-1]}"
    bn = mods.get(bn_name)
    if not isinstance(bn, nn.BatchNorm2d):
        return w.to(torch.float16), conv.bias.detach().double()
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return (w * scale.view(-1, 1, 1, 1)).to(torch.float16), bn.bias.detach().double() - bn.running_mean.double() * scale


def _check_packing(m, eng):
    from dcfp_amd import deploy
    for rec in eng.conv_records():
        want, shift = _folded_fp16(m, rec)
        packed = eng.tensors[rec["w"]]
        cout, cin, k = rec["cout"], rec["cin"], rec["k"]
        assert packed.dtype == torch.float16 and tuple(packed.shape) == ((cout + 7) // 8 * 8, k, k, rec["cin8"]), rec["name"]
        assert torch.equal(deploy.unpack_weight(packed, cout, rec["segments"]), want), rec["name"]
        # the padding: output rows beyond cout, and every input column outside the segments, are zero
        mask = torch.zeros(rec["cin8"], dtype=torch.bool)
        for off, cnt in rec["segments"]:
            mask[off:off + cnt] = True
        assert int(mask.sum()) == cin
        assert packed[cout:].abs().sum() == 0 and packed[:, :, :, ~mask].abs().sum() == 0, rec["name"]
        sh = eng.tensors[rec["shift"]]
        assert sh.dtype == torch.float32 and sh.numel() == packed.shape[0]
        assert torch.equal(sh[:cout], shift.float()) and sh[cout:].abs().sum() == 0, rec["name"]


def test_packed_weights_are_the_folded_fp16_weights():
    from dcfp_amd import deploy
    m = _eval_model("deeplabv3")
    _check_packing(m, deploy.freeze(m))


def test_slim_model_packs_ragged_widths(tmp_path):
    """A model slimmed by init_pruned_model: widths that are no multiple of 8 occur, on both sides of a conv and in
    the ASPP concat, and pack with zeros in the padding."""
    from dcfp_amd import deploy, pruners
    m = mc.host_model("deeplabv3")
    _, pruned, cfg = mc._prune_gp50(m, str(tmp_path / "score.pth"))
    slim = mc.host_model("deeplabv3")
    pruners.init_pruned_model(slim, cfg)
    slim.load_state_dict(pruned.state_dict())
    slim.eval()
    eng = deploy.freeze(slim)
    recs = eng.conv_records()
    assert any(r["cout"] % 8 for r in recs) and any(r["cin"] % 8 for r in recs)
    cat = [r for r in recs if r["name"] == "aspp.conv1"][0]
    assert len(cat["segments"]) == 5 and all(off % 8 == 0 for off, _ in cat["segments"])
    _check_packing(slim, eng)


@pytest.mark.parametrize("name", ["deeplabv3p", "psp"])
def test_other_heads_are_refused_by_name(name):
    from dcfp_amd import deploy
    with pytest.raises(NotImplementedError, match=name):
        deploy.freeze(_eval_model(name))


def test_unknown_modules_and_training_mode_are_refused():
    from dcfp_amd import deploy
    with pytest.raises(RuntimeError, match="training"):
        deploy.freeze(mc.host_model("simple"))
    with pytest.raises(NotImplementedError):
        deploy.freeze(nn.Sequential(nn.Conv2d(3, 8, 3)).eval())
    m = _eval_model("simple")
    m.backbone.layer1[0].conv2 = nn.Conv2d(64, 64, 5, padding=2, bias=False)
    with pytest.raises(NotImplementedError, match="layer1.0.conv2"):
        deploy.freeze(m)
    with pytest.raises(NotImplementedError):
        deploy.freeze(_eval_model("simple"), dtype=torch.bfloat16)


def test_state_dict_is_plain_and_round_trips(tmp_path):
    from dcfp_amd import deploy
    eng = deploy.freeze(_eval_model("simple", deepsup=False))
    sd = eng.state_dict()

    def plain(v):
        if isinstance(v, dict):
            return all(isinstance(k, str) and plain(x) for k, x in v.items())
        if isinstance(v, (list, tuple)):
            return all(plain(x) for x in v)
        return isinstance(v, (torch.Tensor, int, float, bool, str))
    assert plain(sd)
    path = str(tmp_path / "engine.pth")
    torch.save(sd, path)
    back = deploy.load_engine(path)          # (weights_only load: tensors and plain containers)
    assert back.plan == eng.plan and back.buffers == eng.buffers and back.meta == eng.meta
    assert all(torch.equal(a, b) for a, b in zip(back.tensors, eng.tensors))
    with pytest.raises(RuntimeError):        # no CPU path
        back.lowres_logits(torch.zeros(1, 3, 32, 32))


def test_fp16_launchers_reject_bad_descriptors_on_the_host():
    from dcfp_amd import _lib
    L = _lib.lib()

    def desc(**kw):
        v = dict(N=1, H=8, W=8, Cin8=8, x_pitch=8, Cout=8, K=3, stride=1, pad=1, dil=1, Hout=8, Wout=8, y_pitch=8,
                 y_off=0, res_pitch=0, res_off=0, relu=1)
        v.update(kw)
        return ctypes.byref(_lib.ConvF16Desc(*[v[n] for n, _ in _lib.ConvF16Desc._fields_]))
    call = L.dcfp_conv2d_fwd_f16_nhwc
    assert call(desc(K=5, pad=2), None, None, None, None, None, None) == _lib.E_UNSUPPORTED
    assert call(desc(stride=3, Hout=3, Wout=3), None, None, None, None, None, None) == _lib.E_UNSUPPORTED
    assert call(desc(Hout=7), None, None, None, None, None, None) == _lib.E_BADDESC
    assert call(desc(Cin8=12), None, None, None, None, None, None) == _lib.E_BADDESC
    assert call(desc(y_off=4), None, None, None, None, None, None) == _lib.E_BADDESC
    assert call(desc(y_off=8), None, None, None, None, None, None) == _lib.E_BADDESC      # slice past the pitch
    assert call(desc(), None, None, None, None, None, None) == _lib.E_BADDESC              # null pointers
    assert L.dcfp_conv2d_fwd_f16_nhwc_to_f32_nchw(desc(K=2), None, None, None, None, None) == _lib.E_UNSUPPORTED
    assert L.dcfp_conv2d_fwd_f16_nhwc_to_f32_nchw(desc(Cout=19), None, None, None, None, None) == _lib.E_BADDESC
    assert L.dcfp_maxpool3x3s2_nhwc_f16(None, None, 1, 8, 8, 8, 8, 4, 4, 8, None) == _lib.E_BADDESC
    assert L.dcfp_avgpool_nhwc_f16(None, None, 1, 64, 8, 8, 8, None, 0, None) == _lib.E_BADDESC
    assert L.dcfp_broadcast_nhwc_f16(None, 8, None, 1, 64, 8, 8, 0, None) == _lib.E_BADDESC
    assert L.dcfp_nchw_f32_to_nhwc_f16(None, None, 1, 3, 8, 8, 8, None) == _lib.E_BADDESC
    assert L.dcfp_avgpool_nhwc_f16_workspace_bytes(2, 264, 4900) == 2 * 20 * 264 * 4
