"""CPU: deploy.build_engine plans and packs the DeepLabv3+ and PSPNet heads without a device - record names, slice
offsets, segments, packed weights against fp16(w * scale) with zero padding, ragged widths, the saved form, what is
refused - the two launchers of csrc/heads_f16.hip reject bad arguments on the host, and the CPU yardstick of the GPU
tests (tests/_deploy_heads_ref.py) reproduces the reference's own slim-model logits."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _deploy_heads_ref as href  # noqa: E402
import _model_cases as mc  # noqa: E402
from oracle import fill, model as omodel  # noqa: E402

HEADS = ("psp", "deeplabv3p")
_EXTRA = {"psp": ["maxpool", "pyramid", "resize", "resize", "resize", "resize"],
          "deeplabv3p": ["maxpool", "avgpool", "broadcast", "resize"]}
_cache = {}


def _eval_model(name, deepsup=True):
    return mc.host_model(name, deepsup=deepsup).eval()


def _slim(name, tmp):
    """The R50 of head `name` slimmed as mc.slim_model_logits_check does (global_percent 0.5, synthetic scores)."""
    if name not in _cache:
        from dcfp_amd import pruners
        tag = {"psp": "pspr50", "deeplabv3p": "v3pr50"}[name]
        g = np.load(os.path.join(mc.G, f"prune_{tag}_gp50.npz"))
        cpu = torch.device("cpu")
        m = mc.build_model(name, "resnet50", True, cpu, criterion=False)
        _, pruned, cfg = mc._prune_gp50(m, os.path.join(str(tmp), "score.pth"))
        assert list(cfg.keys()) == g["names"].tolist()
        slim = mc.build_model(name, "resnet50", True, cpu, criterion=False)
        pruners.init_pruned_model(slim, cfg)
        slim.load_state_dict(pruned.state_dict())
        _cache[name] = (slim.eval(), g["slim_logits"])
    return _cache[name]


def _bn_of(mods, conv_name):
    """The BatchNorm that follows conv `conv_name` in the module tree (None: the classifier)."""
    fixed = {"backbone.conv1.6": "backbone.bn1", "decoder.conv1": "decoder.bn1", "aspp.conv1": "aspp.bn1"}
    if conv_name in fixed:
        return mods[fixed[conv_name]]
    parent, leaf = conv_name.rsplit(".", 1) if "." in conv_name else ("", conv_name)
    if leaf.isdigit():
        name = f"{parent}.{int(leaf) + 1}"
    elif leaf == "atrous_conv":
        name = parent + ".bn"
    else:
        name = f"{parent}.bn{leaf[-1]}"
    bn = mods.get(name)
    return bn if isinstance(bn, nn.BatchNorm2d) else None


def _check_packing(m, eng):
    from dcfp_amd import deploy
    mods = dict(m.named_modules())
    for rec in eng.conv_records():
        conv, bn = mods[rec["name"]], _bn_of(mods, rec["name"])
        w = conv.weight.detach().double()
        if bn is None:
            want, shift = w.to(torch.float16), conv.bias.detach().double()
        else:
            scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
            want = (w * scale.view(-1, 1, 1, 1)).to(torch.float16)
            shift = bn.bias.detach().double() - bn.running_mean.double() * scale
        packed = eng.tensors[rec["w"]]
        cout, cin, k = rec["cout"], rec["cin"], rec["k"]
        assert packed.dtype == torch.float16 and tuple(packed.shape) == ((cout + 7) // 8 * 8, k, k, rec["cin8"]), rec["name"]
        assert torch.equal(deploy.unpack_weight(packed, cout, rec["segments"]), want), rec["name"]
        mask = torch.zeros(rec["cin8"], dtype=torch.bool)
        for off, cnt in rec["segments"]:
            mask[off:off + cnt] = True
        assert int(mask.sum()) == cin
        assert packed[cout:].abs().sum() == 0 and packed[:, :, :, ~mask].abs().sum() == 0, rec["name"]
        sh = eng.tensors[rec["shift"]]
        assert sh.dtype == torch.float32 and sh.numel() == packed.shape[0]
        assert torch.equal(sh[:cout], shift.float()) and sh[cout:].abs().sum() == 0, rec["name"]


def _check_plan(name, m, eng):
    convs = [n for n, mod in m.named_modules() if isinstance(mod, nn.Conv2d) and not n.startswith("conv_deepsup")]
    assert sorted(r["name"] for r in eng.conv_records()) == sorted(convs)
    assert sorted(r["op"] for r in eng.plan if r["op"] != "conv") == sorted(_EXTRA[name])
    assert len(eng.plan) == len(convs) + len(_EXTRA[name])
    assert not any(r["name"].startswith("conv_deepsup") for r in eng.plan)
    assert all(t.device.type == "cpu" for t in eng.tensors)
    assert all(p % 8 == 0 for p in eng.buffers) and eng.buffers[0] == 8
    for r in eng.plan:
        assert r["y_off"] % 8 == 0 and r.get("x_off", 0) % 8 == 0, r["name"]
        for off, _ in r.get("segments", []):
            assert off % 8 == 0, r["name"]
    by_name = {r["name"]: r for r in eng.plan}
    if name == "psp":
        cat = by_name["ppm.bottleneck.0"]
        assert len(cat["segments"]) == 5
        last = [r for r in eng.plan if r["name"].startswith("backbone.layer4") and r["name"].endswith("conv3")][-1]
        pyr = by_name["ppm.stages.pool"]
        # no cat, no copy: conv3 writes the feats slice of the concat, the pyramid pools from that slice, and each
        # prior is resized into its own slice of the same buffer
        assert last["dst"] == cat["src"] == pyr["src"] and last["y_off"] == pyr["x_off"] == cat["segments"][4][0]
        assert last["res"] >= 0 and eng.buffers[last["res"]] != eng.buffers[last["dst"]]
        assert pyr["sizes"] == [1, 2, 3, 6] and len(pyr["dsts"]) == 4
        ups = [r for r in eng.plan if r["op"] == "resize"]
        assert [u["dst"] for u in ups] == [cat["src"]] * 4
        assert [u["y_off"] for u in ups] == [off for off, _ in cat["segments"][:4]]
        assert eng.plan[-1]["name"] == "last_conv" and eng.plan[-1]["f32"]
    else:
        cat = by_name["decoder.last_conv.0"]
        assert len(cat["segments"]) == 2
        up, c1 = by_name["decoder.up"], by_name["decoder.conv1"]
        assert up["dst"] == c1["dst"] == cat["src"]
        assert [up["y_off"], c1["y_off"]] == [off for off, _ in cat["segments"]]
        l1 = [r for r in eng.plan if r["name"].startswith("backbone.layer1") and r["name"].endswith("conv3")][-1]
        assert c1["src"] == l1["dst"] and up["src"] == by_name["aspp.conv1"]["dst"]
        assert eng.plan[-1]["name"] == "decoder.last_conv.6" and eng.plan[-1]["f32"]
    return by_name


@pytest.mark.parametrize("name", HEADS)
def test_build_engine_plans_on_the_cpu(name):
    from dcfp_amd import deploy
    m = _eval_model(name)
    eng = deploy.build_engine(m)
    by_name = _check_plan(name, m, eng)
    assert eng.align_corner is True and eng.num_classes == 19 and eng.meta["model"] == name
    if name == "psp":
        assert by_name["ppm.bottleneck.0"]["segments"] == [[0, 512], [512, 512], [1024, 512], [1536, 512], [2048, 2048]]
        hw = eng.buffer_shapes(65, 65)
        assert [hw[b] for b in by_name["ppm.stages.pool"]["dsts"]] == [(1, 1), (2, 2), (3, 3), (6, 6)]
        assert hw[by_name["ppm.bottleneck.0"]["src"]] == (9, 9) and hw[-1] == (9, 9)
    else:
        assert by_name["decoder.last_conv.0"]["segments"] == [[0, 512], [512, 48]]
        hw = eng.buffer_shapes(65, 65)
        assert hw[by_name["decoder.last_conv.0"]["src"]] == (17, 17) and hw[by_name["decoder.up"]["src"]] == (9, 9)
        assert hw[-1] == (17, 17)
    _check_packing(m, eng)


@pytest.mark.parametrize("name", HEADS)
def test_slim_models_plan_and_pack_ragged_widths(name, tmp_path):
    from dcfp_amd import deploy
    slim, _ = _slim(name, tmp_path)
    eng = deploy.build_engine(slim)
    recs = eng.conv_records()
    assert any(r["cout"] % 8 for r in recs) and any(r["cin"] % 8 for r in recs)
    _check_plan(name, slim, eng)
    _check_packing(slim, eng)


@pytest.mark.parametrize("name", HEADS)
def test_state_dict_is_plain_and_round_trips(name, tmp_path):
    from dcfp_amd import deploy
    eng = deploy.build_engine(_eval_model(name, deepsup=False))
    sd = eng.state_dict()

    def plain(v):
        if isinstance(v, dict):
            return all(isinstance(k, str) and plain(x) for k, x in v.items())
        if isinstance(v, (list, tuple)):
            return all(plain(x) for x in v)
        return isinstance(v, (torch.Tensor, int, float, bool, str))
    assert plain(sd) and sd["format"] == 1
    path = str(tmp_path / "engine.pth")
    torch.save(sd, path)
    assert isinstance(torch.load(path, map_location="cpu", weights_only=True), dict)
    back = deploy.load_engine(path)
    assert back.plan == eng.plan and back.buffers == eng.buffers and back.meta == eng.meta
    assert all(torch.equal(a, b) for a, b in zip(back.tensors, eng.tensors))
    assert back._slot_of == eng._slot_of
    with pytest.raises(RuntimeError):        # no CPU path
        back.lowres_logits(torch.zeros(1, 3, 32, 32))


def test_kept_buffers_do_not_share_a_slot_with_what_is_written_meanwhile():
    """Liveness: the layer1 output lives until decoder.conv1 reads it; the pyramid's pooled maps until their convs."""
    from dcfp_amd import deploy
    for name in HEADS:
        eng = deploy.build_engine(_eval_model(name, deepsup=False))
        first, last = {0: -1}, {}
        for i, r in enumerate(eng.plan):
            for b in [r["src"], r["dst"], r.get("res", -1)] + list(r.get("dsts", ())):
                if b >= 0:
                    first.setdefault(b, i)
                    last[b] = i
        for a in first:
            for b in first:
                if a < b and eng._slot_of[a] == eng._slot_of[b]:
                    assert last[a] < first[b] or last[b] < first[a], (name, a, b)


@pytest.mark.parametrize("name", ["deeplabv3", "simple"])
def test_build_engine_equals_freeze_on_the_first_two_heads(name):
    from dcfp_amd import deploy
    m = _eval_model(name)
    a, b = deploy.freeze(m), deploy.build_engine(m)
    assert type(a) is type(b) is deploy.Engine
    assert a.plan == b.plan and a.buffers == b.buffers and a.meta == b.meta
    assert len(a.tensors) == len(b.tensors) and all(torch.equal(s, t) for s, t in zip(a.tensors, b.tensors))


def test_what_build_engine_refuses():
    from dcfp_amd import deploy
    with pytest.raises(RuntimeError, match="training"):
        deploy.build_engine(mc.host_model("psp"))
    with pytest.raises(RuntimeError, match="training"):
        deploy.build_engine(mc.host_model("deeplabv3p"))
    with pytest.raises(NotImplementedError):
        deploy.build_engine(_eval_model("psp"), dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        deploy.build_engine(nn.Sequential(nn.Conv2d(3, 8, 3)).eval())
    m = _eval_model("psp")
    m.ppm.stages[3][0] = nn.AdaptiveAvgPool2d((9, 9))
    with pytest.raises(NotImplementedError, match=r"ppm\.stages\.3"):
        deploy.build_engine(m)
    m = _eval_model("psp")
    m.ppm.stages[1][0] = nn.AdaptiveAvgPool2d((2, 3))
    with pytest.raises(NotImplementedError, match=r"ppm\.stages\.1"):
        deploy.build_engine(m)
    m = _eval_model("psp")
    m.ppm.stages.append(m.ppm._make_stage(2048, 512, 4))
    with pytest.raises(NotImplementedError, match=r"ppm\.stages"):
        deploy.build_engine(m.eval())
    m = _eval_model("psp")
    m.ppm.stages[2][1] = nn.Conv2d(2048, 512, 1, bias=True)
    with pytest.raises(NotImplementedError, match=r"ppm\.stages\.2\.1"):
        deploy.build_engine(m.eval())
    m = _eval_model("deeplabv3p")
    m.decoder.conv1 = nn.Conv2d(256, 48, 3, padding=1, bias=False)
    with pytest.raises(NotImplementedError, match=r"decoder\.conv1"):
        deploy.build_engine(m.eval())
    m = _eval_model("deeplabv3p")
    m.decoder.extra = nn.Identity()
    with pytest.raises(NotImplementedError, match=r"decoder\.extra"):
        deploy.build_engine(m)


def test_head_launchers_reject_bad_arguments_on_the_host():
    from dcfp_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096 + 16)            # host memory: every call below returns before any HIP call
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    P = ctypes.c_void_p

    def resize(x=p, N=1, h=3, w=3, C8=8, xp=8, y=p, H=9, W=9, yp=16, yo=8, align=1):
        return L.dcfp_resize_bilinear_nhwc_f16(P(x) if x else None, N, h, w, C8, xp, P(y) if y else None, H, W, yp, yo,
                                               align, None)
    assert resize(x=None) == _lib.E_BADDESC and resize(y=None) == _lib.E_BADDESC
    assert resize(x=p + 2) == _lib.E_BADDESC and resize(y=p + 8) == _lib.E_BADDESC
    assert resize(N=0) == _lib.E_BADDESC and resize(h=0) == _lib.E_BADDESC and resize(W=-1) == _lib.E_BADDESC
    assert resize(C8=12) == _lib.E_BADDESC and resize(xp=12) == _lib.E_BADDESC and resize(yp=20) == _lib.E_BADDESC
    assert resize(yo=4) == _lib.E_BADDESC
    assert resize(yo=16) == _lib.E_BADDESC                  # the slice does not fit its pitch
    assert resize(C8=16, xp=8) == _lib.E_BADDESC
    assert resize(H=40000) == _lib.E_UNSUPPORTED

    ws_bytes = L.dcfp_pyramid_pool_nhwc_f16_workspace_bytes

    def pyramid(x=p, N=1, H=9, W=9, C8=8, xp=16, xo=8, sizes=(1, 2, 3, 6), y=None, yp=None, ws=p, nbytes=None):
        n = len(sizes)
        s = (ctypes.c_int * n)(*sizes)
        outs = (P * n)(*(y if y is not None else [p] * n))
        pitches = (ctypes.c_int * n)(*(yp if yp is not None else [8] * n))
        if nbytes is None:
            nbytes = ws_bytes(N, H, W, C8, n, s)
        return L.dcfp_pyramid_pool_nhwc_f16(P(x) if x else None, N, H, W, C8, xp, xo, n, s, outs, pitches,
                                            P(ws) if ws else None, nbytes, None)
    assert pyramid(x=None) == _lib.E_BADDESC and pyramid(x=p + 4) == _lib.E_BADDESC
    assert pyramid(N=0) == _lib.E_BADDESC and pyramid(H=0) == _lib.E_BADDESC
    assert pyramid(C8=12) == _lib.E_BADDESC and pyramid(xp=20) == _lib.E_BADDESC and pyramid(xo=4) == _lib.E_BADDESC
    assert pyramid(xo=16) == _lib.E_BADDESC                 # the slice does not fit its pitch
    assert pyramid(sizes=()) == _lib.E_BADDESC and pyramid(sizes=(1, 0)) == _lib.E_BADDESC
    assert pyramid(y=[p, None, p, p]) == _lib.E_BADDESC and pyramid(yp=[8, 8, 12, 8]) == _lib.E_BADDESC
    assert pyramid(sizes=(1, 9)) == _lib.E_UNSUPPORTED
    assert pyramid(sizes=(1, 2, 3, 4, 6)) == _lib.E_UNSUPPORTED
    assert pyramid(ws=None) == _lib.E_WORKSPACE
    need = ws_bytes(1, 9, 9, 8, 4, (ctypes.c_int * 4)(1, 2, 3, 6))
    assert need > 0 and need % (8 * 4) == 0
    assert pyramid(nbytes=need - 1) == _lib.E_WORKSPACE
    assert ws_bytes(1, 9, 9, 8, 2, (ctypes.c_int * 2)(1, 9)) == 0
    # 9 rows under sizes (1, 2, 3, 6): the windows' boundaries are 0 .. 9, every one of them -> 9 atoms per axis
    assert need == 9 * 9 * 8 * 4


@pytest.mark.parametrize("name", HEADS)
def test_the_cpu_yardstick_reproduces_the_reference_slim_logits(name, tmp_path):
    """tests/_deploy_heads_ref.py against the reference's own output: fp64 logits of the slimmed R50 at 2x3x33x33,
    upsampled with align_corners, within the 1e-3 the project already uses for these fixtures."""
    slim, gold = _slim(name, tmp_path)
    cfg = omodel.Cfg(name, "resnet50", align_corner=True, deepsup=False)
    low = href.eval_logits64(slim.state_dict(), fill.closed_form_input(2, 33, 33), cfg)
    full = F.interpolate(low, size=(33, 33), mode="bilinear", align_corners=True)
    err = float(np.abs(full.numpy() - gold).max())
    print(f"{name}: helper fp64 logits vs the reference's slim logits: max-abs {err:.2e}")
    assert tuple(full.shape) == tuple(gold.shape) and err <= 1e-3, err
