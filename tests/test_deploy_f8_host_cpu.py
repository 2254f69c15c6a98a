"""CPU: the host side of the fp8 engine (dcfp_amd/deploy.py) - planning, scales, packing, persistence,
refusals - and the stability of its yardstick (tests/_deploy_f8_ref.py).  The calibration maxima come from the fp64
forward here (f8ref.record_amax), which has the record names deploy.calibrate gives on the device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _deploy_f8_ref as f8ref  # noqa: E402
import _model_cases as mc  # noqa: E402
from oracle import fill, model as omodel  # noqa: E402

F8 = torch.float8_e4m3fn
_SIZES = {"v3_r50_2x65x65": (2, 65, 65), "simple_r50_4x64x64": (4, 64, 64)}
_cache = {}


def _full(tag):
    if tag not in _cache:
        case = mc.CASES[tag]
        m = mc.build_model(case.model, case.backbone, True, torch.device("cpu"), criterion=False).eval()
        x = fill.closed_form_input(*_SIZES[tag])
        cfg = omodel.Cfg(case.model, case.backbone, align_corner=True, deepsup=False)
        _cache[tag] = (m, x, cfg, f8ref.record_amax(m.state_dict(), x, cfg))
    return _cache[tag]


def _slim(tmp):
    from dcfp_amd import pruners
    if "slim" not in _cache:
        cpu = torch.device("cpu")
        m = mc.build_model("deeplabv3", "resnet50", True, cpu, criterion=False)
        _, pruned, cfg = mc._prune_gp50(m, os.path.join(tmp, "score.pth"))
        slim = mc.build_model("deeplabv3", "resnet50", True, cpu, criterion=False)
        pruners.init_pruned_model(slim, cfg)
        slim.load_state_dict(pruned.state_dict())
        slim = slim.eval()
        x = fill.closed_form_input(2, 65, 65)
        ocfg = omodel.Cfg("deeplabv3", "resnet50", align_corner=True, deepsup=False)
        _cache["slim"] = (slim, x, ocfg, f8ref.record_amax(slim.state_dict(), x, ocfg))
    return _cache["slim"]


def _bn_of(name):
    """The BatchNorm module name that follows the conv `name` (None: the classifier)."""
    head, _, leaf = name.rpartition(".")
    if name == "backbone.conv1.6":
        return "backbone.bn1"
    if leaf in ("conv1", "conv2", "conv3"):
        return head + ".bn" + leaf[-1]
    if leaf == "atrous_conv":
        return head + ".bn"
    if name == "last_conv.6":
        return None
    return head + "." + str(int(leaf) + 1)


def _folded(m, name):
    mods = dict(m.named_modules())
    w = mods[name].weight.detach().double()
    bn = _bn_of(name)
    if bn is None:
        return w, mods[name].bias.detach().double()
    b = mods[bn]
    scale = b.weight.detach().double() / torch.sqrt(b.running_var.detach().double() + b.eps)
    return w * scale.view(-1, 1, 1, 1), b.bias.detach().double() - b.running_mean.detach().double() * scale


def _check_packing(m, eng):
    from dcfp_amd import deploy
    assert eng.format == 2 and eng.meta["dtype"] == "float8_e4m3fn"
    n8 = 0
    for r in eng.plan:
        if r["op"] != "conv":
            continue
        if r["fmt"] == "f16":
            assert r["name"] in ("backbone.conv1.0", "aspp.global_avg_pool.1"), r["name"]
            continue
        n8 += 1
        wf, shift = _folded(m, r["name"])
        cout, cin, k, _ = wf.shape
        packed = eng.tensors[r["w"]]
        assert packed.dtype == F8 and tuple(packed.shape) == ((cout + 7) // 8 * 8, k, k, eng.buffers[r["src"]])
        assert eng.buffers[r["src"]] % 16 == 0 and eng.buffer_fmt[r["src"]] == "f8"
        amax = wf.abs().amax(dim=(1, 2, 3))
        s_w = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        back = deploy.unpack_weight(packed, cout, r["segments"]).double() * s_w.view(-1, 1, 1, 1)
        tol = 2.0 ** -4 * wf.abs() + 2.0 ** -10 * s_w.view(-1, 1, 1, 1)
        assert bool(((back - wf).abs() <= tol).all()), r["name"]
        # padded rows and columns: zero bytes
        raw = packed.view(torch.uint8)
        assert int(raw[cout:].count_nonzero()) == 0
        used = torch.zeros(packed.shape[3], dtype=torch.bool)
        for off, cnt in r["segments"]:
            assert off % 16 == 0, (r["name"], r["segments"])
            used[off:off + cnt] = True
        assert int(raw[..., ~used].count_nonzero()) == 0
        # mul = s_w * s_x / s_y and add = shift / s_y, formed in fp64 and rounded once
        s_x = eng.scales[r["src"]]
        s_y = 1.0 if r["f32"] else eng.scales[r["dst"]]
        mul, add = eng.tensors[r["mul"]], eng.tensors[r["add"]]
        assert mul.dtype == torch.float32 and add.dtype == torch.float32
        assert torch.equal(mul[:cout], (s_w * s_x / s_y).float()) and torch.equal(add[:cout], (shift / s_y).float())
        assert int(mul[cout:].count_nonzero()) == 0 and int(add[cout:].count_nonzero()) == 0
        if not r["f32"]:
            assert r["y_off"] % 16 == 0 and eng.buffers[r["dst"]] % 16 == 0
    return n8


def test_fp8_plan_packs_weights_within_the_e4m3_rounding_bound():
    from dcfp_amd import deploy
    for tag in _SIZES:
        m, x, cfg, amax = _full(tag)
        eng = deploy.build_engine(m, precision="fp8", amax=amax)
        assert _check_packing(m, eng) >= 50
        ops = [r["op"] for r in eng.plan]
        assert ops[0] == "conv" and eng.plan[0]["fmt"] == "f16" and ops[1] == "cast"
        assert eng.plan[-1]["f32"] and eng.plan[-1]["fmt"] == "f8"
        # one scale per buffer: s_b = max(amax over its writers) / 448; the pooled map keeps its input's scale
        for r in eng.plan:
            if r["op"] == "maxpool":
                assert eng.scales[r["dst"]] == eng.scales[r["src"]]
        if tag.startswith("v3"):
            cat = [r for r in eng.plan if r["name"] == "aspp.conv1"][0]["src"]
            writers = [r["name"] for r in eng.plan if r["dst"] == cat]
            assert len(writers) == 5
            assert eng.scales[cat] == max(amax[n] for n in writers) / 448.0
            assert all(off % 16 == 0 for off, _ in [r for r in eng.plan if r["name"] == "aspp.conv1"][0]["segments"])


def test_slim_model_with_ragged_widths_packs(tmp_path):
    from dcfp_amd import deploy
    m, x, cfg, amax = _slim(str(tmp_path))
    widths = [c.out_channels for c in m.modules() if isinstance(c, torch.nn.Conv2d)]
    assert any(c % 16 for c in widths), widths
    eng = deploy.build_engine(m, precision="fp8", amax=amax)
    assert _check_packing(m, eng) >= 50
    assert all(p % 16 == 0 for p, f in zip(eng.buffers, eng.buffer_fmt) if f == "f8")


def test_fp8_engine_state_round_trips_bit_identically(tmp_path):
    from dcfp_amd import deploy
    m, x, cfg, amax = _full("v3_r50_2x65x65")
    eng = deploy.build_engine(m, precision="fp8", amax=amax)
    path = str(tmp_path / "engine_fp8.pth")
    torch.save(eng.state_dict(), path)
    again = deploy.load_engine(path)
    a, b = eng.state_dict(), again.state_dict()
    assert a["format"] == b["format"] == 2 and a["meta"] == b["meta"] and a["plan"] == b["plan"]
    assert a["buffers"] == b["buffers"] and a["buffer_fmt"] == b["buffer_fmt"] and a["scales"] == b["scales"]
    assert len(a["tensors"]) == len(b["tensors"])
    for s, t in zip(a["tensors"], b["tensors"]):
        assert s.dtype == t.dtype and s.shape == t.shape
        assert torch.equal(s.contiguous().view(torch.uint8), t.contiguous().view(torch.uint8))
    # an fp16 engine keeps format 1 and its keys
    st = deploy.build_engine(m).state_dict()
    assert st["format"] == 1 and sorted(st) == ["buffers", "format", "meta", "plan", "tensors"]
    assert all("fmt" not in r for r in st["plan"])


def test_fp8_refusals():
    from dcfp_amd import deploy
    m, x, cfg, amax = _full("v3_r50_2x65x65")
    for head in ("deeplabv3p", "psp"):
        other = mc.build_model(head, "resnet50", True, torch.device("cpu"), criterion=False).eval()
        with pytest.raises(NotImplementedError, match=head):
            deploy.build_engine(other, precision="fp8", amax=amax)
    for name in ("backbone.layer2.1.conv2", "aspp.global_avg_pool.up", "backbone.conv1.0"):
        short = {k: v for k, v in amax.items() if k != name}
        with pytest.raises(KeyError, match=name.replace(".", r"\.")):
            deploy.build_engine(m, precision="fp8", amax=short)
    with pytest.raises(ValueError):
        deploy.build_engine(m, precision="fp8")
    with pytest.raises(NotImplementedError):
        deploy.freeze(m, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        deploy.build_engine(m, dtype=torch.bfloat16, precision="fp8", amax=amax)


def test_to_f8_clamps_and_keeps_subnormals():
    from dcfp_amd import deploy
    t = torch.tensor([465.0, -500.0, 448.0, 2.0 ** -9, 2.0 ** -10, 0.3], dtype=torch.float64)
    assert deploy.to_f8(t).float().tolist() == [448.0, -448.0, 448.0, 2.0 ** -9, 0.0, 0.3125]


@pytest.mark.parametrize("tag", list(_SIZES))
def test_yardstick_is_stable_between_summation_orders(tag, capsys):
    """The fp64-sum and the fp32-sum emulation are two roundings of one chaotic computation; their relative L2
    distances to fp64 must agree within a factor 1.5, or the yardstick alone would leave the GPU test's margin."""
    m, x, cfg, amax = _full(tag)
    ref, d = f8ref.distances(m.state_dict(), x, cfg, amax)
    (e64, r64, l64), (e32, r32, l32) = d
    with capsys.disabled():
        print(f"\nfp8 yardstick {tag}: |logits| <= {float(ref.abs().max()):.0f}; fp64 sums rel-L2 {r64:.3e} max-abs "
              f"{e64:.1f} labels {100 * l64:.1f} %; fp32 sums rel-L2 {r32:.3e} max-abs {e32:.1f} labels {100 * l32:.1f} %")
    assert np.isfinite([r64, r32]).all() and min(r64, r32) > 0
    assert max(r64, r32) / min(r64, r32) <= 1.5, (r64, r32)
