"""GPU: the calibrated fp8 engine (dcfp_amd/deploy.py build_engine(precision="fp8")).

On the closed-form weights fp8 rounding is chaotic: two summation orders of one emulation differ from each other by as
much as either differs from fp64, and only relative L2 is stable (tests/test_deploy_f8_host_cpu.py).  Strictness
therefore comes from the per-kernel tests (tests/test_conv_f8_gpu.py) and from the per-record REPLAY here: every record
of a real engine run is recomputed in fp64 from the bytes that record actually read (taken from Engine.trace) and the
engine's packed tensors, and held to the per-kernel bound - rounding flips cannot accumulate, and no record is sampled.

Whole model: low-resolution logits against fp64, relative L2 <= 1.5 r and max-abs <= 3 e with (e, r) the larger of the
two tests/_deploy_f8_ref.py emulations' distances (the margins of tests/test_deploy_gpu.py, for the reason it gives).
The label disagreement is printed, not asserted: at 162 - 256 low-resolution pixels it is noise.

The pooled vector of the replay is held to the average pool's per-kernel bound 2 * ((HW + 1) * 2^-24 * mean|x| * scale +
2^-11 * |ref|) where |ref| >= 2^-14; below fp16's smallest normal number no fp16 value is closer to an arbitrary real
than half the subnormal spacing, so 2 * 2^-25 is added there (the slim model has 3 such channels of 4096: ref 4.98e-6,
stored 5.007e-6 = the nearest fp16 number, 2.8e-8 away, against 4.9e-9 from the relative terms alone).

Measured on an MI355X, relative L2 to fp64 / label disagreement with fp64 (engine; fp64-sum, fp32-sum emulation):
v3_r50_2x65x65 1.52e-1 / 21.0 % (1.47e-1 / 19.8 %, 1.43e-1 / 22.2 %), simple_r50_4x64x64 1.45e-1 / 7.0 % (1.39e-1 /
9.0 %, 1.36e-1 / 9.0 %), slim 1.30e-1 / 9.3 % (1.16e-1 / 8.0 %, 1.17e-1 / 9.9 %); worst replayed conv 0.63 of its bound."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _deploy_f8_ref as f8ref  # noqa: E402
import _model_cases as mc  # noqa: E402
from oracle import fill, model as omodel  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = torch.float8_e4m3fn
_SIZES = {"v3_r50_2x65x65": (2, 65, 65), "simple_r50_4x64x64": (4, 64, 64)}
_cache = {}


def _full(tag):
    """(eval-mode model on the CPU, input, oracle Cfg) of a whole-model case: closed-form weights and input."""
    case = mc.CASES[tag]
    m = mc.build_model(case.model, case.backbone, True, torch.device("cpu"), criterion=False).eval()
    return m, fill.closed_form_input(*_SIZES[tag]), omodel.Cfg(case.model, case.backbone, align_corner=True, deepsup=False)


def _slim(tmp):
    """The v3-R50 slimmed as slim_model_logits_check does: global_percent 0.5 on the prune_v3r50_gp50 scores."""
    from dcfp_amd import pruners
    g = np.load(os.path.join(mc.G, "prune_v3r50_gp50.npz"))
    cpu = torch.device("cpu")
    m = mc.build_model("deeplabv3", "resnet50", True, cpu, criterion=False)
    _, pruned, cfg = mc._prune_gp50(m, os.path.join(tmp, "score.pth"))
    assert list(cfg.keys()) == g["names"].tolist()
    slim = mc.build_model("deeplabv3", "resnet50", True, cpu, criterion=False)
    pruners.init_pruned_model(slim, cfg)
    slim.load_state_dict(pruned.state_dict())
    return slim.eval(), fill.closed_form_input(2, 65, 65), omodel.Cfg("deeplabv3", "resnet50", align_corner=True, deepsup=False)


def _setup(tag, tmp_path_factory):
    """Per case, once: model, input, oracle Cfg, the fp16 engine, its calibration, the fp8 engine and its trace."""
    if tag not in _cache:
        from dcfp_amd import deploy
        m, x, cfg = _slim(str(tmp_path_factory.mktemp("slim"))) if tag == "slim" else _full(tag)
        eng16 = deploy.build_engine(m).to("cuda:0")
        xd = x.to("cuda:0")
        amax = deploy.calibrate(eng16, [xd])
        eng8 = deploy.build_engine(m, precision="fp8", amax=amax).to("cuda:0")
        trace = {k: v.cpu() for k, v in eng8.trace(xd).items()}
        _cache[tag] = (m, x, cfg, eng16, amax, eng8, trace)
    return _cache[tag]


TAGS = list(_SIZES) + ["slim"]


@pytest.mark.parametrize("tag", ["v3_r50_2x65x65"])
def test_calibration_is_the_traced_absolute_maximum(tag, tmp_path_factory, cuda):
    from dcfp_amd import deploy
    m, x, cfg, eng16, amax, eng8, _ = _setup(tag, tmp_path_factory)
    xd = x.to(cuda)
    t = eng16.trace(xd)
    assert set(r["name"] for r in eng16.plan) <= set(t) and set(amax) == set(t)
    for name, v in t.items():
        assert amax[name] == float(v.float().abs().amax()), name
    assert torch.equal(t[eng16.plan[-1]["name"]], eng16.lowres_logits(xd)[0])
    # maxima across batches
    two = deploy.calibrate(eng16, [xd, 2 * xd[:1]])
    one = deploy.calibrate(eng16, [2 * xd[:1]])
    assert all(two[k] == max(amax[k], one[k]) for k in amax)


def _dec(t):
    """Stored bytes -> float64 values."""
    return t.float().double()


def _nchw(t, c):
    return _dec(t[..., :c]).permute(0, 3, 1, 2)


def _replay(eng, trace, N, H, W):
    """Every record's output recomputed in fp64 from the bytes it read; returns the number of records checked."""
    hw = eng.buffer_shapes(H, W)
    bufs = {0: trace["input"]}
    worst_all, checked = 0.0, {}
    for r in eng.plan:
        name, op = r["name"], r["op"]
        src = bufs[r["src"]]
        got_raw = trace[name]
        f8 = r.get("fmt") == "f8"
        if op == "conv":
            cout, cin, k = r["cout"], r["cin"], r["k"]
            w = _dec(eng.tensors[r["w"]].cpu()[:cout]).permute(0, 3, 1, 2)          # [cout, pitch, k, k]
            xin = _nchw(src, w.shape[1])
            acc = F.conv2d(xin, w, None, r["stride"], r["pad"], r["dil"])
            S = F.conv2d(xin.abs(), w.abs(), None, r["stride"], r["pad"], r["dil"])
            bc = lambda v: v.cpu().double()[:cout].view(1, -1, 1, 1)  # noqa: E731
            if f8:
                mul, add = bc(eng.tensors[r["mul"]]), bc(eng.tensors[r["add"]])
            else:
                mul, add = torch.ones(1, cout, 1, 1, dtype=torch.float64), bc(eng.tensors[r["shift"]])
            ref, S = acc * mul + add, S * mul.abs() + add.abs()
            if r["res"] >= 0:
                rm = float(np.float32(r["res_mul"])) if f8 else 1.0
                res = rm * _nchw(bufs[r["res"]], cout)
                ref, S = ref + res, S + res.abs()
            K = cin * k * k
            if r["f32"]:
                got = got_raw.double()
                bound = 2 * ((K + 2) * 2.0 ** -24 * S + 2.0 ** -24)
                worst = float(((got - ref).abs() / bound).max())
            else:
                if r["relu"]:
                    ref = F.relu(ref)
                got = _nchw(got_raw, cout)
                assert int(got_raw[..., cout:].contiguous().view(torch.uint8).count_nonzero()) == 0, name
                if f8:
                    over, inside = ref.abs() >= 480.0, ref.abs() <= 448.0
                    assert torch.equal(got[over], 448.0 * ref[over].sign()), name
                    bound = 2 * ((K + 2) * 2.0 ** -24 * S + 2.0 ** -4 * ref.abs() + 2.0 ** -10)
                    worst = float(((got - ref).abs() / bound)[inside].max())
                else:
                    bound = 2 * ((K + 2) * 2.0 ** -24 * S + 2.0 ** -11 * ref.abs() + 2.0 ** -24)
                    worst = float(((got - ref).abs() / bound).max())
            assert torch.isfinite(got).all(), name
            assert worst <= 1.0, (name, worst)
            worst_all = max(worst_all, worst)
        elif op == "cast":
            c = r["c"]
            want = (src[..., :c].float() * torch.tensor(np.float32(r["scale"]))).clamp(-448.0, 448.0).to(F8)
            assert torch.equal(got_raw[..., :c].contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)), name
            assert int(got_raw[..., c:].contiguous().view(torch.uint8).count_nonzero()) == 0, name
        elif op == "maxpool":
            want = F.max_pool2d(_dec(src).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
            assert torch.equal(_dec(got_raw), want), name
        elif op == "avgpool":
            assert f8
            xs = _dec(src)
            scale, HWn = float(np.float32(r["scale"])), src.shape[1] * src.shape[2]
            ref = xs.mean(dim=(1, 2)) * scale
            bound = 2 * ((HWn + 1) * 2.0 ** -24 * xs.abs().mean(dim=(1, 2)) * scale + 2.0 ** -11 * ref.abs())
            # below fp16's smallest normal number the output's spacing is 2^-24 whatever |ref| is (module docstring)
            bound = torch.where(ref.abs() < 2.0 ** -14, bound + 2 * 2.0 ** -25, bound)
            got = got_raw.double().view(ref.shape[0], -1)[:, :ref.shape[1]]
            bad = (got - ref).abs() > bound
            if bool(bad.any()):
                print(f"\n{name}: {int(bad.sum())} of {bad.numel()} outside the bound; ref {ref[bad][:8].tolist()} "
                      f"got {got[bad][:8].tolist()} bound {bound[bad][:8].tolist()}")
            assert not bool(bad.any()), name
        elif op == "broadcast":
            assert f8
            c = r["c"]
            v = src.view(src.shape[0], -1)[:, :c]
            want = (v.float() * torch.tensor(np.float32(r["scale"]))).clamp(-448.0, 448.0).to(F8).view(torch.uint8)
            assert torch.equal(got_raw[..., :c].contiguous().view(torch.uint8),
                               want.view(v.shape[0], 1, 1, c).expand(got_raw[..., :c].shape)), name
            assert int(got_raw[..., c:].contiguous().view(torch.uint8).count_nonzero()) == 0, name
        else:
            raise AssertionError(f"unexpected record {op} in an fp8 plan")
        checked[op] = checked.get(op, 0) + 1
        # the record's bytes land in its slice of the destination buffer
        if r["dst"] >= 0:
            h, w = hw[r["dst"]]
            if r["dst"] not in bufs:
                dt = F8 if eng.buffer_fmt[r["dst"]] == "f8" else torch.float16
                bufs[r["dst"]] = torch.zeros((N, h, w, eng.buffers[r["dst"]]), dtype=torch.uint8 if dt == F8 else dt)
                if dt == F8:
                    bufs[r["dst"]] = bufs[r["dst"]].view(F8)
            y_off = r.get("y_off", 0)
            bufs[r["dst"]][..., y_off:y_off + got_raw.shape[-1]] = got_raw.view(N, h, w, -1)
    return checked, worst_all


@pytest.mark.parametrize("tag", TAGS)
def test_every_record_replays_within_its_kernel_bound(tag, tmp_path_factory, cuda, capsys):
    m, x, cfg, eng16, amax, eng8, trace = _setup(tag, tmp_path_factory)
    checked, worst = _replay(eng8, trace, *x.shape[0:1], *x.shape[2:])
    with capsys.disabled():
        print(f"\nfp8 replay {tag}: {checked}, worst conv err/bound {worst:.3f}")
    assert sum(checked.values()) == len(eng8.plan)
    assert checked["conv"] >= 50 and checked["cast"] == 1 and checked["maxpool"] == 1
    if tag != "simple_r50_4x64x64":
        assert checked["avgpool"] == 1 and checked["broadcast"] == 1
    if tag == "slim":
        assert any(r["cout"] % 16 for r in eng8.conv_records())


def _compare(tag, tmp_path_factory, cuda):
    from dcfp_amd import evaluate as ev
    m, x, cfg, eng16, amax, eng8, trace = _setup(tag, tmp_path_factory)
    ref, d = f8ref.distances(m.state_dict(), x, cfg, amax)
    e, r = max(v[0] for v in d), max(v[1] for v in d)
    xd = x.to(cuda)
    low = eng8.lowres_logits(xd)[0]
    assert low.dtype == torch.float32 and tuple(low.shape) == tuple(ref.shape)
    got = low.double().cpu()
    rel = float((got - ref).norm() / ref.norm())
    err = float((got - ref).abs().max())
    dis = float((got.argmax(1) != ref.argmax(1)).double().mean())
    print(f"\nfp8 deploy {tag}: |logits| <= {float(ref.abs().max()):.0f}; emulations (fp64 / fp32 sums) rel-L2 "
          f"{d[0][1]:.3e} / {d[1][1]:.3e}, max-abs {d[0][0]:.1f} / {d[1][0]:.1f}, label disagreement "
          f"{100 * d[0][2]:.1f} % / {100 * d[1][2]:.1f} %; engine rel-L2 {rel:.3e} max-abs {err:.1f} "
          f"label disagreement {100 * dis:.1f} %")
    assert torch.isfinite(got).all()
    assert rel <= 1.5 * r, (rel, r)
    assert err <= 3 * e, (err, e)
    labels = ev.predict_labels(eng8, xd)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (x.shape[0],) + tuple(x.shape[2:])
    full = eng8(xd)
    assert isinstance(full, list) and tuple(full[0].shape) == (x.shape[0], 19) + tuple(x.shape[2:])


@pytest.mark.parametrize("tag", TAGS)
def test_engine_logits_against_fp64(tag, tmp_path_factory, cuda, capsys):
    with capsys.disabled():
        _compare(tag, tmp_path_factory, cuda)


def test_saved_engines_of_both_formats_give_bit_identical_logits(tmp_path_factory, tmp_path, cuda):
    from dcfp_amd import deploy
    m, x, cfg, eng16, amax, eng8, trace = _setup("v3_r50_2x65x65", tmp_path_factory)
    xd = x.to(cuda)
    a = eng8.lowres_logits(xd)[0].clone()
    assert torch.equal(trace[eng8.plan[-1]["name"]], a.cpu())
    assert torch.equal(deploy.load_engine(eng8.state_dict(), cuda).lowres_logits(xd)[0], a)
    path = str(tmp_path / "engine_fp8.pth")
    torch.save(eng8.state_dict(), path)
    assert torch.equal(deploy.load_engine(path, cuda).lowres_logits(xd)[0], a)
    assert torch.equal(eng8.lowres_logits(xd)[0], a)              # buffers reused across calls: same bits
    small = eng8.lowres_logits(xd[:1, :, :33, :41])[0]            # another input shape, then the first one again
    assert tuple(small.shape) == (1, 19, 5, 6)
    assert torch.equal(eng8.lowres_logits(xd)[0], a)
    # an fp16 engine as it was saved before format 2 existed: the five keys, format 1
    st = eng16.state_dict()
    old = {"format": 1, "meta": st["meta"], "plan": st["plan"], "buffers": st["buffers"], "tensors": st["tensors"]}
    assert sorted(st) == sorted(old) and st["format"] == 1
    path16 = str(tmp_path / "engine_fp16.pth")
    torch.save(old, path16)
    assert torch.equal(deploy.load_engine(path16, cuda).lowres_logits(xd)[0], eng16.lowres_logits(xd)[0])


def test_evaluate_tool_runs_on_a_saved_fp8_engine(tmp_path_factory, tmp_path, cuda):
    m, x, cfg, eng16, amax, eng8, trace = _setup("simple_r50_4x64x64", tmp_path_factory)
    path, snap = str(tmp_path / "engine_fp8.pth"), str(tmp_path / "snap")
    torch.save(eng8.state_dict(), path)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), "--engine-file", path, "--input-size", "65,65",
           "--whole", "True", "--batch-size", "2", "--num-images", "4", "--snapshot-dir", snap]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "meanIU" in r.stdout and "float8_e4m3fn" in r.stdout
    assert open(os.path.join(snap, "result.txt")).read().splitlines()[-1] == "--------"
