"""bench.py --dump-outputs: what the last timed step computed, as DIR/<name>.npy (float32 / float64, at most 64 MB,
the same sample positions every time), and --steps / --warmup validation.  Host logic only: the model's tensors stand
on the CPU here, with gradients and scores filled in by hand."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _model_and_scores():
    from dcfp_amd import networks, pruners
    torch.manual_seed(0)
    m = networks.deeplabv3.Seg_Model(backbone="resnet50", backbone_para={"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128,
                                                                         "pretrained": False},
                                     num_classes=19, align_corner=True, deepsup=True)
    for p in m.parameters():
        p.grad = 2 * p.detach()
    mods = dict(m.named_modules())
    eic = {k: torch.rand(mods[k].weight.numel()) for k in pruners.dcfp_pruning(m, 0.999).state_dict["eic"]}
    return m, eic


def test_dump_outputs_files_dtypes_budget_and_fixed_sample(tmp_path):
    m, eic = _model_and_scores()
    total = bench.dump_outputs(str(tmp_path / "a"), 1.25, m, eic)
    bench.dump_outputs(str(tmp_path / "b"), 1.25, m, eic)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["bn_running.npy", "eic.npy", "grads.npy", "loss.npy", "params.npy"]
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    b = {n[:-4]: np.load(tmp_path / "b" / n) for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) == total <= 64 * 2**20
    assert all(np.array_equal(a[n], b[n]) for n in a)             # same positions from run to run
    assert a["loss"].tolist() == [1.25]
    assert np.array_equal(a["eic"], torch.cat(list(eic.values())).numpy())
    assert np.array_equal(a["grads"], 2 * a["params"])                # gradients sampled where the parameters are
    sizes = [p.numel() for p in m.parameters()]
    assert a["params"].size == sum(min(n, bench.DUMP_PER_TENSOR) for n in sizes)


def test_steps_must_be_positive():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    for argv in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 2 and "--steps must be at least 1" in r.stderr and r.stdout.strip() == "", argv


def test_alt_legs_need_full():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--alt-legs"], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and "--alt-legs is part of a --full run" in r.stderr and r.stdout.strip() == ""
