"""bench.py end to end at a toy size: a plain run prints the headline and leaves out everything that takes runs of its
own; --full adds the roofline of one instrumented step (with its per-kernel detail) and the CPU baseline."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--size", "64,128"]


def _bench(argv):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + TOY + argv, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines                   # ONE JSON line on stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_rest(cuda):
    plain = _bench([])
    assert plain["value"] > 0 and plain["unit"] == "images/s" and plain["higher_is_better"] is True
    assert plain["ms_per_step"] > 0 and plain["dtype"] == "f32" and plain["steps"] == 2 and plain["warmup"] == 1
    assert [k for k in ("roofline", "detail", "cpu_baseline", "direct_conv", "alt_math") if plain[k] is not None] == []
    full = _bench(["--full", "--cpu-sample", "2,64,128"])
    assert full["value"] > 0 and full["ms_per_step"] > 0
    assert full["roofline"]["unit"] == "TFLOP/s" and full["roofline"]["achieved"] > 0
    assert full["detail"]["conv_kernels"]
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["kind"] == "port"
