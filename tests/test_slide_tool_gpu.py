"""GPU: tools/evaluate.py as a child process through the multi-scale + flip sliding-window path, once through the chain
(evaluate.predict_multiscale) and once with --fused-sliding True (evaluate.predict_sliding_vote): the same records, the
same ground-truth counts, and true positives that differ by at most the 0.5 % of the pixels that tests/test_slide_gpu.py
allows to be undecided."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
# the arguments of tests/test_evaluate_tool_gpu.py's ms_flip_sliding (its leading --whole True, which the later
# --whole False overrides, left out)
COMMON = ["--model", "simple", "--backbone", "resnet50", "--input-size", "65,65", "--batch-size", "2",
          "--num-images", "4", "--whole", "False", "--ms", "0.75,1", "--flip", "True"]


def run_tool(extra, snap):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "evaluate.py")] + COMMON + extra + ["--snapshot-dir", snap]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = open(os.path.join(snap, "result.txt")).read().splitlines()
    assert lines[0].startswith("test with") and lines[-1] == "--------"
    return [json.loads(l) for l in lines if l.startswith("{")], r.stdout


def test_fused_sliding_tool_against_the_chain(tmp_path):
    tails = {}
    for name, extra in (("fused", ["--fused-sliding", "True"]), ("chain", [])):
        recs, stdout = run_tool(extra, str(tmp_path / name))
        assert len(recs) == 4
        iou, prec, rec, tail = recs
        assert 0.0 <= iou["meanIU"] <= 1.0 and len(iou["IU_array"]) == 19
        assert all(0.0 <= v <= 1.0 for v in iou["IU_array"])
        assert len(prec["p"]) == 19 and len(rec["r"]) == 19 and 0.0 <= prec["meanP"] <= 1.0 and 0.0 <= rec["meanR"] <= 1.0
        assert tail["iou_type"] == "segm"
        assert tail["FPS"] > 0 and tail["images"] == 2                 # 2 batches: one warm-up, one timed
        assert sum(tail["pos"]) > 0
        assert "'meanIU'" in stdout and "'IU_array'" in stdout and "Iter2/2" in stdout
        tails[name] = tail
    assert tails["fused"]["pos"] == tails["chain"]["pos"]
    print("sum tp fused %d, chain %d, sum pos %d" % (sum(tails["fused"]["tp"]), sum(tails["chain"]["tp"]),
                                                     sum(tails["chain"]["pos"])))
    assert abs(sum(tails["fused"]["tp"]) - sum(tails["chain"]["tp"])) <= 0.005 * sum(tails["chain"]["pos"])
