"""GPU: tools/evaluate.py end to end as a child process (like the train and prune tools in tests/_model_cases.py):
the reference's evaluate.py command line on synthetic piecewise-constant ground truth, with both IoU types, through the
fp16 engine, and through the multi-scale + flip + sliding-window path."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
COMMON = ["--model", "simple", "--backbone", "resnet50", "--input-size", "65,65", "--whole", "True", "--batch-size", "2",
          "--num-images", "4"]
VARIANTS = {
    "segm": ["--iou-type", "segm"],
    "boundary": ["--iou-type", "boundary"],
    "trt": ["--use-trt", "True"],
    "ms_flip_sliding": ["--whole", "False", "--ms", "0.75,1", "--flip", "True"],
}
_done = {}


def run_tool(name, tmp_path_factory):
    """One run per variant and session: (records of result.txt, stdout)."""
    if name not in _done:
        snap = str(tmp_path_factory.mktemp("eval_" + name))
        cmd = [sys.executable, os.path.join(ROOT, "tools", "evaluate.py")] + COMMON + VARIANTS[name] + ["--snapshot-dir", snap]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = open(os.path.join(snap, "result.txt")).read().splitlines()
        assert lines[0].startswith("test with") and lines[-1] == "--------"
        recs = [json.loads(l) for l in lines if l.startswith("{")]
        _done[name] = (recs, r.stdout)
    return _done[name]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_evaluate_tool(name, tmp_path_factory):
    recs, stdout = run_tool(name, tmp_path_factory)
    assert len(recs) == 4
    iou, prec, rec, tail = recs
    assert 0.0 <= iou["meanIU"] <= 1.0 and len(iou["IU_array"]) == 19
    assert all(0.0 <= v <= 1.0 for v in iou["IU_array"])
    assert len(prec["p"]) == 19 and len(rec["r"]) == 19 and 0.0 <= prec["meanP"] <= 1.0 and 0.0 <= rec["meanR"] <= 1.0
    assert tail["iou_type"] == ("boundary" if name == "boundary" else "segm")
    assert tail["FPS"] > 0 and tail["images"] == 2                 # 2 batches: one warm-up, one timed
    assert sum(tail["pos"]) > 0
    assert "'meanIU'" in stdout and "'IU_array'" in stdout and "Iter2/2" in stdout


def test_boundary_counts_are_bounded_by_segm_counts(tmp_path_factory):
    """Same seed, same model: a boundary true positive is a pixel where ground truth and prediction agree, so per class
    the boundary run counts at most the segm run's true positives and ground-truth pixels."""
    segm = run_tool("segm", tmp_path_factory)[0][3]
    bnd = run_tool("boundary", tmp_path_factory)[0][3]
    assert all(b <= s for b, s in zip(bnd["tp"], segm["tp"]))
    assert all(b <= s for b, s in zip(bnd["pos"], segm["pos"]))
    assert 0 < sum(bnd["pos"]) < sum(segm["pos"])                  # d = 2 at 65x65: rectangles keep an interior
