"""GPU: tools/evaluate.py --dataset CS end to end as a child process, on five generated 60x90 image / label PNG pairs
with raw Cityscapes ids: every labelled pixel is counted exactly once (the 8k+1 padding is cropped, no file is
dropped or repeated) - through the fused vote, with --longsize, over two ranks and through the unfused path."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
H, W, FILES = 60, 90, 5
COMMON = ["--model", "simple", "--backbone", "resnet50", "--dataset", "CS", "--whole", "True", "--ms", "0.75,1",
          "--flip", "True", "--num-workers", "2"]
VARIANTS = {
    "fused": ["--batch-size", "1", "--save-predict", "True"],
    "longsize": ["--batch-size", "1", "--longsize", "120"],
    "unfused": ["--batch-size", "1", "--fused-vote", "False"],
}
_done = {}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (root, list file, number of labelled pixels computed on the host through the id table)."""
    from PIL import Image
    from dcfp_amd.datasets import cs
    root = tmp_path_factory.mktemp("cs_val")
    rng = np.random.RandomState(3)
    lines, labelled = [], 0
    table = np.full(256, 255, dtype=np.uint8)
    for raw, train in cs._TRAIN_IDS.items():
        table[raw] = train
    for i in range(FILES):
        image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        label = np.zeros((H, W), dtype=np.uint8)
        for _ in range(12):                                   # rectangles of raw ids 0 .. 33, classes and void alike
            y, x = rng.randint(0, H - 8), rng.randint(0, W - 8)
            label[y:y + rng.randint(8, 30), x:x + rng.randint(8, 40)] = rng.randint(0, 34)
        Image.fromarray(image).save(str(root / ("im%d_leftImg8bit.png" % i)))
        Image.fromarray(label).save(str(root / ("im%d_gtFine_labelIds.png" % i)))
        lines.append("im%d_leftImg8bit.png im%d_gtFine_labelIds.png" % (i, i))
        labelled += int((table[label] != 255).sum())
    lst = root / "val.lst"
    lst.write_text("\n".join(lines) + "\n")
    assert 0 < labelled < FILES * H * W
    return str(root), str(lst), labelled


def command(data, snap, extra):
    para = json.dumps({"root": data[0], "list_path": data[1]})
    return [sys.executable, os.path.join(ROOT, "tools", "evaluate.py")] + COMMON + ["--data-para", para,
                                                                                     "--snapshot-dir", snap] + extra


def records(snap):
    lines = open(os.path.join(snap, "result.txt")).read().splitlines()
    assert lines[0].startswith("test with") and lines[-1] == "--------"
    assert sum(l.startswith("test with") for l in lines) == 1
    return [json.loads(l) for l in lines if l.startswith("{")]


def run_tool(name, data, tmp_path_factory):
    """One run per variant and session: (records of result.txt, stdout, snapshot directory)."""
    if name not in _done:
        snap = str(tmp_path_factory.mktemp("evalds_" + name))
        r = subprocess.run(command(data, snap, VARIANTS[name]), capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        _done[name] = (records(snap), r.stdout, snap)
    return _done[name]


def test_fused_vote_counts_every_labelled_pixel_once(data, tmp_path_factory):
    from PIL import Image
    from dcfp_amd.datasets import cs
    recs, stdout, snap = run_tool("fused", data, tmp_path_factory)
    assert len(recs) == 4
    iou, prec, rec, tail = recs
    assert 0.0 <= iou["meanIU"] <= 1.0 and len(iou["IU_array"]) == 19
    assert len(prec["p"]) == 19 and len(rec["r"]) == 19
    assert tail["iou_type"] == "segm" and tail["FPS"] > 0 and tail["images"] == 1      # 5 batches: 4 warm-up, 1 timed
    assert sum(tail["pos"]) == data[2]
    assert sum(tail["res"]) == data[2] and sum(tail["tp"]) <= data[2]
    assert "'meanIU'" in stdout and "'IU_array'" in stdout and "Iter5/5" in stdout
    palette = [int(v) for v in cs.DataSet(data[0], data[1], split="val").cmap_labels.reshape(-1)]
    for i in range(FILES):
        with Image.open(os.path.join(snap, "outputs", "im%d_gtFine_labelIds.png" % i)) as im:
            assert im.mode == "P" and im.size == (W, H)
            assert im.getpalette()[:57] == palette
            assert int(np.asarray(im).max()) < 19
    assert len(os.listdir(os.path.join(snap, "outputs"))) == FILES


def test_longsize_counts_the_same_pixels(data, tmp_path_factory):
    tail = run_tool("longsize", data, tmp_path_factory)[0][3]
    assert sum(tail["pos"]) == data[2]


def test_unfused_path_counts_the_same_pixels(data, tmp_path_factory):
    tail = run_tool("unfused", data, tmp_path_factory)[0][3]
    assert sum(tail["pos"]) == data[2]


def test_two_ranks_sum_to_the_single_process_matrix(data, tmp_path_factory):
    """Two ranks sharing the GPU (gloo): one image per rank and step, as in the single-process run."""
    single = run_tool("fused", data, tmp_path_factory)[0][3]
    snap = str(tmp_path_factory.mktemp("evalds_ranks"))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = command(data, snap, ["--batch-size", "2", "--dist-backend", "gloo"])
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=env))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-3000:]
    tail = records(snap)[3]                                        # one set of records: rank 0's
    for key in ("tp", "pos", "res"):
        assert tail[key] == single[key], key
    assert "'meanIU'" in outs[0][0] and "'meanIU'" not in outs[1][0]
    sums = [json.loads(l) for l in outs[0][0].splitlines() if l.startswith('{"tp"')]
    assert sums == [{"tp": int(sum(single["tp"])), "pos": int(sum(single["pos"])), "res": int(sum(single["res"]))}]
