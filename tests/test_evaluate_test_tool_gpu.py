"""GPU: tools/evaluate_test.py end to end as a child process, on five generated 60x90 image / label PNG pairs with raw
Cityscapes ids and a `val.lst` and a `test.lst` over the same images: its `test_pred` PNGs - deflated on the device and
written through PIL - decode to what `tools/evaluate.py --save-predict True` wrote for the same image, its `test_id`
PNGs are the reverse id table applied to them, names and counts follow the reference, and --longsize returns to the
file's own size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
H, W, FILES = 60, 90, 5
COMMON = ["--model", "simple", "--backbone", "resnet50", "--dataset", "CS", "--whole", "True", "--ms", "0.75,1",
          "--flip", "True", "--num-workers", "2", "--batch-size", "1", "--seed", "4321"]
VARIANTS = {                        # name -> (tool, list, options)
    "evaluate": ("evaluate.py", "val", ["--save-predict", "True"]),
    "device": ("evaluate_test.py", "test", ["--device-png", "True"]),
    "pil": ("evaluate_test.py", "test", ["--device-png", "False"]),
    "evaluate_device": ("evaluate.py", "val", ["--save-predict", "True", "--device-png", "True"]),
    "evaluate_long": ("evaluate.py", "val", ["--save-predict", "True", "--longsize", "120"]),
    "device_long": ("evaluate_test.py", "test", ["--device-png", "True", "--longsize", "120"]),
}
_done = {}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """-> (root, {'val': list file, 'test': list file})."""
    from PIL import Image
    root = tmp_path_factory.mktemp("cs_test")
    rng = np.random.RandomState(3)
    val, test = [], []
    for i in range(FILES):
        image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        label = np.zeros((H, W), dtype=np.uint8)
        for _ in range(12):
            y, x = rng.randint(0, H - 8), rng.randint(0, W - 8)
            label[y:y + rng.randint(8, 30), x:x + rng.randint(8, 40)] = rng.randint(0, 34)
        Image.fromarray(image).save(str(root / ("town_%06d_000019_leftImg8bit.png" % i)))
        Image.fromarray(label).save(str(root / ("town_%06d_000019_gtFine_labelIds.png" % i)))
        val.append("town_%06d_000019_leftImg8bit.png town_%06d_000019_gtFine_labelIds.png" % (i, i))
        test.append("town_%06d_000019_leftImg8bit.png" % i)
    (root / "val.lst").write_text("\n".join(val) + "\n")
    (root / "test.lst").write_text("\n".join(test) + "\n")
    return str(root), {"val": str(root / "val.lst"), "test": str(root / "test.lst")}


def run_tool(name, data, tmp_path_factory):
    """One run per variant and session -> the snapshot directory."""
    if name not in _done:
        tool, lst, extra = VARIANTS[name]
        snap = str(tmp_path_factory.mktemp("evaltest_" + name))
        para = json.dumps({"root": data[0], "list_path": data[1][lst]})
        cmd = [sys.executable, os.path.join(ROOT, "tools", tool)] + COMMON + ["--data-para", para, "--snapshot-dir",
                                                                              snap] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        _done[name] = snap
    return _done[name]


def decode(path):
    from PIL import Image
    with Image.open(path) as im:
        im.load()
        return im.mode, np.asarray(im).copy(), im.getpalette()


def check_against_evaluate(data, tmp_path_factory, ours, theirs):
    from dcfp_amd import evaluate
    from dcfp_amd.datasets import cs
    snap, ref = run_tool(ours, data, tmp_path_factory), run_tool(theirs, data, tmp_path_factory)
    table = evaluate.reverse_id_table(cs.DataSet(data[0], data[1]["test"], split="test"))
    pred_dir, id_dir = os.path.join(snap, "outputs", "test_pred"), os.path.join(snap, "outputs", "test_id")
    stems = ["town_%06d_000019" % i for i in range(FILES)]
    assert sorted(os.listdir(pred_dir)) == [s + "_leftImg8bit.png" for s in stems]
    assert sorted(os.listdir(id_dir)) == [s + ".png" for s in stems]
    for s in stems:
        mode, pred, palette = decode(os.path.join(pred_dir, s + "_leftImg8bit.png"))
        rmode, rpred, rpalette = decode(os.path.join(ref, "outputs", s + "_gtFine_labelIds.png"))
        assert mode == rmode == "P" and pred.shape == (H, W)
        assert np.array_equal(pred, rpred) and palette[:57] == rpalette[:57]
        assert int(pred.max()) < 19
        mode, ids, _ = decode(os.path.join(id_dir, s + ".png"))
        assert mode == "L" and np.array_equal(ids, table[pred])


def test_device_pngs_match_evaluate(data, tmp_path_factory):
    check_against_evaluate(data, tmp_path_factory, "device", "evaluate")


def test_pil_pngs_match_evaluate(data, tmp_path_factory):
    check_against_evaluate(data, tmp_path_factory, "pil", "evaluate")


def test_longsize_returns_to_the_file_size(data, tmp_path_factory):
    check_against_evaluate(data, tmp_path_factory, "device_long", "evaluate_long")


def test_evaluate_tool_writes_the_same_pngs_through_the_device(data, tmp_path_factory):
    """tools/evaluate.py --save-predict True --device-png True: the same files, the same images and palette."""
    ours, ref = (os.path.join(run_tool(n, data, tmp_path_factory), "outputs") for n in ("evaluate_device", "evaluate"))
    assert sorted(os.listdir(ours)) == sorted(os.listdir(ref)) and len(os.listdir(ours)) == FILES
    for name in os.listdir(ref):
        mode, pred, palette = decode(os.path.join(ours, name))
        rmode, rpred, rpalette = decode(os.path.join(ref, name))
        assert mode == rmode == "P" and np.array_equal(pred, rpred) and palette[:57] == rpalette[:57]
