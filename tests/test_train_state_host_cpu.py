"""CPU: the host side of resumable training (dcfp_amd/train_state.py) - the refusals of a state file that
belongs to another run or is damaged, the argument checks of tools/train.py, the scorers' and the loader's state round
trips, and the atomic write.  Every comparison is torch.equal / ==."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

from dcfp_amd import networks, pruners, train_state  # noqa: E402
from dcfp_amd.datasets import TrainLoader, build_dataset  # noqa: E402


def train_tool():
    import importlib
    return importlib.import_module("train")


def parser_with_continue(monkeypatch):
    from dcfp_amd.engine import Engine
    train = train_tool()
    p = train.get_parser()
    monkeypatch.setattr(sys, "argv", ["train.py"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    Engine(custom_parser=p)                       # adds -c/--continue, as main() does
    return train, p


def tiny_model(width=4):
    return torch.nn.Sequential(torch.nn.Conv2d(3, width, 3), torch.nn.BatchNorm2d(width))


def make_fp(argv=(), width=4, world=1):
    args = train_tool().get_parser().parse_args(list(argv))
    return train_state.fingerprint(args, tiny_model(width), 19, world)


# ------------------------------------------------------------------ fingerprint
def test_equal_fingerprints_pass():
    train_state.check_fingerprint(make_fp(), make_fp())


@pytest.mark.parametrize("argv,width,world,field,old,new", [
    (["--num-steps", "7"], 4, 1, "num_steps", "40000", "7"),
    (["--optim", "adamw"], 4, 1, "optim", "'sgd'", "'adamw'"),
    ([], 5, 1, "0.weight", "[4, 3, 3, 3]", "[5, 3, 3, 3]"),
    ([], 4, 2, "world_size", "1", "2"),
])
def test_fingerprint_refusal_names_the_field_and_both_values(argv, width, world, field, old, new):
    with pytest.raises(ValueError) as e:
        train_state.check_fingerprint(make_fp(), make_fp(argv, width, world))
    msg = str(e.value)
    assert field in msg and old in msg and new in msg, msg


def test_fingerprint_names_a_parameter_that_is_missing():
    saved, cur = make_fp(), make_fp()
    cur["params"] = cur["params"][1:]
    with pytest.raises(ValueError, match="0.weight"):
        train_state.check_fingerprint(saved, cur)


# ------------------------------------------------------------------ the file
def small_state(tag=1.0):
    return {"format": train_state.FORMAT, "iteration": 3, "model": {"w": torch.full((300,), tag)}, "optimizer": {},
            "scorer": None, "ranks": [], "fingerprint": make_fp(), "digests": {}}


def test_save_load_round_trip(tmp_path):
    path = str(tmp_path / "train_state_3.pth")
    train_state.save(small_state(2.0), path)
    back = train_state.load(path)
    assert back["iteration"] == 3 and torch.equal(back["model"]["w"], torch.full((300,), 2.0))
    assert os.listdir(tmp_path) == ["train_state_3.pth"]


def test_truncated_file_is_refused(tmp_path):
    path = str(tmp_path / "s.pth")
    train_state.save(small_state(), path)
    blob = open(path, "rb").read()
    with open(path, "wb") as f:
        f.write(blob[:len(blob) // 2])
    with pytest.raises(RuntimeError, match="truncated"):
        train_state.load(path)
    with open(path, "wb") as f:
        pass
    with pytest.raises(RuntimeError, match="truncated"):
        train_state.load(path)


def test_unknown_format_and_plain_checkpoint_are_refused(tmp_path):
    path = str(tmp_path / "s.pth")
    st = small_state()
    st["format"] = 99
    torch.save(st, path)
    with pytest.raises(RuntimeError, match="format 99"):
        train_state.load(path)
    torch.save({"conv.weight": torch.zeros(3)}, path)           # what --resume takes
    with pytest.raises(RuntimeError, match="not a state file"):
        train_state.load(path)


def test_a_save_that_dies_midway_leaves_the_previous_file(tmp_path, monkeypatch):
    path = str(tmp_path / "train_state_3.pth")
    train_state.save(small_state(1.0), path)
    real = torch.save

    def dying(obj, f, *a, **k):
        f.write(b"half a file")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", dying)
    with pytest.raises(OSError, match="disk full"):
        train_state.save(small_state(5.0), path)
    fresh = str(tmp_path / "train_state_6.pth")
    with pytest.raises(OSError, match="disk full"):
        train_state.save(small_state(5.0), fresh)
    monkeypatch.setattr(torch, "save", real)
    assert os.listdir(tmp_path) == ["train_state_3.pth"]        # no partial file, no temporary left, no new final name
    assert torch.equal(train_state.load(path)["model"]["w"], torch.full((300,), 1.0))


def test_prune_old_keeps_the_newest(tmp_path):
    for k in (3, 6, 9, 12):
        train_state.save(small_state(), train_state.state_path(str(tmp_path), k))
    (tmp_path / "train_state_x.pth").write_text("not ours")
    gone = train_state.prune_old(str(tmp_path), 2)
    assert sorted(os.path.basename(p) for p in gone) == ["train_state_3.pth", "train_state_6.pth"]
    assert sorted(os.listdir(tmp_path)) == ["train_state_12.pth", "train_state_9.pth", "train_state_x.pth"]


# ------------------------------------------------------------------ tools/train.py arguments
def test_continue_refuses_resume_and_start_iters(monkeypatch):
    train, p = parser_with_continue(monkeypatch)
    train.check_args(p.parse_args(["--continue", "s.pth"]))
    train.check_args(p.parse_args(["-c", "s.pth", "--state-every", "3", "--keep-states", "1", "--log-digest", "1"]))
    with pytest.raises(ValueError, match="--resume"):
        train.check_args(p.parse_args(["--continue", "s.pth", "--resume", "w.pth"]))
    with pytest.raises(ValueError, match="--start-iters"):
        train.check_args(p.parse_args(["--continue", "s.pth", "--start-iters", "3"]))
    with pytest.raises(ValueError):
        train.check_args(p.parse_args(["--state-every", "-1"]))
    a = p.parse_args([])
    assert a.state_every == 0 and a.keep_states == 2 and a.log_digest == 0 and a.continue_fpath is None


# ------------------------------------------------------------------ scorers
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(3)
    return networks.simple.Seg_Model(backbone="resnet50", backbone_para={"pretrained": False}, num_classes=19,
                                     align_corner=True, criterion=None, deepsup=True)


def random_scores(p, model, seed):
    g = torch.Generator().manual_seed(seed)
    mods = dict(model.named_modules())
    return {n: torch.rand(mods[n].weight.numel(), generator=g) for n in p._names}


def test_dcfp_scorer_round_trips_through_set_eic(model, tmp_path):
    a = pruners.dcfp_pruning(model, 0.999)
    want = random_scores(a, model, 5)
    a.set_eic({"eic": {n: v.clone() for n, v in want.items()}})
    state = train_state._cpu(train_state.scorer_state(a))
    b = pruners.dcfp_pruning(model, 0.999)
    assert all(v == 0 for v in b.get_eic()["eic"].values())
    b.set_eic(state)
    got = b.get_eic()["eic"]
    assert list(got) == list(want) and all(torch.equal(got[n], want[n]) for n in want)
    b.export_eic(str(tmp_path / "score.pth"))
    f = torch.load(str(tmp_path / "score.pth"))["eic"]
    assert all(torch.equal(f[n], want[n]) for n in want)
    assert b.state_dict is b.get_eic()                       # the reference's attribute keeps its name and its kind
    with pytest.raises(ValueError):
        b.set_eic({"eic": dict(list(want.items())[1:])})
    fresh = pruners.dcfp_pruning(model, 0.999)
    fresh.set_eic({"eic": {n: 0 for n in want}})             # a state taken before the first step
    assert all(v == 0 for v in fresh.get_eic()["eic"].values())


def test_taylor_scorer_round_trips_through_set_state(model, tmp_path):
    a = pruners.taylor_pruning(model, "gate")
    want = random_scores(a, model, 6)
    a.set_state({"eic": {n: v.clone() for n, v in want.items()}, "steps": 5, "criterion": "taylor"})
    state = train_state._cpu(train_state.scorer_state(a))
    assert state["steps"] == 5 and state["criterion"] == "taylor"
    b = pruners.taylor_pruning(model, "gate")
    b.set_state(state)
    assert b.steps == 5 and all(torch.equal(b.get_eic()["eic"][n], want[n]) for n in want)
    sa, sb = a.scores(), b.scores()
    assert all(torch.equal(sa[n], sb[n]) and torch.equal(sb[n], want[n] / 5) for n in want)
    with pytest.raises(ValueError, match="criterion"):
        pruners.taylor_pruning(model, "weight").set_state(state)
    bad = dict(state, eic=dict(state["eic"]))
    first = next(iter(bad["eic"]))
    bad["eic"][first] = torch.zeros(bad["eic"][first].numel() + 1)
    with pytest.raises(ValueError, match=first):
        b.set_state(bad)


# ------------------------------------------------------------------ loader
def write_cs(root, n, size=(12, 20)):
    from PIL import Image
    rs = np.random.RandomState(0)
    lines = []
    for i in range(n):
        Image.fromarray(rs.randint(0, 256, size + (3,)).astype(np.uint8)).save(root / ("im%d.png" % i))
        Image.fromarray(rs.randint(0, 34, size).astype(np.uint8)).save(root / ("gt%d.png" % i))
        lines.append("im%d.png gt%d.png" % (i, i))
    (root / "train.lst").write_text("\n".join(lines) + "\n")
    return {"root": str(root), "list_path": str(root / "train.lst")}


class RecordingLoader(TrainLoader):
    """TrainLoader up to the device: `apply` hands back the draws and the batch's indices instead of launching."""

    def apply(self, decoded, params, idx=None, sources=None, target=None):
        return [tuple(sorted(vars(p).items())) if hasattr(p, "__dict__") else p for p in params], list(idx)


def make_loader(para):
    ds = build_dataset("CS", split="train", crop_size=(8, 8), scale=True, mirror=True, brightness=True, balance=1,
                       data_para=para)
    decoded = []
    real = ds.decode

    def decode(i):
        decoded.append(i)
        return real(i)
    ds.decode = decode
    return RecordingLoader(ds, 2, torch.device("cpu"), seed=11, num_workers=1, rank=0, world_size=1), decoded


def take(loader, n):
    out = []
    while len(out) < n:
        for batch in loader:
            out.append(batch)
            if len(out) == n:
                break
    return out


@pytest.mark.parametrize("k", [0, 2, 3, 4, 6])
def test_loader_state_continues_the_draws(tmp_path, k):
    """7 files in batches of 2: 3 batches per epoch.  k = 2 and 4 cut inside an epoch, 3 and 6 on a boundary."""
    para = write_cs(tmp_path, 7)
    total = 8
    whole, _ = make_loader(para)
    assert len(whole) == 3

    def endless(loader):
        while True:
            yield from loader
    it = endless(whole)
    want, state = [], None
    for b in range(total):
        if b == k:
            state = whole.state_dict()
        want.append(next(it))
    assert state["epoch"] == k // 3 and state["batch"] == k % 3
    assert len({str(w[0]) for w in want}) == total                  # the draws differ from batch to batch
    cont, decoded = make_loader(para)
    cont.load_state_dict(torch.load(_saved(tmp_path, state), weights_only=False))
    it = endless(cont)
    got = [next(it) for _ in range(total - k)]
    assert got == want[k:]
    # decoding starts at the cursor and never goes back before it (one worker: files are decoded in submission order)
    served = cont.indices(k // 3)[2 * (k % 3):6] + [i for e in range(k // 3 + 1, 4) for i in cont.indices(e)[:6]]
    seen = list(decoded)
    assert len(seen) >= 2 * (total - k) and seen == served[:len(seen)]


def _saved(tmp_path, state):
    """Through torch.save, as the state file carries it (the generator's tuple comes back as it went)."""
    path = str(tmp_path / "loader_state.pth")
    torch.save({"s": state}, path)
    torch.save(torch.load(path, weights_only=False)["s"], path)
    return path


def test_loader_refuses_a_cursor_outside_the_epoch(tmp_path):
    loader, _ = make_loader(write_cs(tmp_path, 7))
    st = loader.state_dict()
    with pytest.raises(ValueError):
        loader.load_state_dict(dict(st, batch=3))
