"""GPU: a run that is stopped and continued leaves the bits of the run that never stopped (dcfp_amd/train_state.py,
tools/train.py --state-every / -c/--continue).

Every case makes three runs of tools/train.py into three directories: A uninterrupted (writing states), A' the same
command again - the CONTROL: if A' differs from A the failure is a determinism finding about the named tensor, not about
this feature - and B, continued from a state of A.  Then every tensor of the final checkpoint, of score.pth and of the
final state file (optimizer arenas, scorer, generators) is compared with torch.equal, and the `--log-digest 1` lines of B
with the tail of A's.  There is no tolerance anywhere in this file.

The driver is loaded with importlib and run by main(argv); one case runs it in fresh processes (no process-global cache
is silently part of the state), one as two ranks sharing the GPU over gloo (tests/test_ddp2_gpu.py's way)."""
import contextlib
import importlib
import io
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

BB = '{"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128, "pretrained": false}'
SLIM_CFG = os.path.join(ROOT, "tools", "data", "channel_cfg_r101_p60_synthetic.pth")
PORT = "29561"


def common(backbone="resnet50", batch=2):
    return ["--model", "deeplabv3", "--backbone", backbone, "--backbone-para", BB, "--input-size", "65,65",
            "--batch-size", str(batch), "--deepsup", "True", "--log-digest", "1"]


def run(argv):
    """main(argv) of tools/train.py in this process -> its `digest` lines."""
    train = importlib.import_module("train")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        train.main(argv)
    return digest_lines(out.getvalue())


def digest_lines(text):
    return [l for l in text.splitlines() if l.startswith("digest it=")]


def differences(a, b, path=""):
    """Paths at which two nested structures of tensors / numbers differ (torch.equal on tensors)."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        ok = isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype \
            and a.shape == b.shape and torch.equal(a, b)
        if ok and a.is_floating_point():                      # torch.equal holds +0 == -0: compare the bits as well
            ok = bool((a.reshape(-1).contiguous().view(torch.uint8) == b.reshape(-1).contiguous().view(torch.uint8)).all())
        return [] if ok else [path]
    if isinstance(a, dict) and isinstance(b, dict):
        if list(a) != list(b):
            return [path + " (keys)"]
        return [d for k in a for d in differences(a[k], b[k], "%s/%s" % (path, k))]
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return [path + " (length)"]
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, "%s/%d" % (path, i))]
    return [] if a == b else [path]


def load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def same_run(da, db, steps, what, score=True):
    """Everything run `db` left at `steps` equals what run `da` left: the checkpoint, score.pth and the state file."""
    names = ["CS_scenes_%d.pth" % steps, "train_state_%d.pth" % steps] + (["score.pth"] if score else [])
    for name in names:
        a, b = load(os.path.join(da, name)), load(os.path.join(db, name))
        if name.startswith("train_state"):
            a, b = dict(a), dict(b)
            assert a["iteration"] == b["iteration"] == steps
            for part in ("model", "optimizer", "scorer", "ranks", "digests", "fingerprint"):
                diff = differences(a[part], b[part], part)
                assert not diff, "%s: %s of %s differs at %s" % (what, part, name, diff[:5])
        else:
            diff = differences(a, b)
            assert not diff, "%s: %s differs at %s" % (what, name, diff[:5])


def three_runs(tmp_path, argv, steps, cut, every):
    """A, A' and B of one case; returns the directories and the digest lines of A."""
    da, dc, db = (str(tmp_path / n) for n in ("A", "A2", "B"))
    head = argv + ["--num-steps", str(steps), "--state-every", str(every), "--keep-states", "100"]
    la = run(head + ["--snapshot-dir", da])
    lc = run(head + ["--snapshot-dir", dc])
    assert len(la) == steps and la[-1].startswith("digest it=%d params=" % steps) and len(la[-1].split("=")[-1]) == 33
    assert la == lc, "CONTROL: the same command twice gives other parameter digests - a determinism finding"
    same_run(da, dc, steps, "CONTROL (the same command twice; a determinism finding, not the feature)",
             score="--prune-type" in argv)
    lb = run(head + ["--snapshot-dir", db, "--continue", os.path.join(da, "train_state_%d.pth" % cut)])
    assert lb == la[cut:], (lb, la[cut:])
    same_run(da, db, steps, "continued at %d" % cut, score="--prune-type" in argv)
    assert not os.path.exists(os.path.join(db, "train_state_%d.pth" % cut))      # B wrote only what it ran
    return da, db, la


# ------------------------------------------------------------------ case 1 (shared with cases 5 and 7)
CASE1 = common() + ["--optim", "sgd", "--prune-type", "dcfp", "--save-steps", "3", "--save-pred-every", "3"]


@pytest.fixture(scope="module")
def case1(cuda, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("case1")
    da, db, la = three_runs(tmp, CASE1, 6, 3, 3)
    return tmp, da, db, la


def test_sgd_dcfp_continues_bit_identically_and_resume_does_not(case1):
    tmp, da, db, la = case1
    assert sorted(f for f in os.listdir(da) if f.startswith("train_state")) == ["train_state_3.pth", "train_state_6.pth"]
    st = load(os.path.join(da, "train_state_3.pth"))
    assert st["format"] == 1 and st["iteration"] == 3 and len(st["ranks"]) == 1
    assert set(st["digests"]) == {"flat_param", "momentum", "scorer"}
    assert all(not t.is_cuda for t in st["model"].values())
    # today's way - weights and the step counter only - does NOT reproduce A: the comparison above is not vacuous
    dr = str(tmp / "R")
    lr = run(CASE1 + ["--num-steps", "6", "--snapshot-dir", dr, "--resume", os.path.join(da, "CS_scenes_3.pth"),
                      "--start-iters", "3"])
    assert len(lr) == 3 and lr != la[3:]
    assert differences(load(os.path.join(da, "CS_scenes_6.pth")), load(os.path.join(dr, "CS_scenes_6.pth")))
    assert differences(load(os.path.join(da, "score.pth")), load(os.path.join(dr, "score.pth")))


def test_keep_states_deletes_the_older_files(cuda, tmp_path):
    d = str(tmp_path / "K")
    run(common() + ["--num-steps", "3", "--state-every", "1", "--keep-states", "1", "--snapshot-dir", d])
    assert sorted(f for f in os.listdir(d) if f.startswith("train_state")) == ["train_state_3.pth"]


# ------------------------------------------------------------------ case 7: restore verification
def test_a_corrupted_momentum_value_is_caught_by_the_digest(case1, tmp_path):
    _, da, _, _ = case1
    st = load(os.path.join(da, "train_state_3.pth"))
    buf = st["optimizer"]["state"][0]["momentum_buffer"]
    buf.view(-1)[0] = buf.view(-1)[0] + 1.0
    bad = str(tmp_path / "bad_state.pth")
    torch.save(st, bad)                                           # (with the digests of the uncorrupted state)
    with pytest.raises(RuntimeError, match="momentum buffer"):
        run(CASE1 + ["--num-steps", "6", "--snapshot-dir", str(tmp_path / "X"), "--continue", bad])
    assert not os.path.exists(str(tmp_path / "X" / "CS_scenes_6.pth"))


def test_a_state_of_another_run_is_refused_by_name(case1, tmp_path):
    _, da, _, _ = case1
    st = os.path.join(da, "train_state_3.pth")
    with pytest.raises(ValueError, match="num_steps"):
        run(CASE1 + ["--num-steps", "7", "--snapshot-dir", str(tmp_path / "X"), "--continue", st])
    with pytest.raises(ValueError, match="optim"):
        run(common() + ["--optim", "adamw", "--prune-type", "dcfp", "--num-steps", "6", "--snapshot-dir",
                        str(tmp_path / "X"), "--continue", st])


# ------------------------------------------------------------------ case 2
def test_adamw_taylor_slimming_continues_bit_identically(cuda, tmp_path):
    da, _, _ = three_runs(tmp_path, common() + ["--optim", "adamw", "--learning-rate", "1e-3", "--prune-type", "taylor",
                                                "--slim-lambda", "1e-4"], 6, 3, 3)
    st = load(os.path.join(da, "train_state_6.pth"))
    assert set(st["digests"]) == {"flat_param", "exp_avg", "exp_avg_sq", "scorer"}
    assert st["scorer"]["steps"] == 6 and load(os.path.join(da, "score.pth"))["steps"] == 6


# ------------------------------------------------------------------ case 3: a dataset, the cut inside the second epoch
def write_cs(root, sizes, index=False):
    """A Cityscapes-shaped tree: PNG pairs under img/a and gt/a with blocky label maps of raw ids, the list file and -
    for the `resample` sampler - the class index next to it."""
    import _augment_ref as ref
    from PIL import Image
    rs = np.random.RandomState(9)
    raw_ids = sorted(ref.CS_TRAIN_IDS)
    table = ref.cs_id_table()
    os.makedirs(root / "img" / "a", exist_ok=True)
    os.makedirs(root / "gt" / "a", exist_ok=True)
    lines, idx = [], {str(c): [] for c in range(19)}
    for i, (h, w) in enumerate(sizes):
        coarse = rs.choice(np.array(raw_ids[:6] + [0, 3], dtype=np.uint8), size=(-(-h // 5), -(-w // 5)))
        ids = np.ascontiguousarray(np.kron(coarse, np.ones((5, 5), dtype=np.uint8))[:h, :w])
        if i == 0:
            ids[:2, :38] = np.repeat(np.array(raw_ids, dtype=np.uint8), 2)[None, :]
        Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(root / "img" / "a" / ("s%d_leftImg8bit.png" % i))
        Image.fromarray(ids).save(root / "gt" / "a" / ("s%d_gtFine_labelIds.png" % i))
        lines.append("img/a/s%d_leftImg8bit.png gt/a/s%d_gtFine_labelIds.png" % (i, i))
        for c in np.unique(table[ids]):
            if c < 19:
                idx[str(int(c))].append({"idx": i, "name": "s%d_gtFine_labelIds" % i})
    (root / "train.lst").write_text("\n".join(lines) + "\n")
    if index:
        idx["label_f"] = np.array([len(idx[str(c)]) for c in range(19)], dtype=np.float64)
        with open(root / "label_index_CS.pkl", "wb") as f:
            pickle.dump(idx, f)
    return {"root": str(root), "list_path": str(root / "train.lst")}


SIZES = [(80, 100), (70, 90), (90, 120), (66, 130), (75, 75), (88, 96)]


def test_gsrl_on_a_dataset_continues_inside_the_second_epoch(cuda, tmp_path):
    data = tmp_path / "data"
    os.makedirs(data)
    para = write_cs(data, SIZES)
    argv = common() + ["--loss-type", "gsrl", "--balance", "1", "--dataset", "CS", "--data-para", json.dumps(para),
                       "--random-scale", "--random-mirror", "--random-brightness", "--learning-rate", "1e-3"]
    da, _, _ = three_runs(tmp_path, argv, 7, 4, 1)               # 6 images in batches of 2: step 4 is batch 1 of epoch 1
    st = load(os.path.join(da, "train_state_4.pth"))
    assert st["ranks"][0]["data_kind"] == "loader"
    assert (st["ranks"][0]["data"]["epoch"], st["ranks"][0]["data"]["batch"]) == (1, 1)


@pytest.mark.parametrize("boundary", [False, True])
def test_resample_loader_state_continues_the_batches(cuda, tmp_path, boundary):
    """The `resample` path (per-sample child generators, the crop placed on the device's answer): a loader restored at
    batch k serves the batches of the one that never stopped - images, labels, weights and the placed pixels."""
    from dcfp_amd.datasets import TrainLoader, build_dataset
    para = write_cs(tmp_path, [(40, 60), (50, 70), (33, 47), (64, 64), (36, 90), (48, 48)], index=True)

    def make():
        ds = build_dataset("CS", split="train", crop_size=(16, 16), scale=True, mirror=True, brightness=True, balance=2,
                           data_para=dict(para, resample=True))
        return TrainLoader(ds, 19, cuda, seed=13, num_workers=2, rank=0, world_size=1)

    def endless(loader):
        while True:
            for batch in loader:
                yield batch, list(loader.last_pixels)

    whole = make()
    per_epoch = len(whole)
    assert 3 <= per_epoch <= 6
    k = per_epoch if boundary else 2
    total = per_epoch + 2
    it, want, state = endless(whole), [], None
    for b in range(total):
        if b == k:
            state = whole.state_dict()
        want.append(next(it))
    assert (state["epoch"], state["batch"]) == ((1, 0) if boundary else (0, 2))
    cont = make()
    cont.load_state_dict(state)
    it = endless(cont)
    for b in range(k, total):
        (images, labels), pixels = next(it)
        (wi, wl), wp = want[b]
        assert pixels == wp, b
        assert not differences({"i": images, "l": labels["ori"], "w": labels["weight"]},
                               {"i": wi, "l": wl["ori"], "w": wl["weight"]}), b
    assert differences(want[0][0][0], want[1][0][0])                            # the batches do differ from each other


# ------------------------------------------------------------------ case 4: the slim model
def test_slim_r101_continues_and_needs_its_channel_cfg(cuda, tmp_path):
    argv = common("resnet101") + ["--channel-cfg", SLIM_CFG, "--prune-type", "dcfp"]
    da, _, _ = three_runs(tmp_path, argv, 6, 3, 3)
    with pytest.raises(ValueError, match=r"parameter \S+\.weight differs"):
        run(common("resnet101") + ["--prune-type", "dcfp", "--num-steps", "6", "--snapshot-dir", str(tmp_path / "X"),
                                   "--continue", os.path.join(da, "train_state_3.pth")])


# ------------------------------------------------------------------ case 5: fresh processes
def test_continue_in_a_fresh_process(case1, tmp_path):
    """A and then B of case 1 as two child processes: each under its own time limit, the second only after the first
    exited 0.  Their files equal each other and those of the in-process run A."""
    _, da_inproc, _, la = case1
    da, db = str(tmp_path / "A"), str(tmp_path / "B")
    head = [sys.executable, os.path.join(ROOT, "tools", "train.py")] + CASE1 + \
        ["--num-steps", "6", "--state-every", "3", "--keep-states", "100"]
    ra = subprocess.run(head + ["--snapshot-dir", da], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert ra.returncode == 0, ra.stderr[-3000:]
    rb = subprocess.run(head + ["--snapshot-dir", db, "--continue", os.path.join(da, "train_state_3.pth")],
                        capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert rb.returncode == 0, rb.stderr[-3000:]
    assert "continued from" in rb.stdout and "restore" in rb.stdout and "save" in ra.stdout
    assert digest_lines(rb.stdout) == digest_lines(ra.stdout)[3:] and len(digest_lines(rb.stdout)) == 3
    same_run(da, db, 6, "continued at 3 in a fresh process")
    assert digest_lines(ra.stdout) == la
    same_run(da_inproc, da, 6, "CONTROL (a fresh process against this one; a determinism finding, not the feature)")


# ------------------------------------------------------------------ case 6: two ranks on one GPU
def _child(rank, world, mode, base):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dcfp_amd import train_state
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=PORT, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    train = importlib.import_module("train")
    out = os.path.join(base, mode, "rank%d" % rank)
    argv = common(batch=4) + ["--prune-type", "dcfp", "--snapshot-dir", out]
    if mode == "perturb":
        real = train_state.capture

        def capture(iteration, seg_model, optimizer, *a, **k):
            if rank == 1:                                    # one word of one rank's parameters, right before the save
                flat = optimizer.arena().flat_param
                flat[5] = flat[5] + 1.0
            return real(iteration, seg_model, optimizer, *a, **k)
        train_state.capture = capture
        try:
            train.main(argv + ["--num-steps", "1", "--state-every", "1"])
        except RuntimeError as e:
            print("REFUSED rank %d: %s" % (rank, e), flush=True)
        assert not [f for f in os.listdir(out) if f.startswith("train_state")] if os.path.isdir(out) else True
    else:
        argv += ["--num-steps", "6", "--state-every", "3", "--keep-states", "100"]
        if mode == "B":
            argv += ["--continue", os.path.join(base, "A", "rank0", "train_state_3.pth")]
        train.main(argv)
    dist.barrier()
    dist.destroy_process_group()


def _run_pair(mode, base):
    env = dict(os.environ)
    for k in ("DCFP_FORCE_SYNCBN", "DCFP_SYNCBN_P2P"):
        env.pop(k, None)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", str(r), "2", mode, base], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d:\n%s" % (r, logs[r][-3000:])
    return logs


def test_two_ranks_continue_bit_identically(cuda, tmp_path):
    base = str(tmp_path)
    la = _run_pair("A", base)                                    # (B starts only after both ranks of A exited 0)
    lb = _run_pair("B", base)
    da, db = os.path.join(base, "A", "rank0"), os.path.join(base, "B", "rank0")
    a0, a1, b0, b1 = (digest_lines(t) for t in (la[0], la[1], lb[0], lb[1]))
    assert len(a0) == 6 and a0 == a1                             # both ranks hold the same parameters at every step
    assert b0 == a0[3:] and b1 == b0
    same_run(da, db, 6, "two ranks continued at 3")
    st = load(os.path.join(da, "train_state_3.pth"))
    assert len(st["ranks"]) == 2 and st["fingerprint"]["world_size"] == 2
    assert not os.path.exists(os.path.join(base, "A", "rank1", "train_state_3.pth"))      # one file, written by rank 0


def test_ranks_that_differ_refuse_to_write(cuda, tmp_path):
    logs = _run_pair("perturb", str(tmp_path))
    for r, log in enumerate(logs):
        assert "REFUSED rank %d" % r in log and "do not hold the same bits" in log, log[-2000:]
        assert "digest of flat_param" in log and "on rank 1" in log, log[-2000:]
    for r in range(2):
        d = os.path.join(str(tmp_path), "perturb", "rank%d" % r)
        assert not [f for f in os.listdir(d) if f.startswith("train_state")]


if __name__ == "__main__" and "--child" in sys.argv:
    i = sys.argv.index("--child")
    _child(int(sys.argv[i + 1]), int(sys.argv[i + 2]), sys.argv[i + 3], sys.argv[i + 4])
