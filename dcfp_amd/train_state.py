"""Resumable training: everything a step reads or writes, in one file.

tools/train.py `--state-every N` writes `train_state_<k>.pth` after step k; `-c/--continue FILE` restores it and runs the
steps k .. num_steps-1.  The contract: the continued run leaves the bits of the run that was never stopped - weights,
BatchNorm buffers, optimizer state and score.pth.  The step is bit-reproducible (no float atomics, fixed reduction
orders), so the contract holds as soon as nothing a step reads is lost.  The file is a plain dict written by
rank 0 with torch.save, `"format": 1`:

    iteration    completed steps
    model        seg_model.state_dict() (the buffers of a criterion that is a child module come along)
    optimizer    optimizer.state_dict() of FusedSGD / FusedAdamW
    scorer       dcfp_pruning: {"eic": {bn: vector}}; taylor_pruning: its get_state() (sums and step count); else None
    ranks        one entry per rank: torch's CPU generator, the rank's device generator (the Dropout2d mask of
                 conv_deepsup is drawn on it), and the synthetic dataset's generator or the TrainLoader's state_dict()
    fingerprint  what must match for a continuation to mean anything (`fingerprint`)
    digests      {buffer: (d0, d1)} of ops.state_digest over the parameter arena, every optimizer-state arena and the
                 scorer's arena, taken on the device before the copy to the host

Not state: the learning rate (a function of `iteration`), the teacher (rebuilt from its own arguments), the permuted
weight copies and kept Winograd filters (rebuilt from the weights), slimming_regularizer (stateless).

All tensors of the file are on the CPU.  Restoring goes in two moves, because the weights must be in the model before it
is moved to the device and adopted by the optimizer's arena (the place `--resume` loads them): `restore_model`, then -
once optimizer, scorer and data source exist - `restore_rest`, which ends by recomputing the digests on the device and
refuses if one differs (state copied into a wrong arena slot)."""
import glob
import os
import re
import time

import torch
import torch.distributed as dist

FORMAT = 1
KEYS = ("format", "iteration", "model", "optimizer", "scorer", "ranks", "fingerprint", "digests")

# fingerprint field -> attribute of the driver's argparse namespace
ARG_FIELDS = (
    ("model", "model"), ("backbone", "backbone"), ("backbone_para", "backbone_para"), ("model_para", "model_para"),
    ("align_corner", "align_corner"), ("deepsup", "deepsup"),
    ("optim", "optim"), ("momentum", "momentum"), ("betas", "betas"), ("weight_decay", "weight_decay"),
    ("no_decay", "no_decay"), ("num_steps", "num_steps"), ("power", "power"), ("warmup", "warmup"),
    ("learning_rate", "learning_rate"), ("batch_size", "batch_size"), ("loss_type", "loss_type"),
    ("loss_para", "loss_para"), ("prune_type", "prune_type"), ("slim_lambda", "slim_lambda"), ("dataset", "dataset"),
    ("data_dir", "data_dir"), ("data_para", "data_para"), ("random_scale", "random_scale"),
    ("random_mirror", "random_mirror"), ("random_brightness", "random_brightness"), ("balance", "balance"),
    ("longsize", "longsize"), ("shortsize", "shortsize"), ("ignore_label", "ignore_label"),
    ("input_size", "input_size"), ("random_seed", "random_seed"),
    ("clip_grad_norm", "clip_grad_norm"), ("ema_decay", "ema_decay"),
)
# fields younger than the format: a state file written before they existed was written without them, which is what
# None says - such a file continues in a run that sets neither, and is refused by name in a run that sets one
ABSENT_IS_NONE = ("clip_grad_norm", "ema_decay")


def fingerprint(args, seg_model, num_classes, world_size):
    """What a state file is a state OF: the model and every parameter's name and shape (a wrong --channel-cfg shows up by
    name), the optimizer and schedule, the batch, the world size, the loss, the scorer, the data and its seed."""
    fp = {"num_classes": int(num_classes), "world_size": int(world_size)}
    for field, attr in ARG_FIELDS:
        fp[field] = getattr(args, attr, None)
    fp["params"] = [[name, list(p.shape)] for name, p in seg_model.named_parameters()]
    return fp


def check_fingerprint(saved, current):
    """ValueError naming the first field in which the state file and this run differ, with both values."""
    for field in list(saved) + [f for f in current if f not in saved]:
        if field == "params":
            continue
        absent = None if field in ABSENT_IS_NONE else "<absent>"
        a, b = saved.get(field, absent), current.get(field, absent)
        if a != b:
            raise ValueError("cannot continue: %s differs - the state file has %r, this run %r" % (field, a, b))
    sp, cp = saved.get("params", []), current.get("params", [])
    have = {n: s for n, s in cp}
    for name, shape in sp:
        if name not in have:
            raise ValueError("cannot continue: parameter %s %r of the state file does not exist in this run's model"
                             % (name, list(shape)))
        if list(have[name]) != list(shape):
            raise ValueError("cannot continue: parameter %s differs - the state file has shape %r, this run %r"
                             % (name, list(shape), list(have[name])))
    there = {n for n, _ in sp}
    for name, shape in cp:
        if name not in there:
            raise ValueError("cannot continue: parameter %s %r of this run's model is not in the state file"
                             % (name, list(shape)))
    if [n for n, _ in sp] != [n for n, _ in cp]:
        raise ValueError("cannot continue: params differ - the same parameters in another order")


def _cpu(obj):
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: _cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_cpu(v) for v in obj)
    return obj


def digest_buffers(optimizer, scorer):
    """{name: flat device buffer} of everything the digests cover: the parameter arena, each optimizer-state arena
    (momentum; exp_avg, exp_avg_sq) and the scorer's arena once it exists."""
    out = {}
    arena = optimizer.arena() if hasattr(optimizer, "arena") else None
    if arena is not None:
        out["flat_param"] = arena.flat_param
        for name in sorted(arena.state_buffers):
            out[name] = arena.state_buffers[name]
    sc = getattr(scorer, "_arena", None) if scorer is not None else None
    if isinstance(sc, torch.Tensor) and sc.is_cuda:
        out["scorer"] = sc
    return out


def digests(optimizer, scorer):
    """{name: (d0, d1)} of `digest_buffers`: the launches first, one read at the end."""
    from . import ops
    bufs = digest_buffers(optimizer, scorer)
    dev = {name: ops.state_digest_device(b) for name, b in bufs.items()}
    return {name: tuple(int(v) & 0xFFFFFFFFFFFFFFFF for v in d.tolist()) for name, d in dev.items()}


def check_ranks(mine, group=None):
    """Every rank holds the same bits, or nobody writes: all ranks gather the digests and all of them raise a RuntimeError
    naming the first buffer that differs and the ranks that hold another value than rank 0."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    every = [None] * dist.get_world_size(group)
    dist.all_gather_object(every, mine, group=group)
    names = list(every[0])
    for d in every[1:]:
        names += [n for n in d if n not in names]
    for name in names:
        odd = [r for r, d in enumerate(every) if d.get(name) != every[0].get(name)]
        if odd:
            def show(d):
                v = d.get(name)
                return "absent" if v is None else "%016x:%016x" % tuple(v)
            raise RuntimeError("train_state: the ranks do not hold the same bits - digest of %s is %s on rank 0 but %s; "
                               "no state file is written" % (name, show(every[0]),
                                                           ", ".join("%s on rank %d" % (show(every[r]), r) for r in odd)))


def scorer_state(scorer):
    if scorer is None:
        return None
    if hasattr(scorer, "get_state"):
        return scorer.get_state()
    return {"eic": dict(scorer.get_eic()["eic"])}


def rank_state(device, source):
    """This rank's generators and its data position.  source: an object with .gen (the synthetic dataset) or with
    state_dict() (TrainLoader)."""
    entry = {"torch_cpu": torch.get_rng_state(), "cuda": None, "data_kind": None, "data": None}
    if device is not None and torch.device(device).type == "cuda":
        entry["cuda"] = torch.cuda.get_rng_state(device)
    if source is not None:
        if hasattr(source, "state_dict"):
            entry["data_kind"], entry["data"] = "loader", source.state_dict()
        else:
            entry["data_kind"], entry["data"] = "generator", source.gen.get_state()
    return entry


def capture(iteration, seg_model, optimizer, scorer, device, source, fp, group=None):
    """The state after `iteration` completed steps, on the host.  Collective: every rank calls it; the digests are
    compared across the ranks before anything is copied (check_ranks)."""
    dg = digests(optimizer, scorer)
    check_ranks(dg, group)
    mine = rank_state(device, source)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        ranks = [None] * dist.get_world_size(group)
        dist.all_gather_object(ranks, mine, group=group)
    else:
        ranks = [mine]
    return {"format": FORMAT, "iteration": int(iteration), "model": _cpu(seg_model.state_dict()),
            "optimizer": _cpu(optimizer.state_dict()), "scorer": _cpu(scorer_state(scorer)), "ranks": ranks,
            "fingerprint": fp, "digests": dg}


def save(state, path):
    """Write to a temporary name in the same directory, then os.replace: a save that dies midway leaves the previous
    file, and never a partial one under the final name."""
    tmp = "%s.tmp.%d" % (path, os.getpid())
    try:
        with open(tmp, "wb") as f:
            torch.save(state, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise
    return path


def load(path):
    """The dict of a state file; RuntimeError on a file that is truncated, is no state file or has a format this code
    does not know."""
    try:
        state = torch.load(path, map_location="cpu", weights_only=False)
    except Exception as e:
        raise RuntimeError("train_state: %s cannot be read (%s: %s) - truncated, or not a state file"
                           % (path, type(e).__name__, e)) from e
    if not isinstance(state, dict) or "format" not in state:
        raise RuntimeError("train_state: %s is not a state file (a checkpoint of weights goes to --resume)" % path)
    if state["format"] != FORMAT:
        raise RuntimeError("train_state: %s has format %r, this code reads format %d" % (path, state["format"], FORMAT))
    missing = [k for k in KEYS if k not in state]
    if missing:
        raise RuntimeError("train_state: %s lacks %s" % (path, ", ".join(missing)))
    return state


def restore_model(state, seg_model, fp):
    """First move, on the CPU model before it goes to the device: refuse a state of another run (ValueError naming the
    field), then load the weights and buffers.  Returns the number of completed steps."""
    check_fingerprint(state["fingerprint"], fp)
    seg_model.load_state_dict(state["model"], strict=True)
    return int(state["iteration"])


def restore_rest(state, optimizer, scorer, device, source, rank=0):
    """Second move, with the model on the device and the optimizer built: optimizer state into its arenas, the scorer,
    this rank's generators and data position; then the digests again, on the device."""
    optimizer.load_state_dict(state["optimizer"])
    if hasattr(optimizer, "arena"):
        optimizer.arena()                     # adopt the loaded state tensors into the arenas now, not at the first step
    if (scorer is None) != (state["scorer"] is None):
        raise ValueError("cannot continue: the state file %s a scorer, this run %s"
                         % (("has", "has none") if scorer is None else ("has no", "has one")))
    if scorer is not None:
        if hasattr(scorer, "set_state"):
            scorer.set_state(state["scorer"], device=device)
        else:
            scorer.set_eic(state["scorer"], device=device)
    ranks = state["ranks"]
    if not 0 <= rank < len(ranks):
        raise ValueError("cannot continue: the state file holds %d ranks, this is rank %d" % (len(ranks), rank))
    mine = ranks[rank]
    torch.set_rng_state(mine["torch_cpu"])
    if mine["cuda"] is not None:
        torch.cuda.set_rng_state(mine["cuda"], device)
    if source is not None:
        kind = "loader" if hasattr(source, "load_state_dict") else "generator"
        if mine["data_kind"] != kind:
            raise ValueError("cannot continue: the state file's data position is a %s's, this run reads from a %s"
                             % (mine["data_kind"], kind))
        if kind == "loader":
            source.load_state_dict(mine["data"])
        else:
            source.gen.set_state(mine["data"])
    verify(state["digests"], optimizer, scorer)


def verify(saved, optimizer, scorer):
    """RuntimeError naming the first buffer whose digest on the device is not the one in the state file."""
    now = digests(optimizer, scorer)
    for name, want in saved.items():
        got = now.get(name)
        if got is None or tuple(got) != tuple(want):
            raise RuntimeError("train_state: after the restore the %s buffer does not hold the bits that were saved - digest "
                               "%016x:%016x in the state file, %s on the device"
                               % (name, want[0], want[1], "no such buffer" if got is None else "%016x:%016x" % tuple(got)))
    for name in now:
        if name not in saved:
            raise RuntimeError("train_state: the %s buffer of this run has no digest in the state file" % name)


def state_path(directory, iteration):
    return os.path.join(directory, "train_state_%d.pth" % iteration)


def prune_old(directory, keep):
    """Delete all but the `keep` newest train_state_<k>.pth of `directory` (after a successful write)."""
    found = []
    for p in glob.glob(os.path.join(directory, "train_state_*.pth")):
        m = re.fullmatch(r"train_state_(\d+)\.pth", os.path.basename(p))
        if m:
            found.append((int(m.group(1)), p))
    found.sort()
    gone = found[:-keep] if keep > 0 else []
    for _, p in gone:
        os.remove(p)
    return [p for _, p in gone]


def format_digest(d):
    return "%016x:%016x" % (d[0], d[1])


class Timer:
    def __enter__(self):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.seconds = time.perf_counter() - self.t0
        return False
