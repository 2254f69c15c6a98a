"""The baseline pruning criteria the DCFP tables are compared against, through the same score file and ChannelPruner.

One fp32 score per output channel of every scored BatchNorm layer (the set `dcfp_pruning` scores: BatchNorm2d /
SyncBatchNorm whose name is not in `model.ignore_prune_layer`); larger means keep.  W [C, Cin, kh, kw] is the weight of
the conv that `build_graph(model).norm_conv_links` links to the BN, K = Cin*kh*kw, gamma / beta the BN weight and bias,
g. the gradients as they stand where `dcfp_pruning.step` runs (after backward and the data-parallel all-reduce):

    taylor     mean over the steps of (gamma_c ggamma_c + beta_c gbeta_c)^2     Molchanov et al. 2019, on the BN gate
    taylor_w   mean over the steps of (sum_k W_ck gW_ck)^2                      the same paper, on the filter
    slimming   |gamma_c|                                                        Liu et al. 2017
    l1, l2     sum_k |W_ck|,  sqrt(sum_k W_ck^2)                                Li et al. 2017
    fpgm       sum_j sqrt(sum_k (W_ck - W_jk)^2)                                He et al. 2019

`taylor_pruning` is the online scorer (one HIP launch per step over a device-resident pointer table, like `dcfp_pruning`),
`slimming_regularizer` the L1 term of Network Slimming on the gamma gradients, `weight_scores` the criteria read off the
weights (one `dcfp_filter_reduce_f32` launch, or the two of `dcfp_fpgm_f32`, for the whole model).  All of them write
score.pth = {"eic": {bn: FloatTensor[C]}, "criterion": name[, "steps": n]}, which `DCFPPruner` loads as it is (it reads
"eic" alone).  Norms and distances of layers with different K are not comparable and `DCFPPruner` thresholds globally
per group: `normalize_scores` / `ScorePruner(score_norm=...)` rescale per layer first.  csrc/score.hip, DESIGN §17."""
import ctypes as C

import torch
import torch.nn as nn

from .. import _lib
from .._lib import FilterEntry, FpgmEntry, GateEntry, check
from .channel_pruner import build_graph
from .dcfp_pruner import DCFPPruner, adopt_scores

WEIGHT_CRITERIA = ("slimming", "l1", "l2", "fpgm")
TAYLOR_MODES = {"gate": "taylor", "weight": "taylor_w"}
SCORE_NORMS = ("none", "l2", "mean")


def scored_bn_names(model):
    """Names of the BatchNorm layers `dcfp_pruning` scores, in module order."""
    return [name for name, m in model.named_modules()
            if isinstance(m, (nn.BatchNorm2d, nn.SyncBatchNorm)) and name not in model.ignore_prune_layer]


def linked_convs(model, names):
    """{bn name: name of the conv feeding it} for `names`, from the static graph the pruner cuts by."""
    links = build_graph(model).norm_conv_links
    missing = [n for n in names if n not in links]
    if missing:
        raise RuntimeError(f"no conv is linked to the scored BatchNorm layers {missing[:3]} (channel_pruner.build_graph)")
    return {n: links[n] for n in names}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _upload(entries, dev):
    return torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8).to(dev)


def _kernel_tensor(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError(f"{what}: the HIP kernels take contiguous fp32 tensors on the device")
    return t


def filter_reduce_table(items):
    """Device table of a `filter_reduce` launch over `items` = [(w, g or None, out)]: w (and g) `rows` rows of K
    contiguous floats with rows = out.numel(), any 4-byte aligned views.  Returns (table, n entries, units)."""
    L = _lib.lib()
    entries = (FilterEntry * max(1, len(items)))()
    unit = 0
    for e, (w, g, out) in zip(entries, items):
        _kernel_tensor(w, "filter_reduce w"), _kernel_tensor(out, "filter_reduce out")
        rows = out.numel()
        if rows < 1 or w.numel() < rows or w.numel() % rows:
            raise ValueError(f"filter_reduce: {w.numel()} weights are not {rows} rows")
        if g is not None and _kernel_tensor(g, "filter_reduce g").numel() != w.numel():
            raise ValueError("filter_reduce: g has another size than w")
        e.w, e.g, e.out = w.data_ptr(), (g.data_ptr() if g is not None else None), out.data_ptr()
        e.rows, e.K, e.first_unit = rows, w.numel() // rows, unit
        unit += L.dcfp_filter_reduce_units(e.rows, e.K)
    if not items:
        return None, 0, 0
    return _upload(entries, items[0][0].device), len(items), unit


def filter_reduce(table, n, units, op):
    """One launch of dcfp_filter_reduce_f32 over a table of `filter_reduce_table`; op = _lib.FILTER_*."""
    check(_lib.lib().dcfp_filter_reduce_f32(C.c_void_p(table.data_ptr() if table is not None else None), n, units, op,
                                            _stream()), "filter_reduce")


def fpgm_table(items):
    """Device table and workspace of an `fpgm` call over `items` = [(w [C, K...], out [C])].
    Returns (table, n entries, tiles, workspace)."""
    if not items:
        return None, 0, 0, None
    L = _lib.lib()
    entries = (FpgmEntry * len(items))()
    tile, ws_off = 0, 0
    for e, (w, out) in zip(entries, items):
        _kernel_tensor(w, "fpgm w"), _kernel_tensor(out, "fpgm out")
        rows = out.numel()
        if rows < 1 or w.numel() < rows or w.numel() % rows:
            raise ValueError(f"fpgm: {w.numel()} weights are not {rows} rows")
        e.w, e.out, e.C, e.K, e.first_tile, e.ws_off = w.data_ptr(), out.data_ptr(), rows, w.numel() // rows, tile, ws_off
        nt = (rows + _lib.FPGM_TILE - 1) // _lib.FPGM_TILE
        tile += nt * nt
        ws_off += L.dcfp_fpgm_workspace_bytes(rows) // 4
    dev = items[0][0].device
    return _upload(entries, dev), len(items), tile, torch.empty(ws_off, dtype=torch.float32, device=dev)


def fpgm(table, n, tiles, ws):
    """The two launches of dcfp_fpgm_f32 over a table of `fpgm_table`: out[i] = sum_j ||w_i - w_j||_2 per matrix."""
    check(_lib.lib().dcfp_fpgm_f32(C.c_void_p(table.data_ptr() if table is not None else None), n, tiles,
                                   C.c_void_p(ws.data_ptr() if ws is not None else None),
                                   ws.numel() * 4 if ws is not None else 0, _stream()), "fpgm")


class _GateTable:
    """What the per-step scorers share with `dcfp_pruning`: a name list fixed at construction, a device table built
    from data_ptrs and rebuilt when they change."""

    def __init__(self, model):
        self._names = scored_bn_names(model)
        self._key = None
        self._table = None

    def _modules(self, model, who, need_bias_grad):
        mods_by_name = dict(model.named_modules())
        mods = [mods_by_name[n] for n in self._names]
        for n, m in zip(self._names, mods):
            if not m.weight.is_cuda:
                raise RuntimeError(f"{who} runs on the HIP kernel: model must be on cuda")
            if m.weight.grad is None or (need_bias_grad and m.bias.grad is None):
                raise RuntimeError(f"{who}: {n} has no gradient (call after backward)")
        return mods


class taylor_pruning(_GateTable):
    """First-order Taylor importance accumulated over training steps; the life cycle of `dcfp_pruning`:
    `step(model)` after backward (and the gradient all-reduce), `export_eic(path)` at the end.
    mode "gate": (gamma ggamma + beta gbeta)^2 per BN channel; "weight": (sum_k W gW)^2 per filter of the linked conv.
    state_dict["eic"][bn] is the running SUM (a view into one arena); the exported score is sum / steps."""

    def __init__(self, model, mode="gate", **kwards):
        if mode not in TAYLOR_MODES:
            raise ValueError(f"taylor_pruning: mode {mode!r} is not one of {sorted(TAYLOR_MODES)}")
        super().__init__(model)
        self.mode, self.criterion, self.steps = mode, TAYLOR_MODES[mode], 0
        mods = dict(model.named_modules())
        self._channels = {n: mods[n].weight.numel() for n in self._names}
        self._convs = linked_convs(model, self._names) if mode == "weight" else {}
        self.state_dict = {"eic": {n: 0 for n in self._names}}

    def _arena_views(self, dev):
        old = self.state_dict["eic"]
        arena = torch.zeros(sum(self._channels.values()), dtype=torch.float32, device=dev)
        off = 0
        for name in self._names:
            view = arena[off:off + self._channels[name]]
            if isinstance(old.get(name), torch.Tensor):
                view.copy_(old[name].to(dev))
            old[name] = view
            off += self._channels[name]
        self._arena = arena
        return old

    def step(self, model):
        if not self._names:
            return
        mods = self._modules(model, "taylor_pruning.step", self.mode == "gate")
        L = _lib.lib()
        if self.mode == "gate":
            key = tuple((m.weight.data_ptr(), m.bias.data_ptr(), m.weight.grad.data_ptr(), m.bias.grad.data_ptr())
                        for m in mods)
            if key != self._key:
                views = self._arena_views(mods[0].weight.device)
                entries = (GateEntry * len(mods))()
                for e, name, k in zip(entries, self._names, key):
                    e.gamma, e.beta, e.ggrad, e.bgrad = k
                    e.score, e.n = views[name].data_ptr(), self._channels[name]
                self._table, self._key = _upload(entries, mods[0].weight.device), key
            check(L.dcfp_gate_taylor_f32(C.c_void_p(self._table.data_ptr()), len(mods), _stream()), "gate_taylor")
        else:
            by_name = dict(model.named_modules())
            convs = [by_name[self._convs[n]] for n in self._names]
            for n, c in zip(self._names, convs):
                if c.weight.grad is None:
                    raise RuntimeError(f"taylor_pruning.step: {self._convs[n]}.weight.grad is None (call after backward)")
            key = tuple((c.weight.data_ptr(), c.weight.grad.data_ptr()) for c in convs)
            if key != self._key:
                views = self._arena_views(convs[0].weight.device)
                items = [(c.weight.detach(), c.weight.grad, views[n]) for n, c in zip(self._names, convs)]
                self._table, self._key = filter_reduce_table(items), key
            filter_reduce(*self._table, _lib.FILTER_DOT_SQ_ACC)
        self.steps += 1

    def get_eic(self):
        return self.state_dict

    def get_state(self):
        """What a continued run needs of this scorer (train_state): the running sums and the step count
        `scores()` divides them by."""
        return {"eic": dict(self.state_dict["eic"]), "steps": int(self.steps), "criterion": self.criterion}

    def set_state(self, state, device=None):
        """Take back what get_state() gave - the twin of dcfp_pruning.set_eic: the sums become views into one fresh
        arena (on `device` if given), which the next step() copies into the arena its table points at."""
        if state.get("criterion", self.criterion) != self.criterion:
            raise ValueError("taylor_pruning.set_state: the state is of criterion %r, this scorer of %r"
                             % (state.get("criterion"), self.criterion))
        for n, v in state["eic"].items():
            if isinstance(v, torch.Tensor) and n in self._channels and v.numel() != self._channels[n]:
                raise ValueError("taylor_pruning.set_state: %s has %d channels, the state %d"
                                 % (n, self._channels[n], v.numel()))
        self.state_dict["eic"] = adopt_scores(state["eic"], self._names, device, "taylor_pruning.set_state", self)
        self.steps = int(state["steps"])
        self._key = None

    def scores(self):
        """{bn: FloatTensor[C]} on the CPU: the running sums over the steps run, divided by their number."""
        out = {}
        for name in self._names:
            v = self.state_dict["eic"][name]
            out[name] = (v.detach().cpu() / self.steps) if isinstance(v, torch.Tensor) \
                else torch.zeros(self._channels[name])
        return out

    def export_eic(self, path):
        torch.save({"eic": self.scores(), "criterion": self.criterion, "steps": self.steps}, path)


class slimming_regularizer(_GateTable):
    """The sparsity term of Network Slimming: `step(model)` after backward, before optimizer.step(), adds
    lam * sign(gamma) (sign(0) = 0) to the gamma gradient of every scored BatchNorm layer, in one launch."""

    def __init__(self, model, lam):
        super().__init__(model)
        self.lam = float(lam)

    def step(self, model):
        if not self._names:
            return
        mods = self._modules(model, "slimming_regularizer.step", False)
        key = tuple((m.weight.data_ptr(), m.weight.grad.data_ptr()) for m in mods)
        if key != self._key:
            entries = (GateEntry * len(mods))()
            for e, m, k in zip(entries, mods, key):
                e.gamma, e.ggrad = k
                e.n = m.weight.numel()
            self._table, self._key = _upload(entries, mods[0].weight.device), key
        check(_lib.lib().dcfp_gate_l1reg_f32(C.c_void_p(self._table.data_ptr()), len(mods), self.lam, _stream()),
              "gate_l1reg")


def weight_scores(model, criterion, timing=None):
    """{bn: FloatTensor[C]} on the model's device for `criterion` in WEIGHT_CRITERIA, keyed like
    dcfp_pruning(model).state_dict["eic"].  l1 / l2: one filter_reduce launch over all linked convs; fpgm: its two
    launches; slimming is |gamma| and needs no kernel.  `timing` (a dict) receives "ms": the device time of the
    scoring launches by events (table upload and allocation excluded)."""
    if criterion not in WEIGHT_CRITERIA:
        raise ValueError(f"weight_scores: criterion {criterion!r} is not one of {WEIGHT_CRITERIA}")
    names = scored_bn_names(model)
    mods = dict(model.named_modules())
    if any(not mods[n].weight.is_cuda for n in names):
        raise RuntimeError("weight_scores runs on the HIP kernels: model must be on cuda")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timing is not None else None
    if criterion == "slimming":
        if ev:
            ev[0].record()
        out = {n: mods[n].weight.detach().abs() for n in names}
    else:
        convs = linked_convs(model, names)
        weights = {n: mods[convs[n]].weight.detach().contiguous() for n in names}
        for n in names:
            if weights[n].shape[0] != mods[n].weight.numel():
                raise RuntimeError(f"{convs[n]} has {weights[n].shape[0]} filters, {n} {mods[n].weight.numel()} channels")
        dev = mods[names[0]].weight.device if names else None
        arena = torch.zeros(sum(mods[n].weight.numel() for n in names), dtype=torch.float32, device=dev)
        out, off = {}, 0
        for n in names:
            out[n] = arena[off:off + mods[n].weight.numel()]
            off += mods[n].weight.numel()
        if criterion == "fpgm":
            plan = fpgm_table([(weights[n], out[n]) for n in names])
            if ev:
                ev[0].record()
            fpgm(*plan)
        else:
            table = filter_reduce_table([(weights[n], None, out[n]) for n in names])
            if ev:
                ev[0].record()
            filter_reduce(*table, _lib.FILTER_ABS_SUM if criterion == "l1" else _lib.FILTER_L2)
    if ev:
        ev[1].record()
        ev[1].synchronize()
        timing["ms"] = ev[0].elapsed_time(ev[1])
    return out


def export_scores(path, scores, criterion):
    """score.pth of a weight criterion, in the format `dcfp_pruning.export_eic` writes plus the criterion's name."""
    torch.save({"eic": {k: v.detach().float().cpu().clone() for k, v in scores.items()}, "criterion": criterion}, path)


def normalize_scores(eic, mode):
    """Per-layer rescaling of {bn: score[C]} on the host, fp64 inside, fp32 out: "none" leaves the scores as they are,
    "l2" is s / ||s||_2, "mean" is s / mean(s); a layer of zeros stays zeros."""
    if mode not in SCORE_NORMS:
        raise ValueError(f"normalize_scores: mode {mode!r} is not one of {SCORE_NORMS}")
    if mode == "none":
        return dict(eic)
    out = {}
    for name, s in eic.items():
        d = torch.as_tensor(s).detach().cpu().double()
        scale = d.norm() if mode == "l2" else d.mean()
        out[name] = (d / scale if float(scale) != 0.0 else torch.zeros_like(d)).float()
    return out


class ScorePruner(DCFPPruner):
    """DCFPPruner on per-layer normalised scores: the same two-group thresholds and masks, on
    normalize_scores(score file, score_norm)."""

    def __init__(self, global_percent=0.8, layer_keep=0.01, except_start_keys=["head.fc"], score_file="",
                 score_norm="none", **kwards):
        super().__init__(global_percent=global_percent, layer_keep=layer_keep, except_start_keys=except_start_keys,
                         score_file=score_file, **kwards)
        self.score_norm = score_norm
        self.eic = normalize_scores(self.eic, score_norm)
