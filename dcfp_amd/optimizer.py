"""Optimizer construction and LR schedule — API of optimizer.py:12-79.

`build_optimizer` returns FusedSGD: the torch.optim.SGD(momentum, weight_decay) update of the
reference (optimizer.py:24-25) executed as ONE multi-tensor HIP launch per step over a
device-resident pointer table (the reference issues four foreach launches over ~470 tensors),
or for `--optim adamw` FusedAdamW: torch.optim.AdamW (optimizer.py:26-31) on the same machinery.
param_groups / lr / weight_decay keep torch.optim semantics, so adjust_learning_rate works
unchanged."""
import ctypes as C

import numpy as np
import torch
from torch.optim.adamw import adamw as _torch_adamw

from . import _lib
from ._lib import AdamEntry, SgdEntry, SGD_CHUNK, check
from .arena import ParamArena


def check_keywords_in_name(name, keywords=()):
    return any(k in name for k in keywords)


def set_weight_decay(model, skip_list=(), skip_keywords=()):
    has_decay, no_decay = [], []
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        if (name in skip_list) or check_keywords_in_name(name, skip_keywords):
            no_decay.append(param)
        else:
            has_decay.append(param)
    if len(no_decay) > 0:
        print("**** some para wo decay ****")
    return [{"params": has_decay}, {"params": no_decay, "weight_decay": 0.0}]


class _ArenaOptimizer(torch.optim.Optimizer):
    """What FusedSGD and FusedAdamW share: the parameters adopted into a ParamArena, per-parameter state kept as views
    into the arena's named state buffers (`_ARENA_STATE`: state key -> buffer name), `zero_grad` through the arena and
    the cache of device pointer tables (`table_rebuilds` counts uploads)."""
    _ARENA_STATE = {}

    def _init_arena(self):
        self._drop_tables()
        self._arena = None
        self.table_rebuilds = 0

    def _drop_tables(self):
        self._tables = {}

    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"] if p.requires_grad]

    def _adopted(self, p, state):
        """Called for every parameter whose state views were just (re)bound to an arena."""

    def arena(self):
        """The arena holding this optimizer's parameters, created on first use once they are on the GPU
        (the reference builds the optimizer before `seg_model.to(device)`, train.py:212-219)."""
        params = self._all_params()
        if not params or not all(p.is_cuda and p.dtype == torch.float32 for p in params):
            return None
        if self._arena is None or not self._arena.covers(params):
            self._arena = ar = ParamArena.of(params)
            self._drop_tables()
            # an arena found again (load_state_dict) holds the old state
            reused = {key: ar.has_state(name) for key, name in self._ARENA_STATE.items()}
            for i, p in enumerate(ar.params):               # state restored before the arena existed
                state = self.state[p]
                for key, name in self._ARENA_STATE.items():
                    old = state.get(key)
                    view = ar.state_view(name, i)
                    if old is None:
                        if reused[key]:  # no loaded state for this parameter: it starts from zero, as torch.optim's would
                            view.zero_()
                    elif old.data_ptr() != view.data_ptr():
                        view.copy_(old)
                    state[key] = view
                self._adopted(p, state)
        return self._arena

    def zero_grad(self, set_to_none: bool = True):
        """Same contract as torch.optim.Optimizer.zero_grad.  With the arena: set_to_none detaches the gradient
        views (no launch; the next backward's first write overwrites), the in-place flavour (torch 1.10's
        default, train.py:256) is ONE fill of the flat gradient buffer."""
        ar = self.arena()
        if ar is not None:
            return ar.zero_grad(set_to_none)
        return super().zero_grad(set_to_none=set_to_none)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._drop_tables()
        self._arena = None          # state tensors were replaced: re-adopt them into the arena on next use
        from . import ops
        ops.WEIGHT_EPOCH[0] += 1

    @staticmethod
    def _weights_changed():
        from . import ops
        ops.WEIGHT_EPOCH[0] += 1
        ops.refresh_wp()          # one launch: the permuted copies the conv kernels read, for the new weights


class FusedSGD(_ArenaOptimizer):
    """SGD with momentum and weight decay (dampening 0, no nesterov):
       g' = g + wd*p ; buf = momentum*buf + g' (buf starts at 0, which makes the first step buf = g' exactly,
       torch's clone) ; p -= lr*buf.

    Parameters, gradients and momentum buffers live in three flat arenas (dcfp_amd/arena.py): addresses are
    stable, so the device pointer table of a param group is built and uploaded ONCE (`table_rebuilds`
    counts uploads) and a step is one kernel launch per non-empty group; `zero_grad()` launches nothing."""
    _ARENA_STATE = {"momentum_buffer": "momentum"}

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self._init_arena()

    def _table(self, gi, group, params):
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["momentum_buffer"].data_ptr()) for p in params) \
            + (group["weight_decay"],)
        cached = self._tables.get(gi)
        if cached is not None and cached[0] == key:
            return cached[1], cached[2], cached[3]
        self.table_rebuilds += 1
        entries = (SgdEntry * len(params))()
        chunk = 0
        for i, p in enumerate(params):
            e = entries[i]
            e.param, e.grad, e.momentum_buf = p.data_ptr(), p.grad.data_ptr(), self.state[p]["momentum_buffer"].data_ptr()
            e.n, e.first_chunk, e.weight_decay = p.numel(), chunk, group["weight_decay"]
            chunk += (p.numel() + SGD_CHUNK - 1) // SGD_CHUNK
        host = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8)
        dev = host.to(params[0].device)
        self._tables[gi] = (key, dev, len(params), chunk)
        return dev, len(params), chunk

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.lib()
        self.arena()
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            for p in params:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() \
                        or not p.grad.is_contiguous():
                    raise RuntimeError("FusedSGD: parameters and grads must be contiguous CUDA fp32")
                if "momentum_buffer" not in self.state[p]:     # parameter outside the arena
                    self.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            table, n, chunks = self._table(gi, group, params)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            check(L.dcfp_sgd_momentum_f32(C.c_void_p(table.data_ptr()), n, chunks, float(group["lr"]),
                                          float(group["momentum"]), 0, stream), "sgd_momentum")
        self._weights_changed()
        return loss


def _kernel_ready(p):
    g = p.grad
    return p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() \
        and g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and not g.is_sparse


class FusedAdamW(_ArenaOptimizer):
    """torch.optim.AdamW (decoupled weight decay; no amsgrad, maximize or capturable), the reference's `--optim adamw`
    (optimizer.py:26-31):
       p *= 1 - lr*wd ; m = lerp(m, g, 1-beta1) ; v = beta2*v + (1-beta2)*g*g ;
       p -= lr/(1-beta1^t) * m / (sqrt(v)/sqrt(1-beta2^t) + eps),   t = the parameter's own step count.

    Parameters, gradients, exp_avg and exp_avg_sq live in four flat arenas (dcfp_amd/arena.py).  A step partitions the
    parameters of a group that have a gradient by their step count and issues ONE launch of dcfp_adamw_f32 per
    partition (the bias corrections belong to the count): one launch per non-empty group once every parameter has had
    its first gradient.  Learning rate, weight decay and the bias corrections are kernel arguments, so the pointer
    tables - cached per group and partition, keyed on the data pointers - are uploaded once (`table_rebuilds`);
    what a step does per parameter on the host is a pointer comparison against the plan of the step before.
    `state_dict()` has torch.optim.AdamW's shape (`step` a float32 scalar on the CPU, `exp_avg`, `exp_avg_sq`) and
    loads into it, and the other way round.

    Parameters or gradients that are not contiguous CUDA fp32 (a CPU model) take torch's own functional AdamW on the
    same state: bit-identical to torch.optim.AdamW there.

    As with FusedSGD, the arena's in-place `zero_grad(set_to_none=False)` attaches a zeroed gradient to EVERY parameter:
    a parameter that never had a gradient then decays and counts steps where torch.optim.AdamW leaves it alone."""
    _ARENA_STATE = {"exp_avg": "exp_avg", "exp_avg_sq": "exp_avg_sq"}
    _TABLES_PER_GROUP = 8        # partitions seen lately (steady state: 1; a late gradient adds one)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, capturable=False):
        b1, b2 = betas
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                                      maximize=maximize))
        self._unsupported(self.param_groups, capturable)
        self._init_arena()

    @staticmethod
    def _unsupported(groups, capturable=False):
        for g in groups:
            for flag in ("amsgrad", "maximize", "capturable"):
                if g.get(flag, False) or (flag == "capturable" and capturable):
                    raise NotImplementedError(f"FusedAdamW: {flag}=True is not implemented")

    @staticmethod
    def _new_step():
        return torch.tensor(0.0, dtype=torch.float32)       # on the CPU, as torch's default (no launch to count)

    def _adopted(self, p, state):
        if "step" not in state:
            state["step"] = self._new_step()

    def load_state_dict(self, state_dict):
        self._unsupported(state_dict["param_groups"])
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            g.setdefault("amsgrad", False)
            g.setdefault("maximize", False)
        for st in self.state.values():
            if "step" in st:                                  # a number (old checkpoints) or a device tensor (fused=True)
                st["step"] = torch.as_tensor(float(st["step"]), dtype=torch.float32)

    def _drop_tables(self):
        super()._drop_tables()
        self._plans = {}

    def _table(self, gi, params, key):
        tables = self._tables.setdefault(gi, {})
        cached = tables.get(key)
        if cached is not None:
            return cached
        self.table_rebuilds += 1
        entries = (AdamEntry * len(params))()
        chunk = 0
        for e, p, k in zip(entries, params, key):
            e.param, e.grad, e.exp_avg, e.exp_avg_sq = k
            e.n, e.first_chunk = p.numel(), chunk
            chunk += (p.numel() + SGD_CHUNK - 1) // SGD_CHUNK
        host = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8)
        while len(tables) >= self._TABLES_PER_GROUP:
            del tables[next(iter(tables))]
        tables[key] = (host.to(params[0].device), len(params), chunk)
        return tables[key]

    def _plan(self, gi, params, key):
        """What a step does with the parameters of group `gi` that have a gradient, worked out once per set of
        (parameter, gradient) addresses `key`: which of them the kernel takes, their state and their table records."""
        state = self.state
        for p in params:
            st = state[p]
            if "exp_avg" not in st:                           # parameter outside the arena: state of its own, as torch's
                st["step"] = self._new_step()
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        ready = [_kernel_ready(p) and state[p]["exp_avg"].is_contiguous() and state[p]["exp_avg_sq"].is_contiguous()
                 for p in params]
        fused = [p for p, ok in zip(params, ready) if ok]
        rest = [p for p, ok in zip(params, ready) if not ok]
        plan = {"key": key, "fused": fused, "rest": rest, "steps": [state[p]["step"] for p in fused],
                "records": tuple((p.data_ptr(), p.grad.data_ptr(), state[p]["exp_avg"].data_ptr(),
                                  state[p]["exp_avg_sq"].data_ptr()) for p in fused)}
        self._plans[gi] = plan
        return plan

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.arena()
        launched = False
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            key = tuple([p.data_ptr() for p in params] + [p.grad.data_ptr() for p in params])
            plan = self._plans.get(gi)
            if plan is None or plan["key"] != key:
                plan = self._plan(gi, params, key)
            beta1, beta2 = group["betas"]
            rest, fused, steps = plan["rest"], plan["fused"], plan["steps"]
            if rest:                                          # torch's own update, on the same state
                state = self.state
                _torch_adamw(rest, [p.grad for p in rest], [state[p]["exp_avg"] for p in rest],
                             [state[p]["exp_avg_sq"] for p in rest], [], [state[p]["step"] for p in rest],
                             amsgrad=False, beta1=beta1, beta2=beta2, lr=group["lr"],
                             weight_decay=group["weight_decay"], eps=group["eps"], maximize=False)
            if not fused:
                continue
            torch._foreach_add_(steps, 1)                     # host tensors: no launch
            counts = torch.stack(steps).tolist()
            if counts.count(counts[0]) == len(counts):        # the steady state: one partition
                parts = [(counts[0], fused, plan["records"])]
            else:
                by_count = {}
                for i, t in enumerate(counts):
                    by_count.setdefault(t, []).append(i)
                parts = [(t, [fused[i] for i in idx], tuple(plan["records"][i] for i in idx))
                         for t, idx in by_count.items()]
            L = _lib.lib()
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for t, part, records in parts:
                table, n, chunks = self._table(gi, part, records)
                bc1 = 1 - beta1 ** t                          # Python doubles, as torch's _single_tensor_adam
                bc2_sqrt = (1 - beta2 ** t) ** 0.5
                check(L.dcfp_adamw_f32(C.c_void_p(table.data_ptr()), n, chunks, float(group["lr"]), beta1, beta2,
                                       group["eps"], group["weight_decay"], bc1, bc2_sqrt, stream), "adamw")
            launched = True
        if launched:
            self._weights_changed()
        return loss


def build_optimizer(config, model):
    skip_keywords = config.no_decay.split(",") if getattr(config, "no_decay", None) is not None else []
    parameters = set_weight_decay(model, [], skip_keywords)
    if config.optim == "sgd":
        return FusedSGD(parameters, momentum=config.momentum, lr=config.learning_rate,
                        weight_decay=config.weight_decay)
    if config.optim == "adamw":
        b1, b2 = map(float, config.betas.split(","))
        return FusedAdamW(parameters, betas=(b1, b2), lr=config.learning_rate, weight_decay=config.weight_decay)
    return None


def lr_poly(base_lr, iter, max_iter, power):
    return base_lr * ((1 - float(iter) / max_iter) ** power)


def lr_warmup(base_lr, iter, warmup_iter=1500, warmup_ratio=1e-6):
    if iter >= warmup_iter:
        return base_lr
    return base_lr * (1 - (1 - float(iter) / warmup_iter) * (1 - warmup_ratio))


def adjust_learning_rate(optimizer, learning_rate, i_iter, max_iter, power, warmup):
    lr = lr_poly(learning_rate, i_iter, max_iter, power)
    if warmup > 0:
        lr = lr_warmup(lr, i_iter, warmup_iter=warmup)
    for param_group in optimizer.param_groups:
        param_group["lr"] = lr
    return lr
