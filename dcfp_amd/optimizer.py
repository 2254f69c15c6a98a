"""Optimizer construction and LR schedule — API of optimizer.py:12-79.

`build_optimizer` returns FusedSGD: the torch.optim.SGD(momentum, weight_decay) update of the
reference (optimizer.py:24-25) executed as ONE multi-tensor HIP launch per step over a
device-resident pointer table (the reference issues four foreach launches over ~470 tensors),
or for `--optim adamw` FusedAdamW: torch.optim.AdamW (optimizer.py:26-31) on the same machinery.
param_groups / lr / weight_decay keep torch.optim semantics, so adjust_learning_rate works
unchanged."""
import contextlib
import ctypes as C
import math

import numpy as np
import torch
from torch.optim.adamw import adamw as _torch_adamw
from torch.optim.sgd import sgd as _torch_sgd

from . import _lib
from ._lib import AdamEntry, AdamExEntry, NormEntry, SgdEntry, SgdExEntry, SGD_CHUNK, check
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
    the cache of device pointer tables (`table_rebuilds` counts uploads).

    Both take `max_grad_norm` and `ema_decay`.  max_grad_norm: torch.nn.utils.clip_grad_norm_ over every
    parameter that has a gradient, all groups together, inside step(): two norm launches leave the coefficient on the
    device and the step launches multiply each gradient by it as they read it - no host read, and `p.grad` is NOT
    scaled (scorers and anything else that reads gradients see the raw ones); the norm is accumulated in fp64.
    ema_decay (0.5 < decay < 1): an exponential moving average of the weights as per-parameter state "ema" (an arena
    state buffer, in state_dict()), `ema = lerp(ema, p_new, 1 - decay)` in the step launch's epilogue for the parameters
    that launch updates; a parameter's average starts as a copy of the parameter.  With both None the optimizers call
    the plain entry points."""
    _ARENA_STATE = {}

    def _init_arena(self, max_grad_norm=None, ema_decay=None):
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not (math.isfinite(max_grad_norm) and max_grad_norm > 0):
                raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (a finite value > 0, or None)")
        if ema_decay is not None:
            ema_decay = float(ema_decay)
            if not 0.5 < ema_decay < 1.0:
                raise ValueError(f"Invalid ema_decay: {ema_decay} (0.5 < decay < 1, or None)")
            self._ARENA_STATE = dict(type(self)._ARENA_STATE, ema="ema")    # the EMA is per-parameter optimizer state
        self.max_grad_norm, self.ema_decay = max_grad_norm, ema_decay
        self._ema_w = 0.0 if ema_decay is None else 1.0 - ema_decay        # a double: rounded once where it is used
        self._ext = max_grad_norm is not None or ema_decay is not None     # the step goes through the *_ex entry points
        self._norm = None               # cached norm table: (key, table, n, chunks, workspace, tensor_sq, params)
        self._norm_result = None        # DcfpGradNorm on the device, as two doubles
        self._host_norm = None          # (norm, [squared norms], params) of a step that took torch's functions
        self._swapped = False
        self._drop_tables()
        self._arena = None
        self.table_rebuilds = 0

    def _drop_tables(self):
        self._tables = {}
        self._norm = None

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
                        if key == "ema":     # no loaded average for this parameter: it starts as the parameter itself
                            view.copy_(p.detach())
                        elif reused[key]:  # no loaded state for this parameter: it starts from zero, as torch.optim's would
                            view.zero_()
                    elif old.data_ptr() != view.data_ptr():
                        view.copy_(old)
                    state[key] = view
                self._adopted(p, state)
        return self._arena

    # ------------------------------------------------------------------ gradient-norm clipping
    def _clip(self):
        """The clip coefficient of this step over every parameter that has a gradient, all groups together, as
        clip_grad_norm_(model.parameters()) takes them; the gradients themselves stay as they are.
        None: no clipping; an int: the device address of the coefficient (two launches, no host read);
        a dict {parameter: scaled gradient}: parameters the kernels cannot take, through torch's own functions."""
        if self.max_grad_norm is None:
            return None
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        ready = [_kernel_ready(p) for p in params]
        if not all(ready):
            if any(ready):
                raise NotImplementedError("max_grad_norm over a mix of parameters the HIP kernels take and parameters "
                                          "they do not (CPU or non-contiguous) is not implemented")
            grads = [p.grad for p in params]
            total = torch.nn.utils.get_total_norm(grads, 2.0, False, None)        # what clip_grad_norm_ computes ...
            coef = torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0)       # ... and scales by
            self._host_norm = (total, [g.detach().double().pow(2).sum() for g in grads], params)
            return {p: g * coef.to(g.device) for p, g in zip(params, grads)}
        self._host_norm = None
        if self._norm_result is None:
            if not params:
                return None
            self._norm_result = torch.zeros(2, dtype=torch.float64, device=params[0].device)
        key = tuple((p.grad.data_ptr(), p.numel()) for p in params)
        if self._norm is None or self._norm[0] != key:
            self.table_rebuilds += 1
            entries = (NormEntry * max(1, len(params)))()
            chunk = 0
            for e, p in zip(entries, params):
                e.data, e.n, e.first_chunk = p.grad.data_ptr(), p.numel(), chunk
                chunk += (p.numel() + SGD_CHUNK - 1) // SGD_CHUNK
            dev = self._norm_result.device
            table = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8).to(dev)
            self._norm = (key, table, len(params), chunk, torch.empty(max(1, chunk), dtype=torch.float64, device=dev),
                          torch.zeros(max(1, len(params)), dtype=torch.float64, device=dev), params)
        _, table, n, chunks, ws, sq, _ = self._norm
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(_lib.lib().dcfp_grad_norm_f32(C.c_void_p(table.data_ptr()), n, chunks, self.max_grad_norm,
                                            C.c_void_p(ws.data_ptr()), ws.numel() * 8, C.c_void_p(sq.data_ptr()),
                                            C.c_void_p(self._norm_result.data_ptr()), stream), "grad_norm")
        return self._norm_result.data_ptr() + 12                # DcfpGradNorm.coef

    def grad_norm(self):
        """The global gradient norm of the last step, before clipping: a scalar on the parameters' device (reading it
        is the caller's sync).  None before the first clipped step."""
        if self._host_norm is not None:
            return self._host_norm[0]
        if self._norm_result is None or self._norm is None:
            return None
        return self._norm_result.view(torch.float32)[2]

    def grad_sqnorms(self):
        """[(parameter, its gradient's squared norm in fp64 - a scalar on the device)] of the last clipped step."""
        if self._host_norm is not None:
            return list(zip(self._host_norm[2], self._host_norm[1]))
        if self._norm is None:
            return []
        return list(zip(self._norm[6], self._norm[5][:self._norm[2]].unbind()))

    # ------------------------------------------------------------------ weight EMA
    def _ema_of(self, p):
        """The EMA of a parameter outside the arena: a copy of the parameter when it is first needed."""
        st = self.state[p]
        if "ema" not in st:
            st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
        return st["ema"]

    def _require_ema(self):
        if self.ema_decay is None:
            raise RuntimeError("this optimizer keeps no weight EMA (ema_decay=None)")

    def ema_state_dict(self, model):
        """model.state_dict() with every parameter this optimizer updates replaced by (a copy of) its EMA; buffers are
        the live ones.  What tools/evaluate.py --restore-from loads."""
        self._require_ema()
        self.arena()
        sd = model.state_dict()
        mine = {id(p) for p in self._all_params()}
        for name, p in model.named_parameters():
            if id(p) in mine and name in sd:
                sd[name] = self._ema_of(p).detach().clone()
        return sd

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate with the averaged weights in place: parameters and EMA change places (the arenas' contents, so every
        address stays what it was), the permuted weight copies are refreshed, and on exit everything is swapped back
        bit for bit.  step() inside the block raises."""
        self._require_ema()
        if self._swapped:
            raise RuntimeError("ema_weights() is already active")
        self._swap_ema()
        self._swapped = True
        try:
            yield self
        finally:
            self._swap_ema()
            self._swapped = False

    @torch.no_grad()
    def _swap_ema(self):
        ar = self.arena()
        if ar is not None:
            pairs = [(ar.flat_param, ar.state_buffer("ema"))]
        else:
            pairs = [(p.data, self._ema_of(p)) for p in self._all_params()]
        for a, b in pairs:
            tmp = a.clone()
            a.copy_(b)
            b.copy_(tmp)
        if ar is not None:
            self._weights_changed()
        else:
            from . import ops
            ops.WEIGHT_EPOCH[0] += 1

    def _check_may_step(self):
        if self._swapped:
            raise RuntimeError("step() inside ema_weights(): the parameters hold the averaged weights")

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

    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0, *, max_grad_norm=None, ema_decay=None):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))
        self._init_arena(max_grad_norm, ema_decay)

    def _table(self, gi, group, params):
        ema = self.ema_decay is not None
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["momentum_buffer"].data_ptr()) +
                    ((self.state[p]["ema"].data_ptr(),) if ema else ()) for p in params) + (group["weight_decay"],)
        cached = self._tables.get(gi)
        if cached is not None and cached[0] == key:
            return cached[1], cached[2], cached[3]
        self.table_rebuilds += 1
        entries = ((SgdExEntry if self._ext else SgdEntry) * len(params))()
        chunk = 0
        for i, p in enumerate(params):
            e = entries[i]
            e.param, e.grad, e.momentum_buf = p.data_ptr(), p.grad.data_ptr(), self.state[p]["momentum_buffer"].data_ptr()
            if ema:
                e.ema = self.state[p]["ema"].data_ptr()
            e.n, e.first_chunk, e.weight_decay = p.numel(), chunk, group["weight_decay"]
            chunk += (p.numel() + SGD_CHUNK - 1) // SGD_CHUNK
        host = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8)
        dev = host.to(params[0].device)
        self._tables[gi] = (key, dev, len(params), chunk)
        return dev, len(params), chunk

    def _step_torch(self, group, params, scaled):
        """torch's own SGD, on the same state, for parameters the kernels cannot take (a CPU model)."""
        bufs = []
        for p in params:
            st = self.state[p]
            if "momentum_buffer" not in st:
                st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            bufs.append(st["momentum_buffer"])
        emas = [self._ema_of(p) for p in params] if self.ema_decay is not None else []      # (before the update)
        _torch_sgd(params, [scaled.get(p, p.grad) for p in params], bufs, weight_decay=group["weight_decay"],
                   momentum=group["momentum"], lr=group["lr"], dampening=0.0, nesterov=False, maximize=False)
        for p, e in zip(params, emas):
            e.lerp_(p, self._ema_w)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_may_step()
        self.arena()
        clip = self._clip()
        launched = not self._ext
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            if self._ext and not all(_kernel_ready(p) for p in params):
                if any(_kernel_ready(p) for p in params):
                    raise NotImplementedError("FusedSGD: a param group mixing parameters the HIP kernel takes with "
                                              "others, with max_grad_norm or ema_decay set")
                self._step_torch(group, params, clip if isinstance(clip, dict) else {})
                continue
            for p in params:
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() \
                        or not p.grad.is_contiguous():
                    raise RuntimeError("FusedSGD: parameters and grads must be contiguous CUDA fp32")
                if "momentum_buffer" not in self.state[p]:     # parameter outside the arena
                    self.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if self.ema_decay is not None:
                    self._ema_of(p)
            table, n, chunks = self._table(gi, group, params)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            L = _lib.lib()
            launched = True
            if self._ext:
                check(L.dcfp_sgd_momentum_ex_f32(C.c_void_p(table.data_ptr()), n, chunks, float(group["lr"]),
                                                 float(group["momentum"]), 0, C.c_void_p(clip), self._ema_w, stream),
                      "sgd_momentum_ex")
            else:
                check(L.dcfp_sgd_momentum_f32(C.c_void_p(table.data_ptr()), n, chunks, float(group["lr"]),
                                              float(group["momentum"]), 0, stream), "sgd_momentum")
        if launched:
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
                 maximize=False, capturable=False, max_grad_norm=None, ema_decay=None):
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
        self._init_arena(max_grad_norm, ema_decay)

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
        entries = ((AdamExEntry if self._ext else AdamEntry) * len(params))()
        chunk = 0
        for e, p, k in zip(entries, params, key):
            if self._ext:
                e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.ema = k        # (ema 0: none)
            else:
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
        ema = self.ema_decay is not None
        if ema:
            for p in params:
                self._ema_of(p)                               # (a parameter outside the arena: its value before the step)
        ready = [_kernel_ready(p) and state[p]["exp_avg"].is_contiguous() and state[p]["exp_avg_sq"].is_contiguous()
                 and (not ema or self._ema_of(p).is_contiguous()) for p in params]
        fused = [p for p, ok in zip(params, ready) if ok]
        rest = [p for p, ok in zip(params, ready) if not ok]
        plan = {"key": key, "fused": fused, "rest": rest, "steps": [state[p]["step"] for p in fused],
                "records": tuple((p.data_ptr(), p.grad.data_ptr(), state[p]["exp_avg"].data_ptr(),
                                  state[p]["exp_avg_sq"].data_ptr()) +
                                 (((state[p]["ema"].data_ptr() if ema else 0),) if self._ext else ()) for p in fused)}
        self._plans[gi] = plan
        return plan

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_may_step()
        self.arena()
        clip = self._clip()
        scaled = clip if isinstance(clip, dict) else {}
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
                _torch_adamw(rest, [scaled.get(p, p.grad) for p in rest], [state[p]["exp_avg"] for p in rest],
                             [state[p]["exp_avg_sq"] for p in rest], [], [state[p]["step"] for p in rest],
                             amsgrad=False, beta1=beta1, beta2=beta2, lr=group["lr"],
                             weight_decay=group["weight_decay"], eps=group["eps"], maximize=False)
                if self.ema_decay is not None:
                    for p in rest:
                        self._ema_of(p).lerp_(p, self._ema_w)
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
                if self._ext:
                    check(L.dcfp_adamw_ex_f32(C.c_void_p(table.data_ptr()), n, chunks, float(group["lr"]), beta1, beta2,
                                              group["eps"], group["weight_decay"], bc1, bc2_sqrt,
                                              C.c_void_p(None if isinstance(clip, dict) else clip), self._ema_w, stream),
                          "adamw_ex")
                else:
                    check(L.dcfp_adamw_f32(C.c_void_p(table.data_ptr()), n, chunks, float(group["lr"]), beta1, beta2,
                                           group["eps"], group["weight_decay"], bc1, bc2_sqrt, stream), "adamw")
            launched = True
        if launched:
            self._weights_changed()
        return loss


def build_optimizer(config, model):
    skip_keywords = config.no_decay.split(",") if getattr(config, "no_decay", None) is not None else []
    parameters = set_weight_decay(model, [], skip_keywords)
    extras = dict(max_grad_norm=getattr(config, "clip_grad_norm", None), ema_decay=getattr(config, "ema_decay", None))
    if config.optim == "sgd":
        return FusedSGD(parameters, momentum=config.momentum, lr=config.learning_rate,
                        weight_decay=config.weight_decay, **extras)
    if config.optim == "adamw":
        b1, b2 = map(float, config.betas.split(","))
        return FusedAdamW(parameters, betas=(b1, b2), lr=config.learning_rate, weight_decay=config.weight_decay,
                          **extras)
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
