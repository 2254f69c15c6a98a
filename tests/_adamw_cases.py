"""Shared by test_adamw_host_cpu.py and test_adamw_gpu.py: the inputs of the AdamW kernel test with their fp64 reference
and per-element roundoff bound, a plain numpy fp32 restatement of the kernel's lines, and the scripted optimizer driver
(the `_Run` protocol of test_step_kernels_gpu.py, for AdamW).

The roundoff bound.  The kernel (dcfp_amd/csrc/adamw.hip) receives fp32 scalars, forms decay = 1 - lr*wd, step = lr/bc1,
w = 1 - beta1 and c = 1 - beta2 in double and rounds each ONCE to fp32, then per element, every operation rounded once
(u = 2^-24, first order):

    p1 = fl(p*decay)                          |dp1| <= 2u|p1|                       (decay's rounding, the product's)
    d  = fl(g - m)
    m1 = fma(w, d, m)            [w < 0.5]    |dm|  <= u(|m1| + 2 w|d|)             (d's and w's rounding, the fma's)
    m1 = fma(-fl(1-w), d, g)     [w >= 0.5]   |dm|  <= u(|m1| + (2-w)|d|)           (fl(1-w) is exact; w's rounding is
                                                                                     an ABSOLUTE u*w <= u on the factor)
    v1 = fma(c, fl(g*g), fl(beta2*v))         |dv|  <= u(v1 + beta2 v + 2 c g^2)    (g*g, c, beta2*v, the fma)
    s  = fl(sqrt(v1)); q = fl(s/bc2s); den = fl(q + eps)
                                              |dden| <= q(dv/(2 v1) + 2u) + u den   (dv/v1 := 0 where v1 = 0: s = 0 exactly)
    r  = fl(m1/den)                           |dr|  <= dm/den + |r|(dden/den + u)
    p2 = fma(-step, r, p1)                    |dp2| <= dp1 + step(dr + u|r|) + u|p2| (step's rounding, the fma's)

and the asserted bound is TWICE that, as test_sgd_kernel_against_fp64_per_element does.  The reference evaluates the same
lines in fp64 from the fp32 inputs and the fp32 scalars as passed, with decay, step, w, c exact."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
CHUNK = 16384
FIXED_SIZES = [1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 2 * 16384, 70001]
SENT = np.float32(-12345.678)
BETA2, EPS = 0.999, 1e-8

#          step  lr    weight decay  beta1  state
KERNEL_CASES = {
    "step1-zero-state": (1, 1e-3, 0.01, 0.9, "zero"),
    "step1000": (1000, 1e-3, 0.01, 0.9, "random"),
    "step1000-wd0": (1000, 1e-3, 0.0, 0.9, "random"),
    "lr0-decay-only": (1000, 0.0, 0.01, 0.9, "random"),
    "lr0-wd0": (1000, 0.0, 0.0, 0.9, "random"),
    "beta1-0": (7, 1e-3, 0.01, 0.0, "random"),
}


@functools.lru_cache(maxsize=None)
def layout():
    """(sizes, offsets, total): every fixed size once at a 16-byte aligned offset and once at residue 1, 2 or 3, then
    300 random sizes in 1..300 at residues 0, 1, 2, 3 in turn; at least one sentinel in front of every tensor."""
    rng = np.random.RandomState(61)
    sizes, residues = [], []
    for i, n in enumerate(FIXED_SIZES):
        sizes += [n, n]
        residues += [0, 1 + i % 3]
    rnd = rng.randint(1, 301, 300).tolist()
    sizes += rnd
    residues += [i % 4 for i in range(len(rnd))]
    offs, off = [], 0
    for n, r in zip(sizes, residues):
        off += int(rng.randint(1, 70))
        off += (r - off) % 4
        offs.append(off)
        off += n
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    return sizes, offs, off + 64


def chunks_of(sizes):
    first, c = [], 0
    for n in sizes:
        first.append(c)
        c += (n + CHUNK - 1) // CHUNK
    return first, c


@functools.lru_cache(maxsize=None)
def kernel_inputs(state):
    """fp32 host arrays p, g, m, v over the flat layout (sentinels in the gaps) and the mask of live elements."""
    sizes, offs, total = layout()
    rng = np.random.RandomState(67)
    live = np.zeros(total, bool)
    for n, o in zip(sizes, offs):
        live[o:o + n] = True
    n = int(live.sum())

    def log_uniform():
        return np.exp(rng.uniform(np.log(1e-6), np.log(10.0), n))
    host = {k: np.full(total, SENT, np.float32) for k in "pgmv"}
    host["p"][live] = rng.randn(n).astype(np.float32)
    g = log_uniform() * rng.choice([-1.0, 1.0], n)
    g[rng.rand(n) < 0.05] = 0.0
    host["g"][live] = g.astype(np.float32)
    if state == "zero":
        host["m"][live] = 0.0
        host["v"][live] = 0.0
    else:
        host["m"][live] = (0.5 * rng.randn(n)).astype(np.float32)
        v = log_uniform() ** 2
        v[rng.rand(n) < 0.05] = 0.0
        host["v"][live] = v.astype(np.float32)
    for a in host.values():
        a.setflags(write=False)
    return host, live


def scalars(step, lr, wd, beta1, beta2=BETA2, eps=EPS):
    """The fp32 arguments of dcfp_adamw_f32 as FusedAdamW.step forms them (bias corrections in Python doubles)."""
    return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=wd,
                bc1=1 - beta1 ** step, bc2_sqrt=(1 - beta2 ** step) ** 0.5)


def _f(x):
    return float(np.float32(x))


def reference(p, g, m, v, sc):
    """fp64 arrays -> dict(m, v, p: the fp64 results; bm, bv, bp: the per-element bounds of the module docstring)."""
    lr, wd, b1, b2, eps = _f(sc["lr"]), _f(sc["weight_decay"]), _f(sc["beta1"]), _f(sc["beta2"]), _f(sc["eps"])
    bc1, bc2s = _f(sc["bc1"]), _f(sc["bc2_sqrt"])
    decay, step, w, c = 1 - lr * wd, lr / bc1, 1 - b1, 1 - b2
    p1 = p * decay
    d = g - m
    m1 = m + w * d
    bm = U * (np.abs(m1) + (2 * w if np.float32(w) < 0.5 else 2 - w) * np.abs(d))
    v1 = b2 * v + c * g * g
    bv = U * (v1 + b2 * v + 2 * c * g * g)
    q = np.sqrt(v1) / bc2s
    den = q + eps
    rel_v = np.divide(bv, v1, out=np.zeros_like(v1), where=v1 > 0)
    bden = q * (rel_v / 2 + 2 * U) + U * den
    r = m1 / den
    br = bm / den + np.abs(r) * (bden / den + U)
    p2 = p1 - step * r
    bp = 2 * U * np.abs(p1) + step * (br + U * np.abs(r)) + U * np.abs(p2)
    return dict(m=m1, v=v1, p=p2, bm=2 * bm, bv=2 * bv, bp=2 * bp)


def restate32(p, g, m, v, sc):
    """The kernel's lines in plain numpy fp32 (no fma: the products round on their own)."""
    f = np.float32
    lr, wd, b1, b2 = _f(sc["lr"]), _f(sc["weight_decay"]), _f(sc["beta1"]), _f(sc["beta2"])
    decay, step, w, c = f(1 - lr * wd), f(lr / _f(sc["bc1"])), f(1 - b1), f(1 - b2)
    p1 = p * decay
    d = g - m
    m1 = m + w * d if w < 0.5 else g - d * (f(1) - w)
    v1 = f(b2) * v + c * (g * g)
    den = np.sqrt(v1) / f(sc["bc2_sqrt"]) + f(sc["eps"])
    p2 = p1 - step * (m1 / den)
    assert p2.dtype == m1.dtype == v1.dtype == np.float32
    return dict(p=p2, m=m1, v=v1)


def worst_ratios(out, ref):
    """max |err| / bound for m, v, p (a zero bound demands a zero error)."""
    res = {}
    for k in "mvp":
        err, b = np.abs(out[k].astype(np.float64) - ref[k]), ref["b" + k]
        assert np.isfinite(out[k]).all(), k
        assert (err[b == 0] == 0).all(), k
        res[k] = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    return res


# ---------------------------------------------------------------------------------------------- scripted optimizer runs
SHAPES = [(7,), (16383,), (16385,), (3, 5, 3, 3), (1,), (40000,), (16384,), (255,)]
GROUP_OF = [0, 0, 0, 0, 0, 1, 1, 1]
BASE_LR, BETAS, WD, STEPS = 1e-2, (0.9, 0.999), 1e-2, 6


def grad_of(step, i):
    g = torch.Generator().manual_seed(100 * step + i + 1)
    return torch.randn(SHAPES[i], generator=g) * 0.5


def init_of(i):
    g = torch.Generator().manual_seed(9000 + i)
    return torch.randn(SHAPES[i], generator=g)


class Run:
    """One optimizer driven through a script of steps; the same driver serves FusedAdamW on either device and
    torch.optim.AdamW on the CPU (gradients are handed over the way the backward kernels do: into the arena's view where
    there is one)."""

    def __init__(self, factory, device, dtype):
        self.factory, self.device, self.dtype = factory, device, dtype
        self.params = [torch.nn.Parameter(init_of(i).to(device=device, dtype=dtype)) for i in range(len(SHAPES))]
        self.opt = self._make(self.params)
        self.fresh_state = self.opt.state_dict()          # of an optimizer that never stepped
        self.history = []
        self.floor = [torch.zeros(s, dtype=torch.float64) for s in SHAPES]

    def _make(self, params):
        groups = [{"params": [p for p, gi in zip(params, GROUP_OF) if gi == 0]},
                  {"params": [p for p, gi in zip(params, GROUP_OF) if gi == 1], "weight_decay": 0.0}]
        return self.factory(groups, lr=BASE_LR, betas=BETAS, eps=EPS, weight_decay=WD)

    def give(self, p, g):
        from dcfp_amd import arena
        g = g.to(device=self.device, dtype=self.dtype)
        t, token = arena.grad_target(p)
        t.copy_(g)
        out = arena.grad_commit(p, t, token)
        if out is not None:                               # what autograd's AccumulateGrad does with a returned gradient
            p.grad = out if p.grad is None else p.grad + out

    def resume(self):
        sd = self.opt.state_dict()
        self.params = [torch.nn.Parameter(p.detach().clone()) for p in self.params]
        self.opt = self._make(self.params)
        self.opt.load_state_dict(sd)

    def step(self, it, spec):
        from dcfp_amd import optimizer as om
        for ev in spec.get("before", ()):
            if ev == "resume":
                self.resume()
            elif ev == "load_fresh":
                self.opt.load_state_dict(self.fresh_state)
            elif ev == "load_partial":                        # the state of parameters 1 and 5 is missing from the checkpoint
                sd = self.opt.state_dict()
                self.opt.load_state_dict({"state": {k: v for k, v in sd["state"].items() if k not in (1, 5)},
                                          "param_groups": sd["param_groups"]})
            elif ev == "move_out":
                for i in (1, 5):
                    self.params[i].data = self.params[i].data.clone()
            elif ev[0] == "wd":
                self.opt.param_groups[ev[1]]["weight_decay"] = ev[2]
        self.opt.zero_grad(set_to_none=spec.get("to_none", True))
        om.adjust_learning_rate(self.opt, BASE_LR, it, 20, 0.9, -1)
        for i, p in enumerate(self.params):
            if i not in spec.get("no_grad", ()):
                self.give(p, grad_of(it, i))
        if self.dtype == torch.float64:
            self._floor_terms()
        self.opt.step()
        self.history.append([p.detach().cpu().clone() for p in self.params])

    def steps_taken(self):
        return [float(self.opt.state[p]["step"]) if "step" in self.opt.state.get(p, {}) else 0.0 for p in self.params]

    def _floor_terms(self):
        """The per-element roundoff bound of one update (`reference`), from the fp64 run's values, summed over the steps:
        the floor below which a difference says nothing."""
        for group in self.opt.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                i = next(k for k, q in enumerate(self.params) if q is p)
                st = self.opt.state.get(p, {})
                t = float(st["step"]) + 1 if "step" in st else 1.0
                zeros = np.zeros(p.shape)
                m = st["exp_avg"].numpy() if "exp_avg" in st else zeros
                v = st["exp_avg_sq"].numpy() if "exp_avg_sq" in st else zeros
                sc = scalars(t, group["lr"], group["weight_decay"], *group["betas"], group["eps"])
                ref = reference(p.detach().numpy(), p.grad.numpy(), m, v, sc)
                self.floor[i] += torch.from_numpy(ref["bp"])


def drive(run, script):
    for it, spec in enumerate(script):
        run.step(it, spec)
    if run.device.type == "cuda":
        torch.cuda.synchronize()
    return run
