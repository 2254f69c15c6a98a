"""dcfp_grad_norm_f32, dcfp_sgd_momentum_ex_f32 and dcfp_adamw_ex_f32 through the C ABI on hand-built tables (tensors of
1 ... 40000 elements at every start residue mod 4, sentinels in every gap), FusedSGD / FusedAdamW with max_grad_norm and
ema_decay, and the driver with --clip-grad-norm / --ema-decay: continue and the data-parallel wrapper."""
import contextlib
import ctypes as C
import importlib
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _adamw_cases as ac
import _clip_ema_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIZES, NO_GRAD = ref.SIZES, ref.NO_GRAD
WITH_GRAD = [i for i in range(len(SIZES)) if i != NO_GRAD]
LR, MOMENTUM, WD = 0.05, 0.9, (1e-2, 0.0)               # the two groups differ in weight decay
DECAY = 0.9
SENT_BITS = int(np.float32(ref.SENT).view(np.int32))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _upload(entries, cuda):
    return torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8).to(cuda)


class Flat:
    """One flat, sentinel-filled device buffer per operand (p, g, state, ema) with the tensors of ref.layout(shift)."""

    def __init__(self, cuda, kind, shift, ema):
        self.cuda, self.kind, self.shift = cuda, kind, shift
        self.offs, self.total = ref.layout(shift)
        self.names = "pg" + ("b" if kind == "sgd" else "mv") + ("e" if ema else "")
        self.live = np.zeros(self.total, bool)
        for n, o in zip(SIZES, self.offs):
            self.live[o:o + n] = True
        rng = np.random.RandomState(7)
        self.dev = {}
        for k in self.names:
            self.dev[k] = torch.full((self.total,), float(ref.SENT), dtype=torch.float32, device=cuda)
            assert self.dev[k].data_ptr() % 256 == 0
        init = [rng.randn(n).astype(np.float32) for n in SIZES]
        self.put("p", init)
        for k in self.names[2:]:
            self.put(k, init if k == "e" else [np.zeros(n, np.float32) for n in SIZES])
        self.step_no = 0

    def put(self, k, arrays):
        host = self.dev[k].cpu().numpy()
        for a, n, o in zip(arrays, SIZES, self.offs):
            host[o:o + n] = a
        self.dev[k].copy_(torch.from_numpy(host))

    def view(self, k, i):
        return self.dev[k][self.offs[i]:self.offs[i] + SIZES[i]]

    def ptr(self, k, i):
        return self.dev[k].data_ptr() + 4 * self.offs[i]

    def live_bits(self, k):
        return self.dev[k].cpu().numpy()[self.live].view(np.int32)

    def sentinels_intact(self):
        return all(bool((self.dev[k].cpu().numpy()[~self.live].view(np.int32) == SENT_BITS).all()) for k in self.names)

    def aligned(self):
        return [i for i in WITH_GRAD if self.ptr("p", i) % 16 == 0]

    # -------------------------------------------------------------------------------------------------- the launches
    def norm(self, max_norm, tensors=WITH_GRAD, result=None, workspace="own", ws_bytes=None, table="own", n=None,
             chunks=None, tensor_sq="own"):
        """dcfp_grad_norm_f32 over the gradients of `tensors` -> (status, result as 2 doubles, per-tensor doubles)."""
        from dcfp_amd import _lib
        L = _lib.lib()
        first, total_chunks = ref.chunks_of([SIZES[i] for i in tensors])
        entries = (_lib.NormEntry * max(1, len(tensors)))()
        for e, i, fc in zip(entries, tensors, first):
            e.data, e.n, e.first_chunk = self.ptr("g", i), SIZES[i], fc
        self._keep = tab = _upload(entries, self.cuda)
        res = torch.zeros(2, dtype=torch.float64, device=self.cuda) if result is None else result
        ws = torch.zeros(max(1, total_chunks), dtype=torch.float64, device=self.cuda)
        sq = torch.full((max(1, len(tensors)),), -1.0, dtype=torch.float64, device=self.cuda)
        assert L.dcfp_grad_norm_workspace_bytes(total_chunks) == 8 * total_chunks
        status = L.dcfp_grad_norm_f32(
            C.c_void_p(tab.data_ptr() if table == "own" else table), len(tensors) if n is None else n,
            total_chunks if chunks is None else chunks, max_norm,
            C.c_void_p(ws.data_ptr() if workspace == "own" else workspace), 8 * total_chunks if ws_bytes is None else ws_bytes,
            C.c_void_p(sq.data_ptr() if tensor_sq == "own" else tensor_sq), C.c_void_p(res.data_ptr()), _stream())
        return status, res, sq

    def step(self, plain, coef=None):
        """One optimizer step over the tensors that have a gradient, one launch per group; `plain`: the existing entry
        points (DcfpSgdEntry / DcfpAdamEntry), else the *_ex ones with `coef` (a device address or None) and the EMA."""
        from dcfp_amd import _lib
        L = _lib.lib()
        self.step_no += 1
        ema = "e" in self.names
        for gi in (0, 1):
            idx = [i for i in WITH_GRAD if ref.GROUP_OF[i] == gi]
            first, chunks = ref.chunks_of([SIZES[i] for i in idx])
            if self.kind == "sgd":
                entries = ((_lib.SgdEntry if plain else _lib.SgdExEntry) * len(idx))()
                for e, i, fc in zip(entries, idx, first):
                    e.param, e.grad, e.momentum_buf = self.ptr("p", i), self.ptr("g", i), self.ptr("b", i)
                    e.n, e.first_chunk, e.weight_decay = SIZES[i], fc, WD[gi]
                    if ema:
                        e.ema = self.ptr("e", i)
                tab = _upload(entries, self.cuda)
                if plain:
                    st = L.dcfp_sgd_momentum_f32(C.c_void_p(tab.data_ptr()), len(idx), chunks, LR, MOMENTUM, 0, _stream())
                else:
                    st = L.dcfp_sgd_momentum_ex_f32(C.c_void_p(tab.data_ptr()), len(idx), chunks, LR, MOMENTUM, 0,
                                                    C.c_void_p(coef), 1.0 - DECAY if ema else 0.0, _stream())
            else:
                entries = ((_lib.AdamEntry if plain else _lib.AdamExEntry) * len(idx))()
                for e, i, fc in zip(entries, idx, first):
                    e.param, e.grad, e.exp_avg, e.exp_avg_sq = (self.ptr(k, i) for k in "pgmv")
                    e.n, e.first_chunk = SIZES[i], fc
                    if ema:
                        e.ema = self.ptr("e", i)
                tab = _upload(entries, self.cuda)
                sc = ac.scalars(self.step_no, LR, WD[gi], 0.9)
                args = (C.c_void_p(tab.data_ptr()), len(idx), chunks, sc["lr"], sc["beta1"], sc["beta2"], sc["eps"],
                        sc["weight_decay"], sc["bc1"], sc["bc2_sqrt"])
                if plain:
                    st = L.dcfp_adamw_f32(*args, _stream())
                else:
                    st = L.dcfp_adamw_ex_f32(*args, C.c_void_p(coef), 1.0 - DECAY if ema else 0.0, _stream())
            assert st == 0, st
            torch.cuda.synchronize()           # (the table is freed when `tab` goes)


def _grads(kind, it=0, scale=1.0):
    g = [a * np.float32(scale) for a in ref.values(kind, seed=it)]
    g[NO_GRAD] = np.full(SIZES[NO_GRAD], 1e30, np.float32)          # the stale arena slot of the parameter without grad
    return g


# ====================================================================================================== the norm kernel
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["randn", "tiny", "huge", "inf", "nan"])
def test_grad_norm_kernel(cuda, capsys, kind, shift):
    """sqnorm within rel 1e-10 of the fp64 restatement (sequential fp64 summation of <= 2^19 exact squares is bounded by
    n * 2^-53 ~ 6e-11), norm within one fp32 ulp of the restated one, coef the restated formula on the kernel's own norm
    bit for bit, the per-tensor values to the same bound, the gradient-less parameter's stale 1e30 excluded, two calls
    the same bits, gradients and sentinels untouched."""
    MAXN = 0.5
    f = Flat(cuda, "sgd", shift, ema=False)
    g = _grads(kind)
    f.put("g", g)
    g_bits = f.live_bits("g")
    st, res, sq = f.norm(MAXN)
    st2, res2, sq2 = f.norm(MAXN)
    torch.cuda.synchronize()
    assert st == 0 and st2 == 0
    assert ref.torch_bits_equal(res, res2) and ref.torch_bits_equal(sq, sq2)
    sqnorm = float(res[0])
    norm, coef = (np.float32(v) for v in res.view(torch.float32)[2:4].tolist())
    want_sq, want_per = ref.sqnorm64([g[i] for i in WITH_GRAD])
    per = sq.tolist()
    if kind in ("randn", "tiny", "huge"):
        assert math.isfinite(sqnorm) and abs(sqnorm - want_sq) <= 1e-10 * want_sq, (sqnorm, want_sq)
        assert sqnorm < 1e55                                       # (the stale 1e30 slot would have brought 5e60)
        for a, b in zip(per, want_per):
            assert abs(a - b) <= 1e-10 * b
        want_norm = ref.norm32(want_sq)
        assert abs(float(norm) - float(want_norm)) <= float(np.spacing(want_norm)), (norm, want_norm)
        assert float(norm) > 0 and math.isfinite(float(norm))
    elif kind == "inf":
        assert sqnorm == math.inf and norm == np.inf and coef == 0.0
        assert per[WITH_GRAD.index(6)] == math.inf and sum(not math.isfinite(v) for v in per) == 1
    else:
        assert math.isnan(sqnorm) and math.isnan(norm) and math.isnan(coef)
        assert math.isnan(per[WITH_GRAD.index(7)]) and sum(not math.isfinite(v) for v in per) == 1
    if kind != "nan":
        assert coef.view(np.int32) == ref.coef32(norm, MAXN).view(np.int32), (coef, norm)
    assert np.array_equal(f.live_bits("g"), g_bits) and f.sentinels_intact()
    with capsys.disabled():
        print("\n[grad_norm %s shift %d] sqnorm %.17g (fp64 restatement %.17g) norm %r coef %r"
              % (kind, shift, sqnorm, want_sq, float(norm), float(coef)))


def test_grad_norm_empty_table_and_refusals(cuda):
    from dcfp_amd import _lib
    f = Flat(cuda, "sgd", 0, ema=False)
    f.put("g", _grads("randn"))
    st, res, _ = f.norm(0.5, tensors=[], table=None, workspace=None, tensor_sq=None)
    torch.cuda.synchronize()
    assert st == 0 and float(res[0]) == 0.0 and res.view(torch.float32)[2:4].tolist() == [0.0, 1.0]
    st, res, _ = f.norm(1e-9, tensors=[])                         # {0, 0, 1} whatever max_norm / 1e-6 would say
    torch.cuda.synchronize()
    assert st == 0 and res.view(torch.float32)[2:4].tolist() == [0.0, 1.0]

    def untouched(**kw):
        out = torch.full((2,), -7.0, dtype=torch.float64, device=cuda)
        st, _, sq = f.norm(kw.pop("max_norm", 0.5), result=out, **kw)
        torch.cuda.synchronize()
        assert out.tolist() == [-7.0, -7.0] and bool((sq == -1.0).all()), "something was launched"
        return st
    assert untouched(table=None) == _lib.E_BADDESC
    assert untouched(n=-1) == _lib.E_BADDESC
    assert untouched(chunks=-1) == _lib.E_BADDESC
    for bad in (0.0, -1.0, float("nan")):
        assert untouched(max_norm=bad) == _lib.E_BADDESC
    assert untouched(workspace=None) == _lib.E_WORKSPACE
    assert untouched(ws_bytes=8 * 7) == _lib.E_WORKSPACE           # (the table has 10 chunks)
    assert f.sentinels_intact()


# ====================================================================================================== the clipped step
def _clipped_run(cuda, kind, shift, max_norm, ema=False, check=True):
    """Three steps of the *_ex entry points with the kernel's own coefficient next to three steps of the PLAIN entry
    points on gradients multiplied by that coefficient with torch.mul -> the clipped run."""
    a, b = Flat(cuda, kind, shift, ema), Flat(cuda, kind, shift, False)
    ema_ref = [a.view("p", i).clone() for i in range(len(SIZES))]
    for it in range(3):
        g = _grads("randn", it, scale=3.0 + it)
        a.put("g", g)
        g_bits = a.live_bits("g")
        st, res, _ = a.norm(max_norm)
        assert st == 0
        coef = res.view(torch.float32)[3]
        a.step(plain=False, coef=res.data_ptr() + 12)
        if max_norm < 1:
            assert 0 < float(coef) < 1                             # the clip bites on every step
            b.dev["g"].copy_(torch.mul(a.dev["g"], coef))
        else:
            assert float(coef) == 1.0
            b.dev["g"].copy_(a.dev["g"])                           # the unclipped optimizer
        b.step(plain=True)
        if check:
            for k in b.names:
                if k != "g":
                    assert np.array_equal(a.live_bits(k), b.live_bits(k)), (kind, shift, it, k)
            assert np.array_equal(a.live_bits("g"), g_bits), "the gradient was written"
            assert a.sentinels_intact()
        if ema:
            for i in WITH_GRAD:
                ema_ref[i] = torch.lerp(ema_ref[i], a.view("p", i), 1.0 - DECAY)
    return a, ema_ref


@pytest.mark.parametrize("max_norm", [0.05, 1e30])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clipped_step_equals_plain_step_on_scaled_gradients(cuda, kind, shift, max_norm):
    a, _ = _clipped_run(cuda, kind, shift, max_norm)
    assert len(a.aligned()) >= 1 and len(a.aligned()) < len(WITH_GRAD)      # both paths ran


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_vector_and_scalar_paths_give_the_same_bits(cuda, kind):
    """The same values at four placements: every tensor is on the 16-byte grid in exactly one of them."""
    runs = [_clipped_run(cuda, kind, shift, 0.05, ema=True, check=False)[0] for shift in range(4)]
    assert sorted(i for r in runs for i in r.aligned()) == WITH_GRAD
    for r in runs[1:]:
        for k in r.names:
            assert np.array_equal(r.live_bits(k), runs[0].live_bits(k)), (kind, r.shift, k)
        assert r.sentinels_intact()


def test_null_coef_and_no_ema_equal_the_plain_entry_points(cuda):
    for kind in ("sgd", "adamw"):
        a, b = Flat(cuda, kind, 0, False), Flat(cuda, kind, 0, False)
        for it in range(2):
            for f in (a, b):
                f.put("g", _grads("randn", it))
            a.step(plain=False, coef=None)
            b.step(plain=True)
        for k in a.names:
            assert np.array_equal(a.live_bits(k), b.live_bits(k)), (kind, k)


def test_clipped_sgd_against_the_fp32_restatement(cuda):
    """One clipped SGD step from a zero buffer against tests/_clip_ema_ref.sgd32 (each fma formed in fp64 and rounded
    once: the restatement's double rounding can cost the last bit, so one ulp per value)."""
    f = Flat(cuda, "sgd", 0, False)
    g = _grads("randn", 0, scale=3.0)
    f.put("g", g)
    p0 = [f.view("p", i).cpu().numpy() for i in range(len(SIZES))]
    _, res, _ = f.norm(0.05)
    f.step(plain=False, coef=res.data_ptr() + 12)
    coef = np.float32(float(res.view(torch.float32)[3]))
    for i in WITH_GRAD:
        p1, b1 = ref.sgd32(p0[i], g[i], np.zeros_like(g[i]), coef, LR, MOMENTUM, WD[ref.GROUP_OF[i]])
        for got, want in ((f.view("p", i), p1), (f.view("b", i), b1)):
            got = got.cpu().numpy()
            assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), i


def test_clipped_adamw_against_torch_adamw_on_the_device(cuda, capsys):
    """One step from zero state: FusedAdamW(max_grad_norm) and torch.optim.AdamW fed torch.mul(g, coef).  The bound per
    element is the sum of
      * 2 bp: each side lies within the roundoff bound bp of tests/_adamw_cases.reference (itself twice the first-order
        bound) of the fp64 result of ITS scalars;
      * the scalars: dcfp_adamw_f32 has always received beta2 as an fp32 value and formed 1 - beta2 from it, torch forms
        1 - beta2 in double.  Rounding beta2 moves c = 1 - beta2 by at most u*beta2, a relative u*beta2/c = 6e-5 at
        beta2 = 0.999; from zero state v = c*g^2, so the denominator moves by half of that and so does the update
        |p2 - p1|  (the bias correction comes from Python doubles on both sides and does not cancel it at step 1)."""
    from dcfp_amd.optimizer import FusedAdamW
    mine, theirs = _params(cuda), _params(cuda)
    opt = FusedAdamW(_groups(mine), lr=LR, weight_decay=WD[0], max_grad_norm=0.05)
    top = torch.optim.AdamW(_groups(theirs), lr=LR, weight_decay=WD[0])
    g = _grads("randn", 0, scale=3.0)
    opt.zero_grad()
    _give(mine, g)
    opt.step()
    coef = opt._norm_result.view(torch.float32)[3].clone()
    assert 0 < float(coef) < 1
    for i in WITH_GRAD:
        theirs[i].grad = torch.mul(torch.from_numpy(g[i]).to(cuda), coef)
    top.step()
    torch.cuda.synchronize()
    worst, same = 0.0, 0
    for i in WITH_GRAD:
        p0 = _init(i).double().numpy()
        gs = theirs[i].grad.double().cpu().numpy()
        sc = ac.scalars(1, LR, WD[ref.GROUP_OF[i]], 0.9)
        r64 = ac.reference(p0, gs, np.zeros_like(p0), np.zeros_like(p0), sc)
        b2 = float(np.float32(sc["beta2"]))
        update = np.abs(r64["p"] - p0 * (1 - float(np.float32(LR)) * float(np.float32(sc["weight_decay"]))))
        bound = 2 * r64["bp"] + 0.5 * ac.U * b2 / (1 - b2) * update
        err = (mine[i].detach() - theirs[i].detach()).abs().double().cpu().numpy()
        assert (err <= bound).all(), (i, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
        same += int(torch.equal(mine[i], theirs[i]))
    assert torch.equal(mine[NO_GRAD], theirs[NO_GRAD])
    with capsys.disabled():
        print("\n[clipped FusedAdamW vs torch.optim.AdamW on the device] worst |diff| / bound %.3f, %d of %d tensors "
              "bit-equal" % (worst, same, len(WITH_GRAD)))


# ====================================================================================================== the EMA kernel
@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_ema_equals_torch_lerp_step_by_step(cuda, kind, shift):
    a, ema_ref = _clipped_run(cuda, kind, shift, 0.05, ema=True)
    for i in range(len(SIZES)):
        assert ref.torch_bits_equal(a.view("e", i), ema_ref[i]), (kind, shift, i)
    assert ref.torch_bits_equal(a.view("e", NO_GRAD), a.view("p", NO_GRAD))        # no gradient: ema == p, both untouched
    assert not torch.equal(a.view("e", 7), a.view("p", 7))


# ====================================================================================================== the optimizers
def _init(i):
    return torch.randn(SIZES[i], generator=torch.Generator().manual_seed(400 + i))


def _params(cuda):
    return [torch.nn.Parameter(_init(i).to(cuda)) for i in range(len(SIZES))]


def _groups(params):
    return [{"params": [p for p, gi in zip(params, ref.GROUP_OF) if gi == 0]},
            {"params": [p for p, gi in zip(params, ref.GROUP_OF) if gi == 1], "weight_decay": WD[1]}]


def _give(params, grads):
    """Gradients handed over the way the backward kernels do: into the arena's view (tests/_adamw_cases.Run.give)."""
    from dcfp_amd import arena
    for i in WITH_GRAD:
        p = params[i]
        t, token = arena.grad_target(p)
        t.copy_(torch.from_numpy(grads[i]).to(p.device))
        out = arena.grad_commit(p, t, token)
        if out is not None:
            p.grad = out if p.grad is None else p.grad + out


def _make(kind, params, **kw):
    from dcfp_amd import optimizer as om
    if kind == "sgd":
        return om.FusedSGD(_groups(params), lr=LR, momentum=MOMENTUM, weight_decay=WD[0], **kw)
    return om.FusedAdamW(_groups(params), lr=LR, weight_decay=WD[0], **kw)


@pytest.fixture
def calls(monkeypatch):
    """Counts the calls of every optimizer entry point."""
    from dcfp_amd import _lib
    L = _lib.lib()
    seen = []
    for name in ("dcfp_grad_norm_f32", "dcfp_sgd_momentum_ex_f32", "dcfp_adamw_ex_f32", "dcfp_sgd_momentum_f32",
                 "dcfp_adamw_f32"):
        def counted(*a, _real=getattr(L, name), _name=name):
            seen.append(_name)
            return _real(*a)
        monkeypatch.setattr(L, name, counted)
    return seen


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_optimizer_launches_tables_norm_and_raw_gradients(cuda, calls, kind):
    """Steady state: one grad-norm call (its two launches) and one step launch per non-empty group, the plain entry points
    never; the tables stop being rebuilt after the first step; grad_norm() is the norm BEFORE clipping over exactly the
    parameters that have a gradient; p.grad stays unscaled; the parameter without gradient keeps ema == p."""
    params = _params(cuda)
    opt = _make(kind, params, max_grad_norm=0.05, ema_decay=DECAY)
    p_nograd = params[NO_GRAD].detach().clone()
    for it in range(3):
        opt.zero_grad()
        g = _grads("randn", it, scale=3.0)
        _give(params, g)
        opt.arena().grad_views[params[NO_GRAD]._dcfp_slot.index].fill_(1e30)       # stale values in its arena slot
        del calls[:]
        opt.step()
        step_name = "dcfp_sgd_momentum_ex_f32" if kind == "sgd" else "dcfp_adamw_ex_f32"
        assert sorted(calls) == sorted(["dcfp_grad_norm_f32", step_name, step_name]), calls
        assert calls[0] == "dcfp_grad_norm_f32"
        if it == 0:
            rebuilds = opt.table_rebuilds
            assert rebuilds == 3                                    # the norm table and one table per group
        assert opt.table_rebuilds == rebuilds
        want = ref.norm32(ref.sqnorm64([g[i] for i in WITH_GRAD])[0])
        got = np.float32(float(opt.grad_norm()))
        assert opt.grad_norm().is_cuda and abs(float(got) - float(want)) <= float(np.spacing(want))
        for i in WITH_GRAD:
            assert np.array_equal(params[i].grad.cpu().numpy().view(np.int32), g[i].view(np.int32)), "p.grad was scaled"
        assert params[NO_GRAD].grad is None
    pairs = opt.grad_sqnorms()
    assert [id(p) for p, _ in pairs] == [id(p) for grp in opt.param_groups for p in grp["params"] if p.grad is not None]
    assert abs(sum(float(s) for _, s in pairs) - float(opt._norm_result[0])) <= 1e-12 * float(opt._norm_result[0])
    ar = opt.arena()
    assert set(ar.state_buffers) == ({"momentum", "ema"} if kind == "sgd" else {"exp_avg", "exp_avg_sq", "ema"})
    assert ref.torch_bits_equal(params[NO_GRAD].detach(), p_nograd)
    assert ref.torch_bits_equal(opt.state[params[NO_GRAD]]["ema"], p_nograd)
    assert not torch.equal(opt.state[params[7]]["ema"], params[7].detach())
    # the digests of a state file walk arena.state_buffers: the EMA arena is one of them
    from dcfp_amd import train_state
    assert "ema" in train_state.digest_buffers(opt, None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_optimizer_equals_the_plain_optimizer_on_scaled_gradients(cuda, kind):
    """FusedSGD / FusedAdamW with max_grad_norm and ema_decay against the same optimizer without them, stepped on
    torch.mul(g, coef): parameters and state bit for bit (the EMA changes nothing it does not own)."""
    mine, plain = _params(cuda), _params(cuda)
    opt, base = _make(kind, mine, max_grad_norm=0.05, ema_decay=DECAY), _make(kind, plain)
    for it in range(3):
        g = _grads("randn", it, scale=3.0)
        opt.zero_grad()
        base.zero_grad()
        _give(mine, g)
        opt.step()
        coef = opt._norm_result.view(torch.float32)[3]
        assert 0 < float(coef) < 1
        _give(plain, [torch.mul(torch.from_numpy(a).to(cuda), coef).cpu().numpy() for a in g])
        base.step()
    keys = ["momentum_buffer"] if kind == "sgd" else ["exp_avg", "exp_avg_sq"]
    for i, (p, q) in enumerate(zip(mine, plain)):
        assert ref.torch_bits_equal(p.detach(), q.detach()), (kind, i)
        for k in keys:
            assert ref.torch_bits_equal(opt.state[p][k], base.state[q][k]), (kind, i, k)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_state_dict_round_trip_continues_with_the_same_bits(cuda, kind):
    a = _params(cuda)
    oa = _make(kind, a, max_grad_norm=0.05, ema_decay=DECAY)
    for it in range(2):
        oa.zero_grad()
        _give(a, _grads("randn", it, scale=3.0))
        oa.step()
    sd = oa.state_dict()
    assert all("ema" in st for st in sd["state"].values())
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ob = _make(kind, b, max_grad_norm=0.05, ema_decay=DECAY)
    ob.load_state_dict({"state": {k: {n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.items()}
                                  for k, st in sd["state"].items()}, "param_groups": sd["param_groups"]})
    for o, ps in ((oa, a), (ob, b)):
        o.zero_grad()
        _give(ps, _grads("randn", 2, scale=3.0))
        o.step()
    for i, (p, q) in enumerate(zip(a, b)):
        assert ref.torch_bits_equal(p.detach(), q.detach()), (kind, i)
        for k in oa.state[p]:
            if torch.is_tensor(oa.state[p][k]):
                assert ref.torch_bits_equal(oa.state[p][k], ob.state[q][k].to(oa.state[p][k].device)), (kind, i, k)
    assert ref.torch_bits_equal(oa.grad_norm(), ob.grad_norm())
    torch.cuda.synchronize()


def test_mixed_parameters_with_max_grad_norm_are_refused(cuda):
    from dcfp_amd.optimizer import FusedAdamW
    on, off = torch.nn.Parameter(torch.randn(5, device=cuda)), torch.nn.Parameter(torch.randn(5))
    opt = FusedAdamW([on, off], lr=0.1, max_grad_norm=1.0)
    on.grad, off.grad = torch.ones(5, device=cuda), torch.ones(5)
    with pytest.raises(NotImplementedError, match="mix"):
        opt.step()


def test_ema_weights_swaps_and_a_block_runs_on_the_average(cuda):
    """One Bottleneck at 2x64x16x16 (the pattern of test_fused_adamw_step_refreshes_the_kept_weight_copies): inside
    ema_weights() the parameters hold the average and the forward equals that of a cold module loaded with
    ema_state_dict; on exit parameters and average are back bit for bit; step() inside raises."""
    from dcfp_amd.networks.backbone.resnet import Bottleneck
    from dcfp_amd.optimizer import FusedSGD
    torch.manual_seed(5)
    blk = Bottleneck(64, 16).to(cuda).train()
    x = torch.randn(2, 64, 16, 16, device=cuda, requires_grad=True)
    opt = FusedSGD(blk.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4, max_grad_norm=0.5, ema_decay=DECAY)
    for _ in range(2):
        opt.zero_grad()
        blk(x).square().mean().backward()
        opt.step()
    esd = opt.ema_state_dict(blk)
    assert list(esd) == list(blk.state_dict())
    weights = [p.detach().clone() for p in blk.parameters()]
    emas = [opt.state[p]["ema"].detach().clone() for p in blk.parameters()]
    assert any(not torch.equal(w, e) for w, e in zip(weights, emas))
    y_live = blk(x)
    with opt.ema_weights():
        for p, e in zip(blk.parameters(), emas):
            assert ref.torch_bits_equal(p.detach(), e)
        y_ema = blk(x)
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
    for p, w, e in zip(blk.parameters(), weights, emas):
        assert ref.torch_bits_equal(p.detach(), w) and ref.torch_bits_equal(opt.state[p]["ema"], e)
    cold = Bottleneck(64, 16).to(cuda).train()
    cold.load_state_dict(esd)
    y_cold = cold(x)
    assert torch.equal(y_ema, y_cold) and not torch.equal(y_ema, y_live)
    assert torch.equal(blk(x), y_live)                               # ... and the live weights' copies are back
    torch.cuda.synchronize()


# ====================================================================================================== the driver
BB = '{"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128, "pretrained": false}'
DRIVER = ["--model", "deeplabv3", "--backbone", "resnet50", "--backbone-para", BB, "--input-size", "65,65",
          "--batch-size", "2", "--deepsup", "True", "--log-digest", "1", "--optim", "adamw", "--learning-rate", "1e-3",
          "--clip-grad-norm", "0.5", "--ema-decay", "0.9", "--save-steps", "2", "--save-pred-every", "2",
          "--num-steps", "4", "--state-every", "2", "--keep-states", "100"]


def _train(argv):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    train = importlib.import_module("train")
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        train.main(argv)
    return out.getvalue().splitlines()


def test_driver_continues_bit_identically_with_both_flags(cuda, tmp_path):
    """The smallest model and size of tests/test_train_state_gpu.py, 4 steps straight against 2 steps + `-c`: final
    weights, EMA checkpoint, optimizer state and the printed digests are equal bit for bit; the log carries gnorm=."""
    import test_train_state_gpu as ts
    da, db = str(tmp_path / "A"), str(tmp_path / "B")
    la = _train(DRIVER + ["--snapshot-dir", da])
    lb = _train(DRIVER + ["--snapshot-dir", db, "--continue", os.path.join(da, "train_state_2.pth")])
    iters = [l for l in la if l.startswith("Iters")]
    assert len(iters) == 4 and all(" gnorm=" in l and math.isfinite(float(l.split("gnorm=")[1])) for l in iters)
    assert ts.digest_lines("\n".join(lb)) == ts.digest_lines("\n".join(la))[2:]
    assert [l for l in lb if l.startswith("Iters")] == iters[2:]
    for name in ("CS_scenes_4.pth", "CS_scenes_4_ema.pth", "train_state_4.pth"):
        a, b = ts.load(os.path.join(da, name)), ts.load(os.path.join(db, name))
        if name.startswith("train_state"):
            assert {"flat_param", "ema", "exp_avg", "exp_avg_sq"} <= set(a["digests"])
            assert a["fingerprint"]["clip_grad_norm"] == 0.5 and a["fingerprint"]["ema_decay"] == 0.9
            assert all("ema" in st for st in a["optimizer"]["state"].values())
            for part in ("model", "optimizer", "scorer", "ranks", "digests", "fingerprint"):
                assert not ts.differences(a[part], b[part], part), (name, part)
        else:
            assert not ts.differences(a, b), name
    w, e = ts.load(os.path.join(da, "CS_scenes_4.pth")), ts.load(os.path.join(da, "CS_scenes_4_ema.pth"))
    assert list(w) == list(e) and any(not torch.equal(w[k], e[k]) for k in w)
    assert os.path.exists(os.path.join(da, "CS_scenes_2_ema.pth"))
    with pytest.raises(ValueError, match="ema_decay"):               # a file written with EMA refuses a run without it
        argv = [a for a in DRIVER if a not in ("--ema-decay", "0.9")]
        _train(argv + ["--snapshot-dir", str(tmp_path / "X"), "--continue", os.path.join(da, "train_state_2.pth")])


def _ddp_child():
    """Two steps of DeepLabv3-R50 2x3x129x257 (the small case of tests/test_ddp_gpu.py) with clipping and EMA, plain and
    through Engine.data_parallel on a world-size-1 group: parameters, EMA and grad_norm() bit for bit."""
    sys.path.insert(0, ROOT)
    import argparse
    import torch.distributed as dist
    from dcfp_amd import networks, optimizer as opt
    from dcfp_amd.engine import Engine, DataParallel
    from dcfp_amd.loss.criterion import build_criterions
    from oracle import fill

    class DS:
        ignore_label = 255; num_classes = 19; class_weights = None

    class A:
        no_decay = "bn"; optim = "sgd"; momentum = 0.9; learning_rate = 1e-3; weight_decay = 5e-4
        clip_grad_norm = 0.5; ema_decay = 0.9
    dev = torch.device("cuda:0")
    bb = {"os": 8, "mg_unit": [1, 2, 4], "inplanes": 128, "pretrained": False}
    x, lab = fill.closed_form_input(2, 129, 257).to(dev), fill.closed_form_labels(2, 129, 257).to(dev)

    def run(ddp):
        torch.manual_seed(12345)
        m = networks.deeplabv3.Seg_Model(backbone="resnet50", backbone_para=dict(bb), num_classes=19, align_corner=True,
                                         criterion=build_criterions("ce", DS(), {"ds_weight": 0.4}), deepsup=True)
        m.load_state_dict(fill.closed_form_state(m.state_dict()))
        m.conv_deepsup[3].p = 0.0
        m = m.to(dev).train()
        optimizer = opt.build_optimizer(A, m)
        optimizer.zero_grad()
        model = m
        if ddp:
            sys.argv = ["x"]
            eng = Engine(custom_parser=argparse.ArgumentParser())
            eng.distributed = True
            model = eng.data_parallel(m)
            assert isinstance(model, DataParallel)
        norms = []
        for it in range(2):
            optimizer.zero_grad()
            model(x, lab, deepsup=True)["loss"].backward()
            optimizer.step()
            norms.append(optimizer.grad_norm().clone())
        torch.cuda.synchronize()
        out = {k: p.detach().clone() for k, p in m.named_parameters()}
        out.update({"ema." + k: v for k, v in optimizer.ema_state_dict(m).items()})
        launched = model.reducer.launched if ddp else None
        return out, torch.stack(norms), launched

    plain = run(False)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", DCFP_FORCE_SYNCBN="1")
    dist.init_process_group("nccl", rank=0, world_size=1)
    ddp = run(True)
    dist.destroy_process_group()
    print("CLIP_DDP_RESULT " + json.dumps({
        "diff": [k for k in plain[0] if not torch.equal(plain[0][k], ddp[0][k])], "n": len(plain[0]),
        "norm_equal": bool((plain[1].view(torch.int32) == ddp[1].view(torch.int32)).all()),
        "norms": plain[1].tolist(), "launched": ddp[2]}))


def test_data_parallel_wrapper_world_size_1_is_bit_identical(cuda):
    env = dict(os.environ, DCFP_FANIN_BN_SUMS="2")                   # (as tests/test_ddp_gpu.py: the same bn3 sums both ways)
    env.pop("DCFP_FORCE_SYNCBN", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ddp-child"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("CLIP_DDP_RESULT ")][-1][len("CLIP_DDP_RESULT "):])
    assert rec["diff"] == [] and rec["n"] > 300, rec["diff"][:8]
    assert rec["norm_equal"] and all(math.isfinite(v) and v > 0 for v in rec["norms"]), rec["norms"]
    assert rec["launched"] == 3


if __name__ == "__main__" and "--ddp-child" in sys.argv:
    _ddp_child()
