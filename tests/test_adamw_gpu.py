"""dcfp_adamw_f32 through the C ABI against fp64 per element, FusedAdamW's state transitions against torch.optim.AdamW
(the scripts of test_step_kernels_gpu.py), and FusedAdamW in a training step: kept weight copies, a whole model."""
import ctypes as C
import functools
import weakref

import numpy as np
import pytest
import torch

import _adamw_cases as ac

pytestmark = pytest.mark.gpu

ALIGNED = dict(p=0, g=0, m=0, v=0)            # floats by which each operand's buffer is shifted off its 256-byte base
SHIFTED = dict(p=1, g=1, m=1, v=1)            # residue-3 tensors become the aligned ones, residue-0 ones unaligned
MIXED = dict(p=0, g=1, m=0, v=2)              # only some pointers of an entry are ever aligned: all scalar path


def _launch(cuda, case, shifts):
    """One launch over the hand-built table; returns the fp32 results at the live elements after checking that the
    sentinels in every gap (and in front of / behind the shifted buffers) and the gradients are bit-intact."""
    from dcfp_amd import _lib
    step, lr, wd, beta1, state = ac.KERNEL_CASES[case]
    host, live = ac.kernel_inputs(state)
    sizes, offs, total = ac.layout()
    first, chunks = ac.chunks_of(sizes)
    assert chunks == len(sizes) + 2 * (1 + 1 + 4)                  # one chunk each; 16385 and 2*16384 two, 70001 five
    PAD = 8
    dev, before = {}, {}
    for k in "pgmv":
        buf = np.full(total + PAD, ac.SENT, np.float32)
        buf[shifts[k]:shifts[k] + total] = host[k]
        before[k] = buf
        dev[k] = torch.from_numpy(buf.copy()).to(cuda)
        assert dev[k].data_ptr() % 256 == 0
    entries = (_lib.AdamEntry * len(sizes))()
    aligned = 0
    for e, n, o, fc in zip(entries, sizes, offs, first):
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = (dev[k].data_ptr() + 4 * (o + shifts[k]) for k in "pgmv")
        e.n, e.first_chunk = n, fc
        aligned += all((o + shifts[k]) % 4 == 0 for k in "pgmv")
    table = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8).to(cuda)
    sc = ac.scalars(step, lr, wd, beta1)
    _lib.check(_lib.lib().dcfp_adamw_f32(C.c_void_p(table.data_ptr()), len(sizes), chunks, sc["lr"], sc["beta1"], sc["beta2"],
                                         sc["eps"], sc["weight_decay"], sc["bc1"], sc["bc2_sqrt"],
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "adamw")
    torch.cuda.synchronize()
    out = {}
    for k in "pgmv":
        got = dev[k].cpu().numpy()
        mask = np.zeros(total + PAD, bool)
        mask[shifts[k]:shifts[k] + total] = live
        assert np.array_equal(got[~mask].view(np.int32), before[k][~mask].view(np.int32)), "written past n: " + k
        out[k] = got[mask]
    assert np.array_equal(out["g"].view(np.int32), host["g"][live].view(np.int32)), "the gradient was written"
    return out, aligned


@functools.lru_cache(maxsize=None)
def _reference(case):
    step, lr, wd, beta1, state = ac.KERNEL_CASES[case]
    host, live = ac.kernel_inputs(state)
    return ac.reference(*(host[k][live].astype(np.float64) for k in "pgmv"), ac.scalars(step, lr, wd, beta1))


@pytest.mark.parametrize("case", list(ac.KERNEL_CASES))
def test_adamw_kernel_against_fp64_per_element(cuda, capsys, case):
    """adamw_kernel over a hand-built table on ONE flat buffer per operand, 336 tensors of 1 ... 70001 elements at every
    start residue mod 4 (aligned entries: float4 body + scalar tail; the others: scalar path), against the same lines
    in fp64.  m, v and p per element within twice the first-order roundoff bound derived in _adamw_cases (which
    test_adamw_host_cpu.py shows a numpy fp32 restatement to respect on the same inputs)."""
    step, lr, wd, beta1, state = ac.KERNEL_CASES[case]
    host, live = ac.kernel_inputs(state)
    out, aligned = _launch(cuda, case, ALIGNED)
    assert 0 < aligned < len(ac.layout()[0])                        # both paths ran
    ref = _reference(case)
    worst = ac.worst_ratios(out, ref)
    with capsys.disabled():
        print("\n[adamw kernel %s] worst |err|/bound: m %.3f, v %.3f, p %.3f" % (case, worst["m"], worst["v"], worst["p"]))
    assert max(worst.values()) <= 1.0, worst
    if lr == 0.0:                       # p *= 1 - lr*wd and p -= (lr/bc1)*...: nothing may move, with or without decay
        assert np.array_equal(out["p"].view(np.int32), host["p"][live].view(np.int32))
    else:
        assert not np.array_equal(out["p"], host["p"][live])
    if beta1 == 0.0:
        assert np.array_equal(out["m"].view(np.int32), host["g"][live].view(np.int32))
    if state == "zero":                 # v = (1-beta2) g^2, m = (1-beta1) g: zero exactly where g is
        zero = host["g"][live] == 0
        assert zero.any() and (out["m"][zero] == 0).all() and (out["v"][zero] == 0).all()
        assert np.array_equal(out["p"][zero], (host["p"][live] * np.float32(1 - ac._f(lr) * ac._f(wd)))[zero])


@pytest.mark.parametrize("case", ["step1000", "beta1-0"])
def test_adamw_vector_and_scalar_paths_give_the_same_bits(cuda, case):
    """The same data at three placements: as laid out; every operand shifted by one float (what was aligned is not, and
    the other way round); operands shifted differently (no entry with all four pointers aligned)."""
    base, n_al = _launch(cuda, case, ALIGNED)
    shifted, n_sh = _launch(cuda, case, SHIFTED)
    mixed, n_mx = _launch(cuda, case, MIXED)
    assert n_al > 0 and n_sh > 0 and n_mx == 0
    for k in "pmv":
        assert np.array_equal(base[k].view(np.int32), shifted[k].view(np.int32)), k
        assert np.array_equal(base[k].view(np.int32), mixed[k].view(np.int32)), k
    ref = _reference(case)
    assert max(ac.worst_ratios(mixed, ref).values()) <= 1.0


# ---------------------------------------------------------------------------------------------- FusedAdamW transitions
@pytest.fixture
def launches(monkeypatch):
    """Counts dcfp_adamw_f32 launches as (n_tensors, total_chunks, bias_correction1)."""
    from dcfp_amd import _lib
    L = _lib.lib()
    real = L.dcfp_adamw_f32
    seen = []

    def counted(table, n, chunks, lr, b1, b2, eps, wd, bc1, bc2s, stream):
        seen.append((n, chunks, bc1))
        return real(table, n, chunks, lr, b1, b2, eps, wd, bc1, bc2s, stream)
    monkeypatch.setattr(L, "dcfp_adamw_f32", counted)
    return seen


def _fused(cuda):
    from dcfp_amd.optimizer import FusedAdamW
    return ac.Run(FusedAdamW, cuda, torch.float32)


WORST = {}


def _against_torch(cuda, capsys, label, script):
    """|FusedAdamW - fp64| <= max(3 x |torch.optim.AdamW fp32 on CPU - fp64|, summed roundoff floor) per tensor and step."""
    cpu = torch.device("cpu")
    mine = ac.drive(_fused(cuda), script)
    t64 = ac.drive(ac.Run(torch.optim.AdamW, cpu, torch.float64), script)
    t32 = ac.drive(ac.Run(torch.optim.AdamW, cpu, torch.float32), script)
    worst = 0.0
    for it in range(len(script)):
        for i in range(len(ac.SHAPES)):
            ref = t64.history[it][i]
            err = float((mine.history[it][i].double() - ref).abs().max())
            spread = float((t32.history[it][i].double() - ref).abs().max())
            floor = float(t64.floor[i].max())
            worst = max(worst, err / max(spread, floor / 3, 1e-300))
            assert err <= max(3 * spread, floor), (label, it, i, err, spread, floor)
    assert mine.steps_taken() == t32.steps_taken(), label
    WORST[label] = worst
    with capsys.disabled():
        print("\n[FusedAdamW %s] worst |mine - fp64| / |torch fp32 - fp64| over %d steps x %d tensors: %.2f (bound 3)"
              % (label, len(script), len(ac.SHAPES), worst))
    return mine


def test_fused_adamw_poly_lr_steady_state(cuda, capsys, launches):
    run = _against_torch(cuda, capsys, "poly lr, set_to_none", [{} for _ in range(ac.STEPS)])
    assert run.opt.table_rebuilds == 2                    # one upload per group, however often the lr changes
    assert len(launches) == 2 * ac.STEPS                  # one launch per non-empty group and step
    assert run.opt.arena() is not None and run.opt.arena().has_state("exp_avg_sq")
    st = run.opt.state[run.params[3]]
    assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == ac.STEPS
    assert st["exp_avg"].data_ptr() == run.opt.arena().state_view("exp_avg", run.params[3]._dcfp_slot.index).data_ptr()
    run = _against_torch(cuda, capsys, "poly lr, in-place zero_grad", [{"to_none": False} for _ in range(ac.STEPS)])
    assert run.opt.table_rebuilds == 2


def test_fused_adamw_late_gradient_is_one_more_partition(cuda, capsys, launches):
    """Parameter 2 has no gradient on steps 0-2: from step 3 on its step count lags by three, its bias corrections are
    its own, and group 0 takes two launches - the table of the others is the one already uploaded."""
    script = [{"no_grad": (2,)}, {"no_grad": (2,)}, {"no_grad": (2,)}, {}, {}, {}]
    run = _against_torch(cuda, capsys, "late gradient", script)
    assert torch.equal(run.history[2][2], ac.init_of(2))  # untouched until its first gradient
    per_step = [2, 2, 2, 3, 3, 3]
    assert len(launches) == sum(per_step)
    late = launches[6:][0::3] + launches[6:][1::3]        # group 0's two launches of steps 3, 4, 5
    assert sorted(n for n, _, _ in late) == [1, 1, 1, 4, 4, 4]
    assert {round(bc1, 6) for n, _, bc1 in late if n == 1} == {round(1 - 0.9 ** t, 6) for t in (1, 2, 3)}
    assert run.opt.table_rebuilds == 3
    assert run.steps_taken() == [6.0, 6.0, 3.0, 6.0, 6.0, 6.0, 6.0, 6.0]


def test_fused_adamw_missing_gradients(cuda, capsys):
    """Parameter 6 loses its gradient at step 4: skipped after zero_grad(set_to_none=True), a step on zeros after the
    in-place flavour.  (The arena's in-place zero_grad attaches a zeroed view to EVERY parameter, so a parameter that
    never had a gradient takes steps on zeros there where torch leaves it alone: pinned for FusedSGD, the same here.)"""
    script = [{}, {}, {}, {}, {"no_grad": (6,)}, {}]
    run = _against_torch(cuda, capsys, "missing gradient", script)
    assert run.steps_taken()[6] == 5.0
    _against_torch(cuda, capsys, "missing gradient, in-place zero_grad", [dict(s, to_none=False) for s in script])
    mixed = [dict(s, to_none=bool(it % 2)) for it, s in enumerate(script)]
    _against_torch(cuda, capsys, "missing gradient, both zero_grad flavours", mixed)


def test_fused_adamw_weight_decay_change_keeps_the_tables(cuda, capsys):
    script = [{}, {}, {}, {"before": [("wd", 0, 1e-3), ("wd", 1, 2e-4)]}, {}, {}]
    run = _against_torch(cuda, capsys, "weight decay change", script)
    assert run.opt.table_rebuilds == 2                    # weight decay is a kernel argument
    plain = ac.drive(_fused(cuda), [{} for _ in range(ac.STEPS)])
    assert not torch.equal(run.history[-1][5], plain.history[-1][5])      # group 1 really decayed after the change


def test_fused_adamw_resume_is_bit_identical(cuda, capsys):
    script = [{}, {}, {}, {"before": ["resume"]}, {}, {}]
    resumed = _against_torch(cuda, capsys, "save / resume", script)
    straight = ac.drive(_fused(cuda), [{} for _ in range(ac.STEPS)])
    for it in range(ac.STEPS):
        for i in range(len(ac.SHAPES)):
            assert torch.equal(resumed.history[it][i], straight.history[it][i]), (it, i)


def test_fused_adamw_loading_a_never_stepped_or_partial_state_restarts_from_zero(cuda, capsys):
    """load_state_dict of a state without moments (a checkpoint taken before the first step) after two steps, and of
    one that lacks parameters 1 and 5: the missing moments and step counts restart from zero, as in torch.optim.AdamW -
    not from what the arena's buffers still hold."""
    script = [{}, {}, {"before": ["load_fresh"]}, {}, {}, {}]
    run = _against_torch(cuda, capsys, "never-stepped state loaded after 2 steps", script)
    assert run.steps_taken() == [4.0] * len(ac.SHAPES)
    script = [{}, {}, {"before": ["load_partial"]}, {}, {}, {}]
    run = _against_torch(cuda, capsys, "partial state loaded after 2 steps", script)
    assert run.steps_taken() == [6.0, 4.0, 6.0, 6.0, 6.0, 4.0, 6.0, 6.0]


def test_fused_adamw_parameters_moved_out_of_the_arena_keep_their_state(cuda, capsys):
    script = [{}, {}, {}, {"before": ["move_out"]}, {}, {}]
    moved = _against_torch(cuda, capsys, "parameters moved out of the arena", script)
    straight = ac.drive(_fused(cuda), [{} for _ in range(ac.STEPS)])
    for i in range(len(ac.SHAPES)):
        assert torch.equal(moved.history[-1][i], straight.history[-1][i]), i


def test_fused_adamw_state_loads_into_torch_adamw_and_back(cuda):
    """A GPU checkpoint of FusedAdamW continues in torch.optim.AdamW (on the CPU, within fp32 noise of its own run) and
    torch's checkpoint continues in FusedAdamW with the moments copied into the arena."""
    from dcfp_amd.optimizer import FusedAdamW
    run = ac.drive(_fused(cuda), [{}, {}, {}])
    sd = run.opt.state_dict()
    assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "params"}
    cpu_params = [torch.nn.Parameter(p.detach().cpu().clone()) for p in run.params]
    topt = torch.optim.AdamW([{"params": cpu_params[:5]}, {"params": cpu_params[5:], "weight_decay": 0.0}])
    topt.load_state_dict(sd)
    for i, p in enumerate(cpu_params):
        st = topt.state[p]
        assert float(st["step"]) == 3.0 and st["exp_avg"].device.type == "cpu"
        assert torch.equal(st["exp_avg_sq"], run.opt.state[run.params[i]]["exp_avg_sq"].cpu())
    back = _fused(cuda)
    back.opt.load_state_dict(topt.state_dict())
    back.opt.zero_grad()
    ar = back.opt.arena()
    for i, p in enumerate(back.params):
        st = back.opt.state[p]
        assert st["exp_avg"].data_ptr() == ar.state_view("exp_avg", p._dcfp_slot.index).data_ptr()
        assert torch.equal(st["exp_avg"].cpu(), topt.state[cpu_params[i]]["exp_avg"]) and float(st["step"]) == 3.0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- in a training step
@pytest.fixture
def wp(monkeypatch):
    """The registry of kept weight copies, empty for this test, and a spy on what every conv call is told about its
    buffer (the fixture of test_step_kernels_gpu.py)."""
    from dcfp_amd import ops
    monkeypatch.setattr(ops, "_WP_OWNERS", weakref.WeakSet())
    monkeypatch.setattr(ops, "_WP_TABLE", {"version": 0, "built": -1, "dev": None, "n": 0, "blocks": 0, "entries": []})
    seen = []
    real = ops._conv_workspace

    def spy(w, which, d, variant=""):
        ws, valid = real(w, which, d, variant)
        seen.append((which, variant, valid, ws.data_ptr()))
        return ws, valid
    monkeypatch.setattr(ops, "_conv_workspace", spy)
    return seen


def test_fused_adamw_step_refreshes_the_kept_weight_copies(cuda, wp):
    """One Bottleneck at 2x64x16x16: after FusedAdamW.step() every kept copy is valid for the new epoch (no conv rebuilds
    its own), and the next forward equals that of a cold module loaded with the same state_dict bit for bit."""
    from dcfp_amd.networks.backbone.resnet import Bottleneck
    from dcfp_amd.optimizer import FusedAdamW
    torch.manual_seed(5)
    blk = Bottleneck(64, 16).to(cuda).train()
    x = torch.randn(2, 64, 16, 16, device=cuda, requires_grad=True)
    opt = FusedAdamW(blk.parameters(), lr=1e-2, weight_decay=1e-2)
    opt.zero_grad()
    y0 = blk(x)
    y0.square().mean().backward()
    cold_calls = len(wp)
    assert cold_calls >= 3 and all(v[2] == 0 for v in wp)
    before = [p.detach().clone() for p in blk.parameters()]
    opt.step()
    assert opt.table_rebuilds == 1
    assert all(not torch.equal(p, q) for p, q in zip(blk.parameters(), before))
    y1 = blk(x)
    warm = wp[cold_calls:]
    assert len(warm) >= 3 and all(v[2] == 1 for v in warm), warm
    cold = Bottleneck(64, 16).to(cuda).train()
    cold.load_state_dict(blk.state_dict())
    n = len(wp)
    y2 = cold(x)
    assert all(v[2] == 0 for v in wp[n:])
    assert torch.equal(y1, y2) and not torch.equal(y1, y0)
    torch.cuda.synchronize()


def test_fused_adamw_two_steps_of_a_model(cuda):
    """DeepLabv3-R50 at 2x3x65x65 through build_optimizer(optim='adamw'): two steps, finite losses, every parameter
    moved and finite, one table per group, every parameter's state in the arena."""
    from _model_cases import build_model
    from oracle import fill
    from dcfp_amd import optimizer as om

    class A:
        no_decay = "bn"; optim = "adamw"; betas = "0.9,0.999"; learning_rate = 1e-3; weight_decay = 1e-2; momentum = 0.9
    m = build_model("deeplabv3", "resnet50", True, cuda)
    opt = om.build_optimizer(A, m)
    assert type(opt) is om.FusedAdamW
    x, lab = fill.closed_form_input(2, 65, 65).to(cuda), fill.closed_form_labels(2, 65, 65).to(cuda)
    start = [p.detach().clone() for p in m.parameters()]
    losses = []
    for it in range(2):
        opt.zero_grad()
        loss = m(x, lab, deepsup=True)["loss"]
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(v) for v in losses), losses
    assert losses[1] != losses[0]
    assert opt.table_rebuilds == 2 and all(len(g["params"]) > 0 for g in opt.param_groups)
    ar = opt.arena()
    for p, p0 in zip(m.parameters(), start):
        assert bool(torch.isfinite(p).all()) and not torch.equal(p, p0)
        st = opt.state[p]
        assert float(st["step"]) == 2.0
        assert st["exp_avg_sq"].data_ptr() == ar.state_view("exp_avg_sq", p._dcfp_slot.index).data_ptr()
    # |m^/sqrt(v^)| <= 1 on the first step and <= 1.0014 on the second (Cauchy-Schwarz on the two weighted gradients),
    # decay adds lr*wd*|p| per step: two steps move no element by more than lr*(2.0014 + 0.02|p|) <= 2.01 lr (1 + max|p|)
    worst = max(float((p - p0).abs().max() - 2.01 * 1e-3 * (1 + p0.abs().max())) for p, p0 in zip(m.parameters(), start))
    assert worst <= 0, worst
    torch.cuda.synchronize()
