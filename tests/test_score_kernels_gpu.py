"""GPU: the kernels of csrc/score.hip, each through its C entry point.

Gate kernels (Taylor score of the BN gate, the slimming L1 term): equal bit for bit to a numpy float32 restatement done
one operation at a time, over three consecutive steps.  filter_reduce and fpgm: planted cases whose result is exact
(one non-zero per row at a chosen column; equal rows) - what catches a dropped tail or chunk edge, which no tolerance
does at K = 18432 - and random cases against fp64 by the rule of tests/_kd_ref.py: distance to fp64, norm-relative per
tensor, at most max(CE_FLOOR, 3 x the distance of the same formula in fp32 on the CPU).  Two runs leave the same bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kd_ref as kr  # noqa: E402

from dcfp_amd import _lib  # noqa: E402
from dcfp_amd.pruners import baseline_pruner as bp  # noqa: E402

pytestmark = pytest.mark.gpu

GATE_TABLES = {"small": (1, 3, 64), "large": (64, 257, 2048), "zero_grad": (257, 2048, 3)}
FILTER_CASES = [(1, 1), (5, 3), (64, 27), (3, 64), (3, 65), (7, 576), (2, 2304), (2, 4611), (1, 18432)]
OFFSET_CASE = (2, 4611)                    # this one is a view that starts at float 1 of a larger buffer
FPGM_CASES = [(1, 9), (2, 1), (17, 27), (64, 64), (130, 577), (64, 2304)]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------ gate kernels
def gate_table(layers, dev):
    entries = (_lib.GateEntry * len(layers))()
    for e, l in zip(entries, layers):
        e.gamma, e.beta, e.ggrad, e.bgrad = (l[k].data_ptr() for k in ("gamma", "beta", "ggrad", "bgrad"))
        e.score, e.n = l["score"].data_ptr(), l["gamma"].numel()
    return torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8).to(dev)


def gate_layers(sizes, seed, dev, zero_grad_layer=None):
    g = torch.Generator().manual_seed(seed)
    layers = []
    for i, n in enumerate(sizes):
        l = {k: torch.randn(n, generator=g).to(dev) for k in ("gamma", "beta", "ggrad", "bgrad")}
        if i == zero_grad_layer:
            l["ggrad"].zero_(), l["bgrad"].zero_()
        l["score"] = torch.zeros(n, device=dev)
        layers.append(l)
    return layers


@pytest.mark.parametrize("name", list(GATE_TABLES))
def test_gate_taylor_three_steps_bit_exact(cuda, name):
    sizes = GATE_TABLES[name]
    zero = 1 if name == "zero_grad" else None
    layers = gate_layers(sizes, 100 + len(name), cuda, zero)
    table = gate_table(layers, cuda)
    want = [np.zeros(n, dtype=np.float32) for n in sizes]
    g = torch.Generator().manual_seed(5)
    for step in range(3):
        for i, l in enumerate(layers):
            if step > 0 and i != zero:                 # new gradients at the same addresses, as a training step leaves them
                l["ggrad"].copy_(torch.randn(l["ggrad"].numel(), generator=g))
                l["bgrad"].copy_(torch.randn(l["bgrad"].numel(), generator=g))
            ga, be, gg, bg = (l[k].cpu().numpy() for k in ("gamma", "beta", "ggrad", "bgrad"))
            a = ga * gg                                 # float32 arrays: every operation rounds once
            b = be * bg
            t = a + b
            want[i] = want[i] + t * t
        _lib.check(_lib.lib().dcfp_gate_taylor_f32(C.c_void_p(table.data_ptr()), len(layers), stream()), "gate_taylor")
        for i, l in enumerate(layers):
            assert want[i].dtype == np.float32
            assert np.array_equal(l["score"].cpu().numpy().view(np.int32), want[i].view(np.int32)), (name, step, i)
    if zero is not None:
        assert bits(layers[zero]["score"]).eq(0).all()          # exactly +0 after three steps
    assert all(float(l["score"].min()) >= 0 for l in layers)


def test_gate_l1reg_bit_exact_and_zero_gamma_untouched(cuda):
    sizes = (1, 3, 64, 257, 2048)
    lam = 1e-4
    layers = gate_layers(sizes, 9, cuda)
    for l in layers:
        n = l["gamma"].numel()
        l["gamma"][::3] = 0.0                                   # sign(0) = 0 ...
        if n > 6:
            l["gamma"][6] = -0.0
            l["ggrad"][6] = -0.0                                # ... and the gradient keeps its bits, a -0 included
    before = [l["ggrad"].clone() for l in layers]
    gamma_before = [l["gamma"].clone() for l in layers]
    table = gate_table(layers, cuda)
    for step in range(3):
        _lib.check(_lib.lib().dcfp_gate_l1reg_f32(C.c_void_p(table.data_ptr()), len(layers), lam, stream()), "gate_l1reg")
    for l, g0, w0 in zip(layers, before, gamma_before):
        ga, want = l["gamma"].cpu().numpy(), g0.cpu().numpy()
        for step in range(3):
            p = np.float32(lam) * np.sign(ga)                   # float32: one rounding
            want = np.where(ga != 0, want + p, want)
        assert np.array_equal(l["ggrad"].cpu().numpy().view(np.int32), want.view(np.int32))
        zero = (w0 == 0).cpu()
        assert zero.any() and torch.equal(bits(l["ggrad"])[zero], bits(g0)[zero])
        assert torch.equal(bits(l["gamma"]), bits(w0)) and bits(l["score"]).eq(0).all()


def test_entry_points_with_nothing_to_do(cuda):
    L = _lib.lib()
    probe = torch.full((8,), 3.0, device=cuda)
    assert L.dcfp_gate_taylor_f32(None, 0, stream()) == 0 and L.dcfp_gate_l1reg_f32(None, 0, 1e-4, stream()) == 0
    assert L.dcfp_filter_reduce_f32(None, 0, 0, _lib.FILTER_ABS_SUM, stream()) == 0
    assert L.dcfp_fpgm_f32(None, 0, 0, None, 0, stream()) == 0
    bp.filter_reduce(*bp.filter_reduce_table([]), _lib.FILTER_L2)
    bp.fpgm(*bp.fpgm_table([]))
    torch.cuda.synchronize()
    assert bool((probe == 3.0).all())


# ----------------------------------------------------------------------------------------------------- filter_reduce
def place(mats, dev):
    """The matrices on the device, each a tensor of its own; OFFSET_CASE as a view at float offset 1 of a larger one."""
    out = []
    for m in mats:
        if tuple(m.shape) == OFFSET_CASE:
            big = torch.full((m.numel() + 5,), float("nan"), device=dev)
            big[1:1 + m.numel()] = m.reshape(-1).to(dev)
            v = big[1:1 + m.numel()].view(m.shape)
            assert v.data_ptr() % 16 == 4 and v.is_contiguous()
            out.append(v)
        else:
            out.append(m.to(dev))
    return out


def run_filter(ws, gs, op, outs):
    items = [(w, g, o) for w, g, o in zip(ws, gs if gs is not None else [None] * len(ws), outs)]
    table = bp.filter_reduce_table(items)
    assert table[1] == len(ws)
    bp.filter_reduce(*table, op)
    return table


@pytest.mark.parametrize("last_column", [False, True])
def test_filter_reduce_planted_exact(cuda, last_column):
    g = torch.Generator().manual_seed(3)
    ws, gs, vals, gvals = [], [], [], []
    for rows, K in FILTER_CASES:
        w = torch.zeros(rows, K)
        gr = torch.randn(rows, K, generator=g)                  # anything: it meets zeros everywhere but one column
        r = torch.arange(rows)
        col = torch.full((rows,), K - 1) if last_column else (r * 97) % K
        v = torch.tensor([(-1.0) ** c * 2.0 ** ((c % 5) - 2) for c in range(rows)])
        gv = torch.tensor([2.0 ** ((c % 3) + 1) for c in range(rows)])
        w[r, col] = v
        gr[r, col] = gv
        ws.append(w), gs.append(gr), vals.append(v), gvals.append(gv)
    dws, dgs = place(ws, cuda), place(gs, cuda)
    for op in (_lib.FILTER_ABS_SUM, _lib.FILTER_L2):
        outs = [torch.full((w.shape[0],), -7.0, device=cuda) for w in ws]
        run_filter(dws, None, op, outs)
        for (rows, K), o, v in zip(FILTER_CASES, outs, vals):
            assert torch.equal(o.cpu(), v.abs()), (op, rows, K, last_column)
    outs = [torch.zeros(w.shape[0], device=cuda) for w in ws]
    table = run_filter(dws, dgs, _lib.FILTER_DOT_SQ_ACC, outs)
    bp.filter_reduce(*table, _lib.FILTER_DOT_SQ_ACC)            # the second step of an accumulation
    for (rows, K), o, v, gv in zip(FILTER_CASES, outs, vals, gvals):
        assert torch.equal(o.cpu(), 2.0 * (v * gv) ** 2), (rows, K, last_column)


def filter_random_inputs():
    g = torch.Generator().manual_seed(17)
    ws = [torch.randn(rows, K, generator=g) for rows, K in FILTER_CASES]
    # g = a w + noise: the dot products stay far from zero, so their fp32 evaluation on the CPU stays a small yardstick
    gs = [[w * a + 0.1 * torch.randn(w.shape, generator=g) for w in ws] for a in (0.5, -0.25)]
    return ws, gs


def filter_formula(w, g1, g2, dtype):
    w, g1, g2 = w.to(dtype), g1.to(dtype), g2.to(dtype)
    return {"abs_sum": w.abs().sum(1), "l2": (w * w).sum(1).sqrt(),
            "dot_sq_acc": (w * g1).sum(1) ** 2 + (w * g2).sum(1) ** 2}


def test_filter_reduce_random_against_fp64_and_repeatable(cuda):
    ws, (g1s, g2s) = filter_random_inputs()
    dws, dg1, dg2 = place(ws, cuda), place(g1s, cuda), place(g2s, cuda)
    runs = []
    for rep in range(2):
        got = {}
        for what, op in (("abs_sum", _lib.FILTER_ABS_SUM), ("l2", _lib.FILTER_L2)):
            got[what] = [torch.full((w.shape[0],), float("nan"), device=cuda) for w in ws]
            run_filter(dws, None, op, got[what])
        got["dot_sq_acc"] = [torch.zeros(w.shape[0], device=cuda) for w in ws]
        run_filter(dws, dg1, _lib.FILTER_DOT_SQ_ACC, got["dot_sq_acc"])
        run_filter(dws, dg2, _lib.FILTER_DOT_SQ_ACC, got["dot_sq_acc"])
        runs.append({k: [o.cpu() for o in v] for k, v in got.items()})
    for i, (rows, K) in enumerate(FILTER_CASES):
        ref64 = filter_formula(ws[i], g1s[i], g2s[i], torch.float64)
        ref32 = filter_formula(ws[i], g1s[i], g2s[i], torch.float32)
        for what in ("abs_sum", "l2", "dot_sq_acc"):
            assert torch.equal(bits(runs[0][what][i]), bits(runs[1][what][i])), (what, rows, K)
            kr.held("filter_reduce", f"{rows}x{K}", what, kr.nrel(runs[0][what][i], ref64[what]),
                    kr.nrel(ref32[what], ref64[what]), kr.CE_FLOOR)


def test_filter_reduce_wrapper_refuses_what_the_kernel_cannot_read(cuda):
    w = torch.randn(4, 6, device=cuda)
    with pytest.raises(ValueError):
        bp.filter_reduce_table([(w, None, torch.zeros(5, device=cuda))])          # 24 weights are not 5 rows
    with pytest.raises(RuntimeError):
        bp.filter_reduce_table([(w.t(), None, torch.zeros(6, device=cuda))])      # not contiguous
    with pytest.raises(RuntimeError):
        bp.filter_reduce_table([(w.cpu(), None, torch.zeros(4, device=cuda))])
    with pytest.raises(ValueError):
        bp.filter_reduce_table([(w, torch.zeros(4, 5, device=cuda), torch.zeros(4, device=cuda))])


# -------------------------------------------------------------------------------------------------------------- fpgm
def fpgm_formula(w, dtype):
    w = w.to(dtype).reshape(w.shape[0], -1)
    return torch.cdist(w, w, compute_mode="donot_use_mm_for_euclid_dist").sum(1)      # distances from differences


def test_fpgm_against_fp64_duplicates_and_repeatable(cuda):
    g = torch.Generator().manual_seed(23)
    ws = [torch.randn(Cc, K, generator=g) for Cc, K in FPGM_CASES]
    mixed = torch.randn(6, 37, generator=g)
    mixed[4] = mixed[3]                                          # two identical rows ...
    mixed[5] = mixed[0]                                          # ... and a third row equal to the first
    same = torch.randn(1, 33, generator=g).repeat(70, 1)        # all rows equal, over a tile edge: every distance is 0
    pair = torch.randn(1, 2304, generator=g).repeat(2, 1)
    trio = torch.randn(3, 577, generator=g)
    trio[2] = trio[0]                                            # rows a, b, a
    ws += [trio, mixed, same, pair]
    dws = [w.to(cuda) for w in ws]
    runs = []
    for rep in range(2):
        outs = [torch.full((w.shape[0],), float("nan"), device=cuda) for w in ws]
        bp.fpgm(*bp.fpgm_table(list(zip(dws, outs))))
        runs.append([o.cpu() for o in outs])
    for w, a, b in zip(ws, runs[0], runs[1]):
        case = "%dx%d" % tuple(w.shape)
        assert torch.equal(bits(a), bits(b)), case
        assert bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0, case
        kr.held("fpgm", case, "score", kr.nrel(a, fpgm_formula(w, torch.float64)),
                kr.nrel(fpgm_formula(w, torch.float32), fpgm_formula(w, torch.float64)), kr.CE_FLOOR)
    assert bits(runs[0][0]).eq(0).all()                          # C = 1
    assert bits(runs[0][-2]).eq(0).all() and bits(runs[0][-1]).eq(0).all()
    # equal rows are at distance exactly 0 from each other and at the same distances from the rest: the same bits as
    # scores; in rows (a, b, a) the score of a is d(a, b) + 0 and that of b is d + d, twice it exactly
    m, t = runs[0][-3], runs[0][-4]
    assert torch.equal(bits(m[3]), bits(m[4])) and torch.equal(bits(m[5]), bits(m[0]))
    assert torch.equal(bits(t[2]), bits(t[0])) and float(t[0]) > 0 and torch.equal(bits(t[1]), bits(2.0 * t[0]))
