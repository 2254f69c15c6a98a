"""GPU: every training kernel at the 1-, 2- and 5-channel layers a pruned model is left with, against fp64 ATen on
the CPU (convs, BatchNorm) or on the device (fused nodes), on inputs from seeded generators.

* every row of tests/_narrow_cases.NARROW - one stand-in per (pass, kernel, narrow side) class the slim models of the
  golden prune fixtures reach, proved complete by tests/test_narrow_routing_host_cpu.py: forward (plain, bias,
  statistics epilogue), data gradient (into a NaN-filled buffer, and accumulating), weight and bias gradient.  The route
  is asserted by name first.  Errors are relative L2 PER CHANNEL of the narrow tensor - y and dx per output channel of
  the pass, dw per filter row and per input-channel column - and the worst channel is asserted: a wrong channel of five
  moves a whole-tensor norm by 1 / sqrt(5) of its own error, one of 129 by less than a tenth.
  Bounds: those of tests/test_conv_random_gpu.py - forward 3e-6 * max(1, sqrt(K) / 8), data gradient max(that, 1e-5),
  weight gradient 2e-5 - which were set for whole-tensor norms; a channel above one of them passes if it is within
  3 x ATen's own fp32 error on the SAME channel (F.conv2d / conv2d_input / conv2d_weight in fp32 on the CPU against
  fp64: the `ref_noise` of tests/test_ops_gpu.py), a yardstick measured against the reference, never the kernel.
  The bias gradient: |db_c - sum dy_c| <= 1e-5 * max(|sum dy_c|, ||dy_c||_2) per channel (1e-5 is the bound
  tests/test_conv_random_gpu.py puts on the vector of sums; ||dy_c||_2 is the size such a sum has where it cancels).
  "NARROW_FIG" lines carry, per row and pass, the worst channel's error over the project bound, over the bound it was
  held to, and ATen's fp32 error on that channel.
* the rows whose operands the network keeps row-pitched cannot be written in tests/_wp_cases.py's dense form: their
  kept weight copies are refreshed and replayed here, bit for bit, as tests/test_step_kernels_gpu.py does for the rest.
* BatchNorm (+residual, +ReLU) forward and backward at C = 1, 2, 5 through ops.batch_norm_act and - what a Bottleneck's
  bn3 runs where H*W % 256 == 0 - through the 1-bit ReLU mask of bn_apply_relu_mask, against fp64 F.batch_norm with the
  bounds of tests/test_misc_random_gpu.py::test_random_bn, per channel.
* the fused nodes at the fixtures' widths with tests/_node_ref.py and the bounds of tests/test_fused_nodes_gpu.py:
  two-block Bottleneck chains cut to (c1, 1, cout) / (2, c2, cout) at stride 2 / (c1, 5, cout) at dilation 2, and a
  256-channel chain whose conv1 takes the masked fan-in data gradient with K = 7 and 3; ASPP with branch widths
  [5, 1, 2, 3, 5]; the DeepLabv3+ decoder concat with 2 + 5 channels; pyramid pooling with stage widths [1, 2, 5, 3].
  The only disagreement tolerated is a ReLU mask flip that _node_ref.masks_honest licenses (a pre-activation within
  1e-4 rms of zero); the flips are counted, printed ("NARROW_FLIPS") and held to the share the existing node tests see:
  14 of 56.6 million mask elements, 2.47e-7 (tests/_narrow_cases.py FLIP_RATE; the count of a case must not exceed the
  99.9 % quantile of a Poisson variable of mean FLIP_RATE * elements - 0 below 4000 elements, 6 at 4.7 million).  Measured:
  0 everywhere but the 128 x 192 chains - 1, 2 and 5 flips of 4.2 / 4.7 / 26 million (means 1.0, 1.2 and 6.5: no excess).
  The pyramid-pooling case has no count: its composite, like that of tests/test_psp_gpu.py, applies torch.relu in fp64 -
  the ReLU sits in front of the interpolation, so the concat does not show the kernel's mask - and a flip there would
  show as an error against the bounds, not as a licensed count.
  The weight gradient runs twice: on |x| and dy + 0.5, where every row and column, one-element ones included, is
  well-conditioned, and on the zero-mean x and dy (whole tensor, and every row / column of more than one element).

What would trip (tests/test_narrow_routing_host_cpu.py runs the mutations on CPU results):
* conv tiles - dead rows of an M = 1 tile stored land in the next image's only channel (or past the tensor): dx is
  NaN-filled first and y / dx are judged per channel, so row 0's forward and row 1's data gradient fail; a K tail read
  beyond Cin*k*k unzeroed adds a stray product to every output of the rows with K = 1 ... 81, an error of the size of the
  output against a bound of 3e-6;
* weight-gradient tiles - a dead dy row of the WIDE tile or a dead column of the one-wave tile that leaks is a wrong filter
  row / input-channel column: "wgrad.rows" / "wgrad.cols" judge each of them alone, where the whole-tensor norm of a
  129-row gradient would pass an error of 11 bounds in one row;
* kept copies - the refreshed copy must equal the conv's own byte for byte and nothing may be written past the layout's
  extent (Mpad = 256 rows for M = 1): a refresh that pads differently from the kernel fails torch.equal before any
  tolerance is involved;
* fused nodes - a width-1 concat slice whose base is rounded to 4 floats shifts that slice by up to three pixels: the
  ASPP output's 1e-5 bound and the per-stage comparison of the pyramid slices fail at O(1)."""
import copy
import math
import weakref

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _narrow_cases as nc
import _node_ref as nr

pytestmark = pytest.mark.gpu


def _flip_cap(flipped, total, what):
    """The flips of a case stay at the share the existing node tests see (nc.FLIP_RATE, nc.flip_allowance)."""
    allowed = nc.flip_allowance(total)
    print(f"NARROW_FLIPS {what} flipped={flipped} of {total} ({flipped / max(total, 1):.2e}; at the existing share "
          f"{nc.FLIP_RATE:.2e}: mean {nc.FLIP_RATE * total:.2f}, allowed {allowed})")
    assert flipped <= allowed, (what, flipped, total, allowed)


# ------------------------------------------------------------------ convolutions
_chan, _per_channel = nc.chan_norms, nc.per_channel


def _operand(t, pitch, device):
    """t on the device, dense or as the row-pitched view with a zero tail the network would hand over."""
    from dcfp_amd import ops
    if not pitch:
        return t.to(device)
    v = ops.new_pitched(tuple(t.shape), pitch, device)
    v.copy_(t)
    assert ops._pitch_of(v) == pitch
    return v


class _Ref:
    """fp64 and fp32 ATen results of one case on the CPU."""

    def __init__(self, case, seed):
        N, Cin, H, W, Cout, k, s, p, d = case
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(N, Cin, H, W, generator=g)
        self.w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
        self.b = torch.randn(Cout, generator=g)
        self.cfg = (s, p, d)
        self.y = {dt: F.conv2d(self.x.to(dt), self.w.to(dt), None, s, p, d) for dt in (torch.float64, torch.float32)}
        self.dy = torch.randn(self.y[torch.float64].shape, generator=g)
        self.seed = torch.randn(N, Cin, H, W, generator=g)
        self.dx = {dt: torch.nn.grad.conv2d_input((N, Cin, H, W), self.w.to(dt), self.dy.to(dt), s, p, d)
                   for dt in (torch.float64, torch.float32)}
        # The weight gradient has operands of its own.  With one channel on a side a row or column of dw is ONE element,
        # a sum over the pixels, and its relative error is the sum's condition number sum|t| / |sum t| times the
        # arithmetic's: for zero-mean operands that number is unbounded (4400 on the worst element of row
        # (2, 130, 16, 32, 1, 1, ...), where ATen's own fp32 result is 8e-5 off, four times the bound) and the figure says
        # nothing about the kernel.  |x| - what a conv behind a ReLU reads - and dy + 0.5 keep every element's terms mostly
        # of one sign (condition number of a few), signs still mixed.
        self.xw, self.dyw = self.x.abs(), self.dy + 0.5
        self.dw = {dt: torch.nn.grad.conv2d_weight(self.xw.to(dt), (Cout, Cin, k, k), self.dyw.to(dt), s, p, d)
                   for dt in (torch.float64, torch.float32)}
        # ... and the zero-mean x and dy run as well, so that a fault that depends on a sign cannot hide: the whole tensor
        # within 2e-5, and every row / column of MORE than one element under the same per-channel rule
        self.dw0 = {dt: torch.nn.grad.conv2d_weight(self.x.to(dt), (Cout, Cin, k, k), self.dy.to(dt), s, p, d)
                    for dt in (torch.float64, torch.float32)}


IDS = ["%d-%s" % (i, "x".join(map(str, c))) for i, (c, *_) in enumerate(nc.NARROW)]


@pytest.mark.parametrize("ri", range(len(nc.NARROW)), ids=IDS)
def test_conv_row_per_channel_vs_fp64(cuda, ri):
    from dcfp_amd import ops
    case, fwd, dgrad, wgrad = nc.NARROW[ri]
    N, Cin, H, W, Cout, k, s, p, d = case
    assert nc.routes(case) == (fwd, dgrad, wgrad), (case, nc.routes(case))     # a change of dispatch fails here
    pitch = nc.pitch_of(case)
    assert pitch == nc.NARROW_PITCH.get(case, 0)
    r = _Ref(case, 7000 + ri)
    f64, f32 = torch.float64, torch.float32
    tol = nc.tolerance(case)
    figs = []

    def hold(what, got, ref64, ref32, dim, bound, min_elems=1):
        a, b, e32 = _per_channel(got, ref64, ref32, dim, bound, min_elems)
        figs.append((what, a, b, e32))
        print(f"NARROW_FIG row={ri} case={case} {what} err/bound={a:.3f} err/held={b:.3f} aten32={e32:.2e}")
        return b

    worst = []
    wd = r.w.to(cuda)
    if fwd is not None:
        xd = _operand(r.x, pitch, cuda)
        y = ops.conv2d_fwd(xd, wd, None, s, p, d)
        worst.append(("fwd", hold(f"fwd[{fwd}]", y, r.y[f64], r.y[f32], 1, tol)))
        yb = ops.conv2d_fwd(xd, wd, r.b.to(cuda), s, p, d)
        bb = r.b.view(1, -1, 1, 1)
        worst.append(("fwd+bias", hold("fwd+bias", yb, r.y[f64] + bb.double(), r.y[f32] + bb, 1, tol)))
        ys, st = ops.conv2d_fwd(xd, wd, None, s, p, d, want_stats=True)
        assert torch.equal(ys, y)
        # a narrow Cout leaves no tile with all rows live: the library must decline the epilogue (nc.STATS: who has it)
        assert (st is not None) == (case in nc.STATS), (case, st is None)
        if st is not None:
            m64 = r.y[f64].mean((0, 2, 3)); v64 = r.y[f64].var((0, 2, 3), unbiased=False)
            em = float((st[0].double().cpu() - m64).abs().max()) / max(1.0, float(m64.abs().max()))
            ev = float(((st[1].double().cpu() - v64).abs() / v64).max())
            print(f"NARROW_FIG row={ri} case={case} stats mean_err={em:.2e} var_rel={ev:.2e} (bounds 2e-6, 2e-6)")
            worst.append(("stats.mean", em / 2e-6)); worst.append(("stats.var", ev / 2e-6))
        del xd, y, yb, ys
    if dgrad is not None:
        dyd = _operand(r.dy, pitch, cuda)
        dx = torch.full((N, Cin, H, W), float("nan"), device=cuda)            # every element must be written
        ops.conv2d_dgrad(dyd, wd, (N, Cin, H, W), s, p, d, out=dx, accumulate=False)
        worst.append(("dgrad", hold(f"dgrad[{dgrad}]", dx, r.dx[f64], r.dx[f32], 1, max(tol, 1e-5))))
        dxa = r.seed.to(cuda)
        ops.conv2d_dgrad(dyd, wd, (N, Cin, H, W), s, p, d, out=dxa, accumulate=True)
        worst.append(("dgrad+acc", hold("dgrad+acc", dxa, r.dx[f64] + r.seed.double(), r.dx[f32] + r.seed, 1,
                                        max(tol, 1e-5))))
        del dx, dxa, dyd
    if wgrad is not None:
        xd, dyd = _operand(r.xw, pitch, cuda), _operand(r.dyw, pitch, cuda)
        if pitch:
            # as the network runs it: both operands row-pitched, no bias (the bias-gradient kernel reads dense rows, and the
            # convs that get pitched operands have no bias) ...
            dw, _ = ops.conv2d_wgrad(dyd, xd, (Cout, Cin, k, k), s, p, d)
            worst.append(("wgrad.pitched.rows", hold(f"wgrad.pitched.rows[{wgrad}]", dw, r.dw[f64], r.dw[f32], 0, 2e-5)))
            worst.append(("wgrad.pitched.cols", hold("wgrad.pitched.cols", dw, r.dw[f64], r.dw[f32], 1, 2e-5)))
            # ... and, for the bias gradient, the same kernel on a dense dy
            dyd = r.dyw.to(cuda)
            dsc = ops._desc((N, Cin, H, W), (Cout, Cin, k, k), s, p, d, pitch, 0)
            assert ops.conv_kernel_name(dsc, nc.WGRAD) == wgrad, (case, ops.conv_kernel_name(dsc, nc.WGRAD))
        dw, db = ops.conv2d_wgrad(dyd, xd, (Cout, Cin, k, k), s, p, d, need_bias=True)
        worst.append(("wgrad.rows", hold(f"wgrad.rows[{wgrad}]", dw, r.dw[f64], r.dw[f32], 0, 2e-5)))
        worst.append(("wgrad.cols", hold("wgrad.cols", dw, r.dw[f64], r.dw[f32], 1, 2e-5)))
        dy64 = r.dyw.double()
        sb = dy64.sum((0, 2, 3))
        eb = (db.double().cpu() - sb).abs() / torch.maximum(sb.abs(), _chan(dy64, 1)).clamp_min(1e-300)
        print(f"NARROW_FIG row={ri} case={case} wgrad.bias err/bound={float(eb.max()) / 1e-5:.3f}")
        worst.append(("wgrad.bias", float(eb.max()) / 1e-5))
        del xd, dyd
        dw0, _ = ops.conv2d_wgrad(_operand(r.dy, pitch, cuda), _operand(r.x, pitch, cuda), (Cout, Cin, k, k), s, p, d)
        ew = float((dw0.double().cpu() - r.dw0[f64]).norm() / r.dw0[f64].norm()) / 2e-5
        print(f"NARROW_FIG row={ri} case={case} wgrad.zero_mean.whole err/bound={ew:.3f}")
        worst.append(("wgrad.zero_mean.whole", ew))
        worst.append(("wgrad.zero_mean.rows", hold("wgrad.zero_mean.rows", dw0, r.dw0[f64], r.dw0[f32], 0, 2e-5, 2)))
        worst.append(("wgrad.zero_mean.cols", hold("wgrad.zero_mean.cols", dw0, r.dw0[f64], r.dw0[f32], 1, 2e-5, 2)))
    torch.cuda.synchronize()
    bad = [(what, v) for what, v in worst if not v <= 1.0]
    assert not bad, (case, bad, figs)


# ------------------------------------------------------------------ kept copies of the row-pitched rows
@pytest.fixture
def wp(monkeypatch):
    """An empty registry of kept copies for the test and a spy on what every conv call is told about its buffer (as
    tests/test_step_kernels_gpu.py)."""
    from dcfp_amd import ops
    monkeypatch.setattr(ops, "_WP_OWNERS", weakref.WeakSet())
    monkeypatch.setattr(ops, "_WP_TABLE", {"version": 0, "built": -1, "dev": None, "n": 0, "blocks": 0, "entries": []})
    seen = []
    real = ops._conv_workspace

    def spy(w, which, d, variant=""):
        ws, valid = real(w, which, d, variant)
        seen.append((which, valid, ws.data_ptr(), d.x_pitch, d.dy_pitch))
        return ws, valid
    monkeypatch.setattr(ops, "_conv_workspace", spy)
    return seen


PITCHED = [(c, which) for c in sorted(nc.NARROW_PITCH) for which in (nc.FWD, nc.DGRAD)]


@pytest.mark.parametrize("case,which", PITCHED, ids=["%s-%s" % ("x".join(map(str, c)), nc.PASS_NAMES[w]) for c, w in PITCHED])
def test_pitched_rows_refresh_then_replay(cuda, wp, case, which):
    """cold call (the conv builds its copy) -> buffer overwritten -> refresh_wp() -> the same bits; weights edited behind
    torch's back -> refresh -> the result of a fresh weight tensor, bit for bit, and the fp64 conv per channel."""
    from dcfp_amd import ops
    N, Cin, H, W, Cout, k, s, p, d = case
    pitch = nc.NARROW_PITCH[case]
    assert nc.pitch_of(case) == pitch and nc.routes(case)[which] == "igemm2_dma8_kernel<9>"
    g = torch.Generator().manual_seed(8100 + which)
    shape = (N, Cin, H, W) if which == nc.FWD else (N, Cout, H, W)
    t_cpu = torch.randn(shape, generator=g)
    t = _operand(t_cpu, pitch, cuda)
    w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).to(cuda)

    def run(wt):
        if which == nc.FWD:
            return ops.conv2d_fwd(t, wt, None, s, p, d)
        return ops.conv2d_dgrad(t, wt, (N, Cin, H, W), s, p, d)

    def refresh():
        ops.WEIGHT_EPOCH[0] += 1
        ops.refresh_wp()

    cold = run(w)
    assert wp[-1][:2] == (which, 0) and (wp[-1][3] if which == nc.FWD else wp[-1][4]) == pitch
    (key, (tag, buf, desc)), = w._dcfp_wp.items()
    assert wp[-1][2] == buf.data_ptr()
    snap = buf.clone()
    buf.fill_(0xFF)
    refresh()
    e = nc_layout(desc, which)
    ext = e.T * e.CkP * e.Mpad * 4
    assert e.perm8 == 1 and e.Mpad == 256 and e.M == (Cout if which == nc.FWD else Cin)
    assert torch.equal(buf[:ext], snap[:ext]), "refresh_wp() and the conv disagree about the kept copy"
    assert bool((buf[ext:] == 0xFF).all()), "the refresh wrote past the layout's extent"
    again = run(w)
    assert wp[-1][:3] == (which, 1, buf.data_ptr()) and torch.equal(again, cold)
    version = w._version
    w.data.view(-1)[::3] += 0.01
    w.data.mul_(1.25)
    assert w._version == version
    refresh()
    out = run(w)
    assert wp[-1][1] == 1
    fresh = run(w.clone())
    assert wp[-1][1] == 0
    assert torch.equal(out, fresh) and not torch.equal(out, cold)
    w64, t64 = w.double().cpu(), t_cpu.double()
    if which == nc.FWD:
        ref = F.conv2d(t64, w64, None, s, p, d)
        ref32 = F.conv2d(t_cpu, w.cpu(), None, s, p, d)
        bound = nc.tolerance(case)
    else:
        ref = torch.nn.grad.conv2d_input((N, Cin, H, W), w64, t64, s, p, d)
        ref32 = torch.nn.grad.conv2d_input((N, Cin, H, W), w.cpu(), t_cpu, s, p, d)
        bound = max(nc.tolerance(case), 1e-5)
    a, b, e32 = _per_channel(out, ref, ref32, 1, bound)
    print(f"NARROW_FIG kept case={case} {nc.PASS_NAMES[which]} err/bound={a:.3f} err/held={b:.3f} aten32={e32:.2e}")
    assert b <= 1.0, (case, which, a, b, e32)
    torch.cuda.synchronize()


def nc_layout(desc, which):
    import ctypes as C
    from dcfp_amd import _lib
    e = _lib.WpEntry()
    assert _lib.lib().dcfp_conv2d_wp_layout(C.byref(desc), which, C.byref(e)) == 0
    return e


# ------------------------------------------------------------------ BatchNorm at C = 1, 2, 5
BN_SHAPES = [(2, 1, 16, 16), (3, 2, 16, 48), (2, 5, 32, 32), (2, 1, 9, 13), (3, 2, 7, 11), (2, 5, 15, 17)]
BN_MODES = [(False, False), (True, False), (False, True), (True, True)]         # (relu, residual)


def _bn_ref(x, gamma, beta, r, dy, mask):
    """fp64 F.batch_norm (+residual) (* the ReLU mask of the HIP run: a pre-activation within rounding of zero may fall on
    either side, masks_honest bounds how far from zero)."""
    dt = torch.float64
    C = x.shape[1]
    xx, gg, bb = (t.to(dt).requires_grad_(True) for t in (x, gamma, beta))
    rr = r.to(dt).requires_grad_(True) if r is not None else None
    rm, rv = torch.zeros(C, dtype=dt), torch.ones(C, dtype=dt)
    pre = F.batch_norm(xx, rm, rv, gg, bb, True, 0.1, 1e-5)
    if rr is not None:
        pre = pre + rr
    y = pre * mask.to(dt) if mask is not None else pre
    y.backward(dy.to(dt))
    return y.detach(), pre.detach(), rm, rv, xx.grad, gg.grad, bb.grad, (rr.grad if rr is not None else None)


@pytest.mark.parametrize("relu,res", BN_MODES, ids=["plain", "relu", "res", "res_relu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=["x".join(map(str, s)) for s in BN_SHAPES])
def test_batch_norm_narrow_vs_fp64(cuda, shape, relu, res):
    """ops.batch_norm_act, and where H*W % 256 == 0 with residual and ReLU also the 1-bit-mask pair bn_forward_impl(want_mask)
    / bn_backward_impl that a Bottleneck's bn3 runs.  Bounds of test_random_bn (y 3e-5 absolute, running mean 1e-6 and var
    1e-5, gradients 2e-4 relative L2), the gradients per channel."""
    from dcfp_amd import ops
    N, C, H, W = shape
    g = torch.Generator().manual_seed(9000 + 100 * C + H + 2 * relu + res)
    x = torch.randn(shape, generator=g) * 1.7 + 0.3
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    r = torch.randn(shape, generator=g) if res else None
    dy = torch.randn(shape, generator=g)

    def check(tag, y, rm, rv, dx, dg, db, dr):
        mask = (y.detach().cpu() > 0) if relu else None
        y64, pre64, rm64, rv64, dx64, dg64, db64, dr64 = _bn_ref(x, gamma, beta, r, dy, mask)
        if relu:
            _flip_cap(nr.masks_honest([mask], [pre64]), y.numel(), f"bn {shape} {tag}")
        assert float((y.double().cpu() - y64).abs().max()) < 3e-5, tag
        assert float((rm.double().cpu() - rm64).abs().max()) < 1e-6, tag
        assert float((rv.double().cpu() - rv64).abs().max()) < 1e-5 * max(1.0, float(rv64.abs().max())), tag
        for what, got, want in (("dx", dx, dx64), ("dres", dr, dr64)):
            if want is None:
                continue
            e = _chan(got.double().cpu() - want, 1) / _chan(want, 1).clamp_min(1e-300)
            assert float(e.max()) < 2e-4, (tag, what, e.tolist())
        for what, got, want in (("dgamma", dg, dg64), ("dbeta", db, db64)):
            e = float((got.double().cpu() - want).norm() / want.norm().clamp_min(1e-300))
            assert e < 2e-4, (tag, what, e)

    xg, gmg, bg = (t.to(cuda).requires_grad_(True) for t in (x, gamma, beta))
    rg = r.to(cuda).requires_grad_(True) if res else None
    rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    y = ops.batch_norm_act(xg, gmg, bg, rm, rv, rg, relu, True, 0.1, 1e-5, False)
    y.backward(dy.to(cuda))
    check("batch_norm_act", y.detach(), rm, rv, xg.grad, gmg.grad, bg.grad, rg.grad if res else None)
    if relu and res:
        rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
        xd, gd, bd, rd, dyd = (t.to(cuda) for t in (x, gamma, beta, r, dy))
        y, state = ops.bn_forward_impl(xd, gd, bd, rm, rv, rd, True, True, 0.1, 1e-5, False, want_mask=True)
        assert (len(state) > 4) == ((H * W) % 256 == 0), (shape, len(state))       # the bit mask exists exactly there
        dx, dg, db, dr = ops.bn_backward_impl(dyd, xd, None if len(state) > 4 else y, gd, bd, state, True, True, 1e-5, True)
        check("bit mask" if len(state) > 4 else "saved output", y, rm, rv, dx, dg, db, dr)
    torch.cuda.synchronize()
    ops.check_fused_status()


# ------------------------------------------------------------------ fused nodes at the fixtures' widths
def _fn():
    import test_fused_nodes_gpu as fn       # its harness: the HIP runs, the fp64 / fp32 composites, the comparisons
    return fn


# name: (input shape, [(planes, stride, dilation, downsample, (c1, c2, cout))] per block)
CHAINS = {
    # layer1.0 and its successor: conv2 leaves ONE channel; small map (H*W % 256 == 0: bn3 keeps its mask as bits)
    "c_to_1": ((2, 20, 16, 32), [(10, 1, 1, True, (7, 1, 37)), (10, 1, 1, False, (9, 1, 37))]),
    # ... at a map where the 3x3 conv reads a row-pitched y1 / d_c2 with one live output row
    "c_to_1_pitched": ((2, 20, 128, 192), [(10, 1, 1, True, (7, 1, 37)), (10, 1, 1, False, (3, 1, 37))]),
    # layer2.0: conv1 leaves TWO channels, stride 2 at odd sizes with a downsample pair
    "2_to_c_stride2": ((2, 37, 33, 41), [(9, 2, 1, True, (2, 9, 20)), (9, 1, 1, False, (2, 7, 20))]),
    # layer3.1: conv2 leaves FIVE channels at dilation 2, identity shortcuts, row-pitched
    "c_to_5_dil2": ((2, 37, 128, 192), [(10, 1, 2, False, (9, 5, 37)), (10, 1, 2, False, (3, 5, 37))]),
    # 256-channel blocks with 7 / 3 and 5 channels inside: conv1's data gradient is the masked fan-in with a narrow K
    "fanin_narrow_k": ((2, 256, 128, 192), [(64, 1, 2, False, (7, 5, 256)), (64, 1, 2, False, (3, 5, 256))]),
}
# name: (row pitch of y1 / d_c2 per block, fan-in data gradient per block (else the plain accumulate form))
NARROW_CHAIN_ROUTING = {"c_to_1": ((0, 0), (False, False)), "c_to_1_pitched": ((196, 196), (False, False)),
                        "2_to_c_stride2": ((0, 0), (False, False)), "c_to_5_dil2": ((196, 196), (False, False)),
                        "fanin_narrow_k": ((196, 196), (True, True))}


def _chain(name):
    fn = _fn()
    xs, blocks = CHAINS[name]
    master, cin, shape = [], xs[1], xs
    shapes = []
    for k, (planes, stride, dil, ds, cut) in enumerate(blocks):
        master.append(fn._block(cin, planes, stride, dil, ds, cut, seed=50 + 7 * len(name) + k))
        shapes.append(shape)
        cin = cut[2]
        shape = (shape[0], cin, (shape[2] - 1) // stride + 1, (shape[3] - 1) // stride + 1)
    return master, xs, shape, shapes


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(CHAINS))
def test_narrow_bottleneck_chain_vs_fp64_composite(cuda, name, train):
    fn = _fn()
    master, xs, ys, shapes = _chain(name)
    pitches, fanins = NARROW_CHAIN_ROUTING[name]
    for blk, shape, pitch, fanin, (_, _, _, _, cut) in zip(master, shapes, pitches, fanins, CHAINS[name][1]):
        rt = fn._block_routing(blk, shape)
        assert [blk.conv1.weight.shape[0], blk.conv2.weight.shape[0], blk.conv3.weight.shape[0]] == list(cut)
        assert rt.pitch == pitch and bool(rt.fanin) == fanin, (name, rt)
        if fanin:
            assert rt.conv1[1] == "igemm2_dma1p_kernel", rt
    x, dy = fn._inputs(71, xs, ys)
    r = fn._run(f"narrow.{name}.{'train' if train else 'eval'}", "bottleneck", cuda, master, x, dy, train)
    total = sum(int(m.numel()) for mk in r.masks for m in mk)
    _flip_cap(r.ref.flipped, total, f"bottleneck {name} {'train' if train else 'eval'}")


ASPP_SHAPE, ASPP_WIDTHS = (4, 24, 17, 33), [5, 1, 2, 3, 5]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_narrow_aspp_vs_fp64_composite(cuda, train):
    from dcfp_amd.networks.tools.aspp import ASPP
    fn = _fn()
    N, cin, H, W = ASPP_SHAPE
    m = ASPP(16, True, inplanes=cin, outplanes=None)
    nr.cut_aspp(m, ASPP_WIDTHS)
    nr.seed(m, torch.Generator().manual_seed(77))
    # the slices behind the width-5, the width-1 and the width-3 branch start 1, 2 and 3 floats off a 16-byte boundary
    assert [(sum(ASPP_WIDTHS[:k]) * H * W) % 4 for k in (1, 2, 4)] == [1, 2, 3], ASPP_WIDTHS
    br = [fn._names(ASPP_SHAPE, (ASPP_WIDTHS[0], cin, 1, 1), 1, 0, 1)]
    br += [fn._names(ASPP_SHAPE, (ASPP_WIDTHS[k], cin, 3, 3), 1, fn.DILATIONS[k], fn.DILATIONS[k]) for k in (1, 2, 3)]
    assert all(fn._direct(b) for b in br), br
    assert fn._names((N, cin, 1, 1), (ASPP_WIDTHS[4], cin, 1, 1), 1, 0, 1) == ["gemv_1x1_map_kernel"] * 3
    x, dy = fn._inputs(72, ASPP_SHAPE, (N, sum(ASPP_WIDTHS), H, W))
    r = fn._run(f"narrow.aspp.{'train' if train else 'eval'}", "aspp", cuda, [m], x, dy, train)
    _flip_cap(r.ref.flipped, int(r.masks.numel()), f"aspp [5, 1, 2, 3, 5] {'train' if train else 'eval'}")


def _rel(a, b):
    return nr.rel(a, b)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("hw,HW", [((17, 33), (33, 65)), ((32, 64), (64, 128))])
def test_narrow_decoder_concat_vs_fp64_composite(cuda, train, hw, HW):
    """DecoderConcatFn with a 2-channel low-level reduction and a 5-channel ASPP output; the bounds of
    test_deeplabv3p_gpu.py::test_decoder_concat_vs_fp64_composite."""
    from dcfp_amd import ops
    from dcfp_amd.networks import _exec
    from dcfp_amd.networks.deeplabv3p import Decoder
    N, Cx, Cl, Cr = 2, 5, 23, 2
    g = torch.Generator().manual_seed(73)
    dec = Decoder(19, True, high_level_inplanes=Cx, low_level_inplanes=Cl)
    nr.cut_conv(dec.conv1, cout=Cr); nr.cut_bn(dec.bn1, Cr)
    nr.cut_conv(dec.last_conv[0], cin=Cx + Cr)
    nr.seed(dec, g)
    ref = copy.deepcopy(dec).double().to(cuda).train(train)
    ref32 = copy.deepcopy(dec).to(cuda).train(train)
    dec = dec.to(cuda).train(train)
    x64 = torch.randn(N, Cx, *hw, generator=g, dtype=torch.float64).to(cuda).requires_grad_(True)
    low64 = torch.relu(torch.randn(N, Cl, *HW, generator=g, dtype=torch.float64)).to(cuda).requires_grad_(True)
    dcat = torch.randn(N, Cx + Cr, *HW, generator=g).to(cuda)
    x = x64.detach().float().requires_grad_(True)
    low = low64.detach().float().requires_grad_(True)
    pitch = dec.concat_pitch((N, Cx + Cr) + tuple(HW))
    cfg = {"bn": _exec._bn_args(dec.bn1), "pitch": pitch, "owner": dec, "align": True}
    cat = ops.decoder_concat(x, low, cfg, dec.conv1.weight, dec.bn1.weight, dec.bn1.bias)
    assert ops._pitch_of(cat) == pitch
    assert (Cx * HW[0] * HW[1]) % 4 or HW == (64, 128)             # 33 x 65: the low-level slice starts at an odd offset
    cat.backward(dcat)
    mask = cat.detach()[:, Cx:] > 0

    def composite(m, xx, ll):
        a = F.interpolate(xx, size=HW, mode="bilinear", align_corners=True)
        pre = m.bn1(m.conv1(ll))
        return torch.cat((a, pre * mask.to(xx.dtype)), 1), pre
    with torch.backends.cudnn.flags(enabled=False):
        want, pre = composite(ref, x64, low64)
        want.backward(dcat.double())
        x32 = x.detach().clone().requires_grad_(True); low32 = low.detach().clone().requires_grad_(True)
        composite(ref32, x32, low32)[0].backward(dcat)
    torch.cuda.synchronize()
    _flip_cap(nr.masks_honest([mask], [pre]), int(mask.numel()), f"decoder {HW} {'train' if train else 'eval'}")
    assert _rel(cat.detach(), want.detach()) <= 1e-5
    assert _rel(x.grad, x64.grad) <= 1e-5
    # per low-level channel and per reduced channel
    for c in range(Cl):
        assert _rel(low.grad[:, c], low64.grad[:, c]) <= max(1e-4, 3 * _rel(low32.grad[:, c], low64.grad[:, c])), c
    for c in range(Cr):
        assert _rel(dec.conv1.weight.grad[c], ref.conv1.weight.grad[c]) <= \
            max(1e-4, 3 * _rel(ref32.conv1.weight.grad[c], ref.conv1.weight.grad[c])), c
    eg, eb = _rel(dec.bn1.weight.grad, ref.bn1.weight.grad), _rel(dec.bn1.bias.grad, ref.bn1.bias.grad)
    print(f"NARROW_FIG decoder {HW} {'train' if train else 'eval'} d_gamma={eg:.2e} (bound 1e-4) d_beta={eb:.2e} (bound 1e-5) "
          f"aten32 {_rel(ref32.bn1.weight.grad, ref.bn1.weight.grad):.2e} {_rel(ref32.bn1.bias.grad, ref.bn1.bias.grad):.2e}")
    assert eg <= 1e-4 and eb <= 1e-5, (eg, eb)
    assert _rel(dec.bn1.running_mean, ref.bn1.running_mean) <= 1e-5
    assert _rel(dec.bn1.running_var, ref.bn1.running_var) <= 1e-5
    assert int(dec.bn1.num_batches_tracked) == int(ref.bn1.num_batches_tracked)


PPM_WIDTHS, PPM_SIZES = [1, 2, 5, 3], (1, 2, 3, 6)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("HW", [(9, 9), (17, 33)])
def test_narrow_pyramid_pooling_vs_fp64_composite(cuda, train, HW):
    """PyramidPoolingFn with stage widths [1, 2, 5, 3]; the composite and the bounds of
    test_psp_gpu.py::test_pyramid_pooling_vs_fp64_composite.  No mask is taken from the kernel (the ReLU sits in front of
    the interpolation: the concat does not show it), so there is no flip count here - a flipped element would be an error."""
    from dcfp_amd import ops
    from dcfp_amd.networks import _exec
    from dcfp_amd.networks.tools.ppm import PPMModule
    # (four images: the first stage's BatchNorm sees N values per channel, and with N = 2 its backward is a difference of
    #  two numbers that agree to eps / var - the ill-conditioned case the ASPP pool branch is run at N = 4 for as well)
    N, Cf = 4, 24
    g = torch.Generator().manual_seed(74)
    mod = PPMModule(Cf, 512, align_corners=True)
    for st, w in zip(mod.stages, PPM_WIDTHS):
        nr.cut_conv(st[1], cout=w); nr.cut_bn(st[2], w)
    nr.cut_conv(mod.bottleneck[0], cin=sum(PPM_WIDTHS) + Cf)
    nr.seed(mod, g)
    ref = copy.deepcopy(mod).double().to(cuda).train(train)
    ref32 = copy.deepcopy(mod).to(cuda).train(train)
    mod = mod.to(cuda).train(train)
    f64 = torch.relu(torch.randn(N, Cf, *HW, generator=g, dtype=torch.float64)).to(cuda).requires_grad_(True)
    f = f64.detach().float().requires_grad_(True)
    dcat = torch.randn(N, sum(PPM_WIDTHS) + Cf, *HW, generator=g).to(cuda)
    tensors = [t for st in mod.stages for t in (st[1].weight, st[2].weight, st[2].bias)]
    pitch = mod.concat_pitch((N, sum(PPM_WIDTHS) + Cf) + tuple(HW))
    cfg = {"sizes": list(PPM_SIZES), "bn": [_exec._bn_args(st[2]) for st in mod.stages], "pitch": pitch, "owner": mod,
           "align": True}
    cat = ops.pyramid_pooling(f, cfg, tensors)
    assert ops._pitch_of(cat) == pitch
    cat.backward(dcat)

    def composite(m, x):
        return torch.cat([F.interpolate(torch.relu(st[2](st[1](F.adaptive_avg_pool2d(x, s)))), size=HW,
                                        mode="bilinear", align_corners=True) for st, s in zip(m.stages, PPM_SIZES)] + [x], 1)
    with torch.backends.cudnn.flags(enabled=False):
        want = composite(ref, f64)
        want.backward(dcat.double())
        f32 = f.detach().clone().requires_grad_(True)
        composite(ref32, f32).backward(dcat)
    torch.cuda.synchronize()
    o = 0
    for k, w in enumerate(PPM_WIDTHS):          # per stage slice: the width-1 slice must not hide behind the others
        assert _rel(cat.detach()[:, o:o + w], want.detach()[:, o:o + w]) <= 1e-5, k
        o += w
    assert torch.equal(cat.detach()[:, o:], f.detach())
    assert _rel(f.grad, f64.grad) <= max(1e-5, 3 * _rel(f32.grad, f64.grad))
    for st, rs, r32 in zip(mod.stages, ref.stages, ref32.stages):
        for a, b, c, floor in ((st[1].weight, rs[1].weight, r32[1].weight, 1e-4),
                               (st[2].weight, rs[2].weight, r32[2].weight, 1e-4),
                               (st[2].bias, rs[2].bias, r32[2].bias, 1e-5)):
            assert _rel(a.grad, b.grad) <= max(floor, 3 * _rel(c.grad, b.grad))
        assert _rel(st[2].running_mean, rs[2].running_mean) <= 1e-5
        assert _rel(st[2].running_var, rs[2].running_var) <= 1e-5
        assert int(st[2].num_batches_tracked) == int(rs[2].num_batches_tracked)
