"""The fp32 training kernels on operands off the 16-byte grid (tests/_align.py), against fp64.

conv_igemm2*.hip, conv_winograd2/3.hip, conv_wgrad.hip, conv_stem.hip, bn.hip, pool.hip and ppm.hip choose between a
16-byte and a 4-byte path on the host, from the addresses they are handed.  Every case here runs a shape that takes the
16-byte path when its operands are aligned - it asserts the aligned call's kernel name, the shape condition and the
operand's data_ptr() % 16 first - and then moves one operand at a time (and all at once) 4, 8 or 12 bytes off the grid,
inside a buffer of guard words.  Held: no call is refused, the result is within the project's own bound of fp64 on the
CPU, nothing outside the tensor is written, every element of an output is written.

Bits.  A displaced weight tensor gives the bits of the aligned call (the kernels read the permuted copy).  A displaced
x / dy gives the bits of the aligned call on every register-staged route (same kernel, same summation order).  On an
LDS-DMA route a displaced source must not reach the kernel - it copies 16 bytes at a time from the source - and runs
another family with another summation order: such a result is held to fp64 only, and to the BITS of the same conv in a
child process whose switches take the LDS-DMA families away (DCFP_IGEMM_DMA=0 DCFP_WINO_FUSED=0 DCFP_WGRAD_DMA=0
DCFP_WINO_WGRAD_FUSED=0; the library latches them, hence the child) - that is what shows which family ran."""
import ctypes as C
import hashlib
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _align as al
import _narrow_cases as nc
import _wp_cases as wp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_ENV = {"DCFP_IGEMM_DMA": "0", "DCFP_WINO_FUSED": "0", "DCFP_WGRAD_DMA": "0", "DCFP_WINO_WGRAD_FUSED": "0"}


def rel_err(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def max_err(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _id(row):
    return "x".join(str(v) for v in row[0])


# ------------------------------------------------------------------ inputs and fp64 references (computed once per case)
_IN, _REF = {}, {}


def _inputs(case):
    if case not in _IN:
        N, Cin, H, W, Cout, k, s, p, d = case
        g = torch.Generator().manual_seed(sum((i + 3) * v for i, v in enumerate(case)))
        x = torch.randn(N, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
        b = torch.randn(Cout, generator=g)
        Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
        dy = torch.randn(N, Cout, Ho, Wo, generator=g)
        seed = torch.randn(N, Cin, H, W, generator=g)
        _IN[case] = (x, w, b, dy, seed)
    return _IN[case]


def _ref(case, what):
    """fp64 on the CPU: "y" F.conv2d, "dx" / "dw" its autograd."""
    if (case, what) not in _REF:
        x, w, b, dy, seed = _inputs(case)
        s, p, d = case[6:]
        if what == "y":
            r = F.conv2d(x.double(), w.double(), None, s, p, d)
        elif what == "dx":
            r = torch.nn.grad.conv2d_input(x.shape, w.double(), dy.double(), s, p, d)
        else:
            r = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), s, p, d)
        _REF[(case, what)] = r
    return _REF[(case, what)]


def _desc(case, xp=0, dp=0):
    from dcfp_amd import ops
    N, Cin, H, W, Cout, k, s, p, d = case
    return ops._desc((N, Cin, H, W), (Cout, Cin, k, k), s, p, d, xp, dp)


def _name(case, which, xp=0, dp=0):
    from dcfp_amd import ops
    return ops.conv_kernel_name(_desc(case, xp, dp), which)


def _operand(t, k, dev, pitch=0):
    """`t` on the device at data_ptr() % 16 == 4 * k, row-pitched where the row is -> (tensor, Guarded or None)."""
    from dcfp_amd import ops
    t = t.to(dev)
    if k == 0 and not pitch:
        return t, None
    if k == 0:
        v = ops.new_pitched(tuple(t.shape), pitch, dev)
        v.copy_(t)
        return v, None
    g = al.displaced_pitched(t, k, pitch) if pitch else al.displaced(t, k)
    assert g.view.data_ptr() % 16 == 4 * k
    return g.view, g


def _intact(*guards):
    for g in guards:
        assert g is None or g.guards_intact(), "a store outside the tensor"


# ------------------------------------------------------------------ the child: the same convs without the LDS-DMA families
def _child(path):
    sys.path.insert(0, ROOT)
    from dcfp_amd import ops
    dev = torch.device("cuda:0")
    out = {}
    for case, fwd, dgrad in al.CONV:
        x, w, b, dy, seed = _inputs(case)
        s, p, d = case[6:]
        if case in nc.NARROW_PITCH:
            continue        # (a displaced pitched operand is made dense by ops: held to fp64 only)
        if fwd in al.LDS_DMA:
            out["fwd:" + _id((case,))] = _sha(ops.conv2d_fwd(x.to(dev), w.to(dev), None, s, p, d))
        if dgrad in al.LDS_DMA:
            out["dgrad:" + _id((case,))] = _sha(ops.conv2d_dgrad(dy.to(dev), w.to(dev), tuple(x.shape), s, p, d))
    for case, name, xp, flags in al.WGRAD:
        if name in al.WGRAD_LDS_DMA and "kept" not in flags:
            x, w, b, dy, seed = _inputs(case)
            s, p, d = case[6:]
            dw, _ = ops.conv2d_wgrad(dy.to(dev), x.to(dev), tuple(w.shape), s, p, d)
            out["wgrad:" + _id((case,))] = _sha(dw)
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump(out, f)


@pytest.fixture(scope="module")
def child(cuda, tmp_path_factory):
    """{pass:case: sha256 of the result} of the LDS-DMA rows computed with the LDS-DMA families switched off."""
    path = str(tmp_path_factory.mktemp("align") / "child.json")
    env = dict(os.environ, **CHILD_ENV)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(path) as f:
        return json.load(f)


# ------------------------------------------------------------------ conv forward
FWD_ROWS = [r for r in al.CONV if r[1] is not None]
DGRAD_ROWS = [r for r in al.CONV if r[2] is not None]
# operand -> k, one at a time; then all at once with three different k
FWD_VARIANTS = [("x", dict(x=1)), ("w", dict(w=1)), ("out", dict(out=1)), ("slice", dict(out=1, slice=True)),
                ("bias", dict(b=1)), ("all", dict(x=1, w=2, out=3, b=2))]


@pytest.mark.parametrize("row", FWD_ROWS, ids=_id)
def test_conv_forward(cuda, child, row):
    from dcfp_amd import _lib, ops
    case, fwd, _ = row
    N, Cin, H, W, Cout, k, s, p, d = case
    pitch = nc.NARROW_PITCH.get(case, 0)
    assert _name(case, _lib.CONV_FWD, pitch, pitch) == fwd and al.vector_eligible(case)
    x, w, b, dy, seed = _inputs(case)
    y64 = _ref(case, "y")
    tol = wp.conv_tolerance(case)
    xa, _ = _operand(x, 0, cuda, pitch)
    wd, bd = w.to(cuda), b.to(cuda)
    assert xa.data_ptr() % 16 == 0 and wd.data_ptr() % 16 == 0
    y0 = ops.conv2d_fwd(xa, wd, None, s, p, d)
    y0b = ops.conv2d_fwd(xa, wd, bd, s, p, d)
    assert y0.data_ptr() % 16 == 0
    e0 = rel_err(y0, y64)
    print(f"fwd {case} {fwd}: aligned {e0:.2e} / {tol:.2e}")
    assert e0 <= tol
    y64b = y64 + b.double().view(1, -1, 1, 1)
    for tag, v in FWD_VARIANTS:
        xv, gx = _operand(x, v.get("x", 0), cuda, pitch)
        wv, gw = _operand(w, v.get("w", 0), cuda)
        bv, gb = _operand(b, v["b"], cuda) if "b" in v else (None, None)
        go = None
        if v.get("slice"):
            go = al.displaced_slice(tuple(y64.shape), v["out"], 1, Cout + 3, device=cuda)
            assert go.view.data_ptr() % 4 == 0 and go.view.stride(0) == (Cout + 3) * y64.shape[2] * y64.shape[3]
        elif "out" in v:
            go = al.displaced_empty(tuple(y64.shape), v["out"], device=cuda)
            assert go.view.data_ptr() % 16 == 4 * v["out"]
        y = ops.conv2d_fwd(xv, wv, bv, s, p, d, out=go.view if go is not None else None)     # (refusals raise)
        torch.cuda.synchronize()
        _intact(gx, gw, gb, go)
        assert go is None or go.unwritten() == 0, (tag, go.unwritten())
        err = rel_err(y, y64b if bv is not None else y64)
        print(f"fwd {case} {fwd}: {tag} {err:.2e} / {tol:.2e}")
        assert err <= tol, (tag, err, tol)
        if tag == "w":
            assert torch.equal(y, y0), "a displaced w changed the result: the kernels read the permuted copy"
        if tag == "bias" and fwd not in (al.WINO_FUSED, al.WINO_3PASS):
            assert torch.equal(y, y0b)
        if tag == "x":
            if pitch:
                pass        # ops hands the library a dense copy of a pitched x that is off the grid: held to fp64 above
            elif fwd in al.LDS_DMA:
                # another family, another summation order: held to fp64 above, and to the bits of the family that must have run
                assert _sha(y) == child["fwd:" + _id(row)], "a displaced x did not run the register-staged family"
            else:
                assert torch.equal(y, y0), "a displaced x changed the bits of a register-staged route"


@pytest.mark.parametrize("row", DGRAD_ROWS, ids=_id)
def test_conv_dgrad(cuda, child, row):
    from dcfp_amd import _lib, ops
    case, _, dgrad = row
    N, Cin, H, W, Cout, k, s, p, d = case
    pitch = nc.NARROW_PITCH.get(case, 0)
    assert _name(case, _lib.CONV_DGRAD, pitch, pitch) == dgrad and al.vector_eligible(case)
    x, w, b, dy, seed = _inputs(case)
    dx64 = _ref(case, "dx")
    tol = max(wp.conv_tolerance(case), 1e-5)
    dya, _ = _operand(dy, 0, cuda, pitch)
    wd = w.to(cuda)
    dx0 = ops.conv2d_dgrad(dya, wd, tuple(x.shape), s, p, d)
    assert dya.data_ptr() % 16 == 0 and dx0.data_ptr() % 16 == 0
    e0 = rel_err(dx0, dx64)
    print(f"dgrad {case} {dgrad}: aligned {e0:.2e} / {tol:.2e}")
    assert e0 <= tol
    acc64 = dx64 + seed.double()
    variants = [("dy", dict(dy=1)), ("w", dict(w=1)), ("out", dict(out=1)), ("acc", dict(out=1, acc=True)),
                ("all", dict(dy=1, w=2, out=3)), ("all-acc", dict(dy=3, w=1, out=2, acc=True))]
    if not pitch:
        variants.append(("slice", dict(dy=1, slice=True)))
    for tag, v in variants:
        wv, gw = _operand(w, v.get("w", 0), cuda)
        if v.get("slice"):      # dy as a channel slice of a displaced wider tensor (ops._batch_strided)
            gy = al.displaced_slice(tuple(dy.shape), v["dy"], 2, Cout + 3, device=cuda, src=dy.to(cuda))
            dyv = gy.view
        else:
            dyv, gy = _operand(dy, v.get("dy", 0), cuda, pitch)
        go = None
        if "out" in v:
            go = al.displaced(seed.to(cuda), v["out"]) if v.get("acc") else al.displaced_empty(tuple(x.shape), v["out"], device=cuda)
            assert go.view.data_ptr() % 16 == 4 * v["out"]
        dx = ops.conv2d_dgrad(dyv, wv, tuple(x.shape), s, p, d, out=go.view if go is not None else None,
                              accumulate=bool(v.get("acc")))
        torch.cuda.synchronize()
        _intact(gy, gw, go)
        assert go is None or go.unwritten() == 0, (tag, go.unwritten())
        err = rel_err(dx, acc64 if v.get("acc") else dx64)       # accumulate: the seed plus the data gradient
        print(f"dgrad {case} {dgrad}: {tag} {err:.2e} / {tol:.2e}")
        assert err <= tol, (tag, err, tol)
        if tag == "w":
            assert torch.equal(dx, dx0)
        if tag in ("dy", "slice"):
            if pitch:
                pass        # (as in the forward: a dense copy of the pitched dy)
            elif dgrad in al.LDS_DMA:
                assert _sha(dx) == child["dgrad:" + _id(row)], "a displaced dy did not run the register-staged family"
            else:
                assert torch.equal(dx, dx0), "a displaced dy changed the bits of a register-staged route"


# ------------------------------------------------------------------ conv options
def _stats_ok(stats, y):
    """The bound tests/test_ops_gpu.py::test_conv_fused_bn_stats holds the fused statistics to."""
    if stats is None:
        return
    m64 = y.double().mean((0, 2, 3)); v64 = y.double().var((0, 2, 3), unbiased=False)
    assert max_err(stats[0], m64) < 2e-6 * max(1.0, m64.abs().max().item())
    assert ((stats[1].double().cpu() - v64.cpu()).abs() / v64.cpu()).max().item() < 2e-6


@pytest.mark.parametrize("case", al.OPTION_ROWS, ids=lambda c: "x".join(map(str, c)))
def test_conv_options(cuda, case):
    from dcfp_amd import _lib, ops
    N, Cin, H, W, Cout, k, s, p, d = case
    x, w, b, dy, seed = _inputs(case)
    y64 = _ref(case, "y")
    tol = wp.conv_tolerance(case)
    xd, wd = x.to(cuda), w.to(cuda)
    name = _name(case, _lib.CONV_FWD)
    # -- want_stats: the aligned call has the statistics epilogue; a displaced y either declines it or is as good
    y0, st0 = ops.conv2d_fwd(xd, wd, None, s, p, d, want_stats=True)
    assert st0 is not None or name not in (al.DMA1P, al.WINO_FUSED), (case, name)      # (the 128-row tile row has ragged pixel tiles)
    _stats_ok(st0, y0)
    for kx, ko in ((0, 1), (1, 0), (2, 3)):
        xv, gx = _operand(x, kx, cuda)
        go = al.displaced_empty(tuple(y64.shape), ko, device=cuda)
        assert go.view.data_ptr() % 16 == 4 * ko
        y, st = ops.conv2d_fwd(xv, wd, None, s, p, d, want_stats=True, out=go.view)
        torch.cuda.synchronize()
        _intact(gx, go)
        assert go.unwritten() == 0 and rel_err(y, y64) <= tol, (kx, ko, rel_err(y, y64))
        _stats_ok(st, y)
        print(f"stats {case} {name}: x%16={4 * kx} y%16={4 * ko} stats {'None' if st is None else 'kept'}")
    # -- the inference epilogue with a displaced residual (and a displaced x)
    g = torch.Generator().manual_seed(5)
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(y64.shape, generator=g)
    want = torch.relu(y64 * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) + res.double())
    f0 = ops.conv2d_fused_infer(xd, wd, scale.to(cuda), shift.to(cuda), s, p, d, residual=res.to(cuda), relu=True)
    for kx, kr in ((0, 1), (1, 0), (3, 2)):
        xv, gx = _operand(x, kx, cuda)
        rv, gr = _operand(res, kr, cuda)
        f1 = ops.conv2d_fused_infer(xv, wd, scale.to(cuda), shift.to(cuda), s, p, d, residual=rv, relu=True)
        torch.cuda.synchronize()
        _intact(gx, gr)
        assert rel_err(f1, want) <= tol, (kx, kr, rel_err(f1, want))
        if kx == 0:
            assert torch.equal(f1, f0), "a displaced residual changed the result"
    # -- keep= on the Winograd row: the forward leaves its transform behind where it can, the weight gradient is right either way
    if name.startswith("winograd"):
        dw64 = _ref(case, "dw")
        for kx in (0, 1):
            xv, gx = _operand(x, kx, cuda)
            kp = {}
            y = ops.conv2d_fwd(xv, wd, None, s, p, d, keep=kp)
            dw, _ = ops.conv2d_wgrad(dy.to(cuda), xv, tuple(w.shape), s, p, d, xform=kp.get("xform"))
            torch.cuda.synchronize()
            _intact(gx)
            assert rel_err(y, y64) <= tol and rel_err(dw, dw64) <= 2e-5


def test_conv_dgrad_fanin(cuda):
    """dx = dgrad(dy) + fan_src * mask where conv2d_dgrad_fanin_ok says yes, every operand displaced in turn."""
    from dcfp_amd import _lib, ops
    case = al.FANIN_ROW
    N, Cin, H, W, Cout, k, s, p, d = case
    x, w, b, dy, seed = _inputs(case)
    wd = w.to(cuda)
    assert ops.conv2d_dgrad_fanin_ok(None, wd, tuple(x.shape)) and _name(case, _lib.CONV_DGRAD) == al.DMA1P
    g = torch.Generator().manual_seed(9)
    gamma, beta = (torch.rand(Cin, generator=g) + 0.5).to(cuda), (torch.randn(Cin, generator=g) * 0.1).to(cuda)
    r = torch.randn(x.shape, generator=g).to(cuda)
    mean, var = ops.bn_stats(x.to(cuda))
    ym = ops.bn_apply_relu_mask(x.to(cuda), mean, var, gamma, beta, 1e-5, r)
    assert ym is not None
    yb, mask = ym
    want = _ref(case, "dx") + seed.double() * (yb > 0).double().cpu()
    tol = max(wp.conv_tolerance(case), 1e-5)
    dx0 = ops.conv2d_dgrad_fanin(dy.to(cuda), wd, tuple(x.shape), seed.to(cuda), mask)
    assert rel_err(dx0, want) <= tol
    for kdy, kw, kf in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3)):
        dyv, gy = _operand(dy, kdy, cuda)
        wv, gw = _operand(w, kw, cuda)
        fv, gf = _operand(seed, kf, cuda)
        dx = ops.conv2d_dgrad_fanin(dyv, wv, tuple(x.shape), fv, mask)
        torch.cuda.synchronize()
        _intact(gy, gw, gf)
        assert rel_err(dx, want) <= tol, (kdy, kw, kf, rel_err(dx, want))
        assert torch.equal(dx, dx0)      # (ops copies an off-grid dy / fan_src onto the grid: the same kernel)


# ------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize("row", al.WGRAD, ids=_id)
def test_conv_wgrad(cuda, child, row):
    from dcfp_amd import _lib, ops
    case, name, xp, flags = row
    N, Cin, H, W, Cout, k, s, p, d = case
    assert _name(case, _lib.CONV_WGRAD, xp, 0) == name and al.vector_eligible(case)
    x, w, b, dy, seed = _inputs(case)
    dw64 = _ref(case, "dw")
    db64 = dy.double().sum((0, 2, 3))
    bias = "bias" in flags
    xa, _ = _operand(x, 0, cuda, xp)
    dya = dy.to(cuda)
    wn = Cout * Cin * k * k
    if "splits" in flags:       # several split-K slabs, reduced by the vector kernel when dw is aligned
        assert wn % 4 == 0 and _lib.lib().dcfp_conv2d_workspace_bytes(C.byref(_desc(case, xp, 0)), _lib.CONV_WGRAD) >= 2 * wn * 4
    kp = {}
    if "kept" in flags:
        ops.conv2d_fwd(xa, w.to(cuda), None, s, p, d, keep=kp)
        assert "xform" in kp, "the aligned forward did not leave its transform behind"
        # ... and a forward whose x is off the grid keeps nothing (no Winograd pass ran) or something its weight gradient can use
        xv, gx = _operand(x, 1, cuda)
        kp2 = {}
        y = ops.conv2d_fwd(xv, w.to(cuda), None, s, p, d, keep=kp2)
        dwk, _ = ops.conv2d_wgrad(dya, xv, tuple(w.shape), s, p, d, xform=kp2.get("xform"))
        assert rel_err(y, _ref(case, "y")) <= wp.conv_tolerance(case) and rel_err(dwk, dw64) <= 2e-5 and gx.guards_intact()
    dw0, db0 = ops.conv2d_wgrad(dya, xa, tuple(w.shape), s, p, d, need_bias=bias, xform=kp.get("xform"))
    e0 = rel_err(dw0, dw64)
    print(f"wgrad {case} {name}: aligned {e0:.2e} / 2e-5")
    assert e0 <= 2e-5 and dw0.data_ptr() % 16 == 0
    variants = [("dy", dict(dy=1)), ("x", dict(x=1)), ("dw", dict(dw=1)), ("slice", dict(dy=1, slice=True)),
                ("all", dict(dy=1, x=2, dw=3, db=1))]
    if bias:
        variants.append(("db", dict(db=1)))
    for tag, v in variants:
        if v.get("slice"):
            gy = al.displaced_slice(tuple(dy.shape), v["dy"], 1, Cout + 3, device=cuda, src=dya)
            dyv = gy.view
        else:
            dyv, gy = _operand(dy, v.get("dy", 0), cuda)
        xv, gx = _operand(x, v.get("x", 0), cuda, xp)
        gw = al.displaced_empty(tuple(w.shape), v["dw"], device=cuda) if "dw" in v else None
        gb = al.displaced_empty((Cout,), v["db"], device=cuda) if (bias and "db" in v) else None
        xf = kp.get("xform") if "x" not in v else None        # (the kept transform is that of the aligned x)
        dw, db = ops.conv2d_wgrad(dyv, xv, tuple(w.shape), s, p, d, need_bias=bias, dw=gw.view if gw else None,
                                  db=gb.view if gb else None, xform=xf)
        torch.cuda.synchronize()
        _intact(gy, gx, gw, gb)
        assert (gw is None or gw.unwritten() == 0) and (gb is None or gb.unwritten() == 0), tag
        err = rel_err(dw, dw64)
        print(f"wgrad {case} {name}: {tag} {err:.2e} / 2e-5")
        assert err <= 2e-5, (tag, err)
        if bias:
            assert rel_err(db, db64) < 1e-5, (tag, rel_err(db, db64))
        if tag in ("dw", "db"):
            assert torch.equal(dw, dw0), "a displaced dw / db changed the result (the split-K reduce adds in a fixed order)"
        if tag in ("dy", "x", "slice"):
            if name in al.WGRAD_LDS_DMA and "kept" not in flags:
                assert _sha(dw) == child["wgrad:" + _id(row)], f"a displaced {tag} did not run the register-staged family"
            elif name not in (al.STEM_WG,):
                # register-staged kernels, the gemv, and the batched Winograd path (its transform kernels read 4-byte
                # elements then, the GEMM its own workspace): the same bits
                assert torch.equal(dw, dw0), f"a displaced {tag} changed the bits"
            # (the stem kernel has 16-byte loads of dy only: a displaced dy runs the general kernels, held to fp64)


# ------------------------------------------------------------------ BatchNorm
BN_SHAPES = [(2, 5, 16, 16), (2, 5, 16, 64), (3, 33, 32, 32)]       # HW 256 / 1024: one chunk and several per channel


def _bn_inputs(shape, seed=7):
    g = torch.Generator().manual_seed(seed + shape[1])
    N, Cc, H, W = shape
    x = torch.randn(shape, generator=g) * 2 + 0.5
    gamma = torch.rand(Cc, generator=g) + 0.5
    beta = torch.randn(Cc, generator=g) * 0.1
    r = torch.randn(shape, generator=g)
    dy = torch.randn(shape, generator=g)
    return x, gamma, beta, r, dy


@pytest.mark.parametrize("shape", BN_SHAPES, ids=str)
def test_bn_kernels(cuda, shape):
    """bn_stats, bn_apply (+residual, +ReLU, slice and pitched out), bn_apply_relu_mask, bn_bwd_reduce, bn_bwd_apply and
    bn_bwd_fused, each tensor operand displaced in turn: the bits of the aligned call (a per-element or fixed-order
    kernel reads the same values 4 bytes at a time), which the fp64 figure of tests/test_ops_gpu.py then covers."""
    from dcfp_amd import ops
    N, Cc, H, W = shape
    assert (H * W) % 256 == 0
    x, gamma, beta, r, dy = _bn_inputs(shape)
    xd, rd, dyd = x.to(cuda), r.to(cuda), dy.to(cuda)
    gd, bd = gamma.to(cuda), beta.to(cuda)
    m0, v0 = ops.bn_stats(xd)
    m64, v64 = x.double().mean((0, 2, 3)), x.double().var((0, 2, 3), unbiased=False)
    assert max_err(m0, m64) < 1e-6 and max_err(v0, v64) < 1e-5
    for k in (1, 2, 3):
        xv, gx = _operand(x, k, cuda)
        m, v = ops.bn_stats(xv)
        torch.cuda.synchronize()
        _intact(gx)
        assert max_err(m, m64) < 1e-6 and max_err(v, v64) < 1e-5, k     # (another chunking of the sums: fp64 only)
    gs = al.displaced_slice(shape, 1, 1, Cc + 2, device=cuda, src=xd)     # a channel slice of a displaced concat
    m, v = ops.bn_stats(gs.view)
    assert max_err(m, m64) < 1e-6 and max_err(v, v64) < 1e-5 and gs.guards_intact()
    # -- apply
    y64 = torch.relu((x.double() - m0.double().cpu().view(1, -1, 1, 1)) / torch.sqrt(v0.double().cpu().view(1, -1, 1, 1) + 1e-5)
                     * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1) + r.double())
    y0 = ops.bn_apply(xd, m0, v0, gd, bd, 1e-5, rd, True)
    assert max_err(y0, y64) < 2e-5
    for kx, kr, ko, sl in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 1, 1), (1, 2, 3, 0), (0, 0, 2, 2)):
        xv, gx = _operand(x, kx, cuda)
        rv, gr = _operand(r, kr, cuda)
        go = None
        if sl == 1:
            go = al.displaced_slice(shape, ko, 1, Cc + 2, device=cuda)
        elif sl == 2:       # a row-pitched destination off the grid
            go = al.displaced_pitched(torch.zeros(shape, device=cuda), ko, W + 4)
        elif ko:
            go = al.displaced_empty(shape, ko, device=cuda)
        y = ops.bn_apply(xv, m0, v0, gd, bd, 1e-5, rv, True, out=go.view if go is not None else None)
        torch.cuda.synchronize()
        _intact(gx, gr, go)
        assert torch.equal(y, y0), (kx, kr, ko, sl)
        if sl == 2:         # the tails of the pitched rows stay zero
            full = go.view.as_strided((N, Cc, H, W + 4), go.view.stride(), go.view.storage_offset())
            assert float(full[..., W:].abs().max()) == 0.0
    ym0 = ops.bn_apply_relu_mask(xd, m0, v0, gd, bd, 1e-5, rd)
    assert ym0 is not None and torch.equal(ym0[0], y0)
    for kx, kr in ((1, 0), (0, 1), (2, 3)):
        xv, gx = _operand(x, kx, cuda)
        rv, gr = _operand(r, kr, cuda)
        ym = ops.bn_apply_relu_mask(xv, m0, v0, gd, bd, 1e-5, rv)
        torch.cuda.synchronize()
        _intact(gx, gr)
        # ("16-byte aligned rows": the wrapper answers None off the grid - its callers then run bn_apply and read the mask
        #  from y - or the same output and mask)
        assert ym is None or (torch.equal(ym[0], y0) and torch.equal(ym[1], ym0[1]))
    # -- backward: reduce, apply, fused, on every mask mode
    cnt = float(N * H * W)
    for relu, ysrc, want_res in ((0, None, False), (2, None, False), (1, y0, True), (3, ym0[1], True)):
        s10, s20, dg0 = ops.bn_bwd_reduce(dyd, xd, ysrc, m0, v0, gd, bd, 1e-5, relu)
        dx0, dr0 = ops.bn_bwd_apply(dyd, xd, ysrc, m0, v0, gd, bd, 1e-5, s10, s20, cnt, relu, want_res)
        f0 = ops.bn_bwd_fused(dyd, xd, ysrc, m0, v0, gd, bd, 1e-5, cnt, relu, want_res)
        assert f0 is not None and torch.equal(f0[3], dx0)
        for kdy, kx, ky in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 1, 2)):
            if ky and relu != 1:
                continue        # (y is read by mask mode 1 only; the bit mask of mode 3 is 8-byte words)
            dyv, gy = _operand(dy, kdy, cuda)
            xv, gx = _operand(x, kx, cuda)
            yv, gyy = (al.displaced(y0, ky).view, None) if (ky and relu == 1) else (ysrc, None)
            s1, s2, dg = ops.bn_bwd_reduce(dyv, xv, yv, m0, v0, gd, bd, 1e-5, relu)
            dx, dr = ops.bn_bwd_apply(dyv, xv, yv, m0, v0, gd, bd, 1e-5, s10, s20, cnt, relu, want_res)
            torch.cuda.synchronize()
            _intact(gy, gx)
            assert rel_err(s1, s10) < 1e-6 and rel_err(s2, s20) < 1e-6 and rel_err(dg, dg0) < 1e-6, (relu, kdy, kx, ky)
            assert torch.equal(dx, dx0) and (dr0 is None or torch.equal(dr, dr0)), (relu, kdy, kx, ky)
            # "needs 16-byte aligned tensors": the wrapper answers None (the caller's two-kernel path) or the same outputs
            f = ops.bn_bwd_fused(dyv, xv, yv, m0, v0, gd, bd, 1e-5, cnt, relu, want_res)
            torch.cuda.synchronize()
            if f is not None:
                assert torch.equal(f[3], dx0) and (dr0 is None or torch.equal(f[4], dr0))
        gs = al.displaced_slice(shape, 1, 2, Cc + 3, device=cuda, src=dyd)      # dy as a slice of a displaced wider tensor
        dx, dr = ops.bn_bwd_apply(gs.view, xd, ysrc, m0, v0, gd, bd, 1e-5, s10, s20, cnt, relu, want_res)
        assert torch.equal(dx, dx0) and gs.guards_intact()
    ops.check_fused_status()


@pytest.mark.parametrize("shape", BN_SHAPES, ids=str)
@pytest.mark.parametrize("relu,res", [(True, True), (False, False)])
def test_batch_norm_act_end_to_end(cuda, shape, relu, res):
    """ops.batch_norm_act forward and backward on displaced x / residual / dy, judged as
    tests/test_ops_gpu.py::test_bn_act_fwd_bwd judges the aligned call."""
    from dcfp_amd import ops
    N, Cc, H, W = shape
    x, gamma, beta, r, dy = _bn_inputs(shape)

    def ref():
        xx = x.double().requires_grad_(True); gg = gamma.double().requires_grad_(True); bb = beta.double().requires_grad_(True)
        rr = r.double().requires_grad_(True) if res else None
        rm, rv = torch.zeros(Cc, dtype=torch.float64), torch.ones(Cc, dtype=torch.float64)
        y = F.batch_norm(xx, rm, rv, gg, bb, True, 0.1, 1e-5)
        y = y + rr if res else y
        y = F.relu(y) if relu else y
        y.backward(dy.double())
        return y, xx.grad, gg.grad, bb.grad, (rr.grad if res else None), rm, rv

    y64, dx64, dg64, db64, dr64, rm64, rv64 = ref()
    for kx, kr, kdy in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 2, 3)):
        if kr and not res:
            continue
        gx, gr, gdy = al.displaced(x.to(cuda), kx), al.displaced(r.to(cuda), kr), al.displaced(dy.to(cuda), kdy)
        assert gx.view.data_ptr() % 16 == 4 * kx and gdy.view.data_ptr() % 16 == 4 * kdy
        xg = gx.view.requires_grad_(True)
        rg = gr.view.requires_grad_(True) if res else None
        gg, bg = gamma.to(cuda).requires_grad_(True), beta.to(cuda).requires_grad_(True)
        rmg, rvg = torch.zeros(Cc, device=cuda), torch.ones(Cc, device=cuda)
        yg = ops.batch_norm_act(xg, gg, bg, rmg, rvg, rg, relu, True, 0.1, 1e-5, False)
        yg.backward(gdy.view)
        torch.cuda.synchronize()
        assert gx.guards_intact() and gr.guards_intact() and gdy.guards_intact()
        assert max_err(yg, y64) < 2e-5
        assert max_err(rmg, rm64) < 1e-6 and max_err(rvg, rv64) < 1e-5
        assert rel_err(dg64, gg.grad) < 1e-4 and rel_err(db64, bg.grad) < 1e-4
        assert rel_err(dx64, xg.grad) < 1e-4
        if res:
            assert rel_err(dr64, rg.grad) < 1e-5
    ops.check_fused_status()


# ------------------------------------------------------------------ pool.hip
@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (2, 3, 32, 40)], ids=str)
def test_maxpool(cuda, shape):
    """Forward and backward through the C entry points (the wrapper allocates y and dx itself), x / y / dx displaced:
    equal to torch element by element, argmax route included."""
    from dcfp_amd import _lib, ops
    N, Cc, H, W = shape
    assert W % 8 == 0
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=g)
    x[0, 0, 0, :3] = float("-inf")
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 3, 2, 1)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    L, st = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    for kx, ky, kdy, kdx in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 2, 3, 1)):
        gx, gdy = al.displaced(x.to(cuda), kx), al.displaced(dy.to(cuda), kdy)
        gy, gdx = al.displaced_empty(tuple(y.shape), ky, device=cuda), al.displaced_empty(shape, kdx, device=cuda)
        idx = torch.empty(y.shape, dtype=torch.int32, device=cuda)
        assert gx.view.data_ptr() % 16 == 4 * kx and gy.view.data_ptr() % 16 == 4 * ky and gdx.view.data_ptr() % 16 == 4 * kdx
        _lib.check(L.dcfp_maxpool3x3s2_fwd_f32(P(gx.view), P(gy.view), P(idx), N, Cc, H, W, Ho, Wo, st), "maxpool_fwd")
        _lib.check(L.dcfp_maxpool3x3s2_bwd_f32(P(gdy.view), P(idx), P(gdx.view), N, Cc, H, W, Ho, Wo, st), "maxpool_bwd")
        torch.cuda.synchronize()
        _intact(gx, gy, gdy, gdx)
        assert gy.unwritten() == 0 and gdx.unwritten() == 0
        assert torch.equal(gy.view.cpu(), y.detach()), (kx, ky)
        assert max_err(gdx.view, xr.grad) < 1e-6, (kx, ky, kdy, kdx)
    xg = al.displaced(x.to(cuda), 1).view.requires_grad_(True)        # ... and the autograd node on a displaced x / dy
    yg = ops.maxpool3x3s2(xg)
    yg.backward(al.displaced(dy.to(cuda), 3).view)
    assert torch.equal(yg.cpu(), y.detach()) and max_err(xg.grad, xr.grad) < 1e-6


def test_small_pool_kernels(cuda):
    """rowsum, broadcast_hw (accumulate), add, channel_scale, global_avg_pool: bit-equal to the aligned call where the
    order is the same (everything but the row sums), the bound of tests/test_ops_gpu.py (1e-6) otherwise."""
    from dcfp_amd import ops
    g = torch.Generator().manual_seed(5)
    N, Cc, H, W = 2, 6, 16, 24
    x = torch.randn(N, Cc, H, W, generator=g)
    v = torch.randn(N, Cc, 1, 1, generator=g)
    m = torch.rand(N, Cc, generator=g)
    base = torch.randn(N, Cc, H, W, generator=g)
    xd = x.to(cuda)
    s64 = x.double().mean((2, 3), keepdim=True)
    assert max_err(ops.rowsum(xd, 1.0 / (H * W)), s64) < 1e-6
    assert max_err(ops.global_avg_pool(xd), x.double().mean((2, 3), keepdim=True)) < 1e-6
    for k in (1, 2, 3):
        gx = al.displaced(xd, k)
        assert max_err(ops.rowsum(gx.view, 1.0 / (H * W)), s64) < 1e-6      # (4-byte loads: another order of the sum)
        assert max_err(ops.global_avg_pool(gx.view), x.double().mean((2, 3), keepdim=True)) < 1e-6
        gs = al.displaced_slice((N, Cc, H, W), k, 1, Cc + 2, device=cuda, src=xd)
        assert max_err(ops.rowsum(gs.view, 1.0 / (H * W)), s64) < 1e-6
        assert gx.guards_intact() and gs.guards_intact()
        # broadcast_hw: write and accumulate, dense and slice destinations
        b0 = ops.broadcast_hw(v.to(cuda), H, W, 0.5)
        go = al.displaced_empty((N, Cc, H, W), k, device=cuda)
        assert torch.equal(ops.broadcast_hw(al.displaced(v.to(cuda), k).view, H, W, 0.5, out=go.view), b0)
        assert go.guards_intact() and go.unwritten() == 0
        acc0 = base.to(cuda).clone()
        ops.broadcast_hw(v.to(cuda), H, W, 0.5, out=acc0, accumulate=True)
        assert max_err(acc0, base.double() + 0.5 * v.double()) < 1e-6
        ga = al.displaced(base.to(cuda), k)
        ops.broadcast_hw(v.to(cuda), H, W, 0.5, out=ga.view, accumulate=True)
        assert torch.equal(ga.view, acc0) and ga.guards_intact(), "the 4-byte branch of broadcast_hw lost the accumulate"
        gsl = al.displaced_slice((N, Cc, H, W), k, 2, Cc + 3, device=cuda, src=base.to(cuda))
        ops.broadcast_hw(v.to(cuda), H, W, 0.5, out=gsl.view, accumulate=True)
        assert torch.equal(gsl.view, acc0) and gsl.guards_intact()
        # add, channel_scale
        a0 = ops.add(xd, base.to(cuda))
        for ka, kb in ((k, 0), (0, k), (k, (k % 3) + 1)):
            ga2, gb2 = al.displaced(xd, ka), al.displaced(base.to(cuda), kb)
            assert torch.equal(ops.add(ga2.view, gb2.view), a0) and ga2.guards_intact() and gb2.guards_intact()
        gd = al.displaced(xd, k)
        ops.add_into(gd.view, base.to(cuda))
        assert torch.equal(gd.view, a0) and gd.guards_intact()
        c0 = ops.ChannelScaleFn.apply(xd, m.to(cuda))
        assert torch.equal(c0.cpu(), x * m.view(N, Cc, 1, 1))
        gx2 = al.displaced(xd, k)
        assert torch.equal(ops.ChannelScaleFn.apply(gx2.view, al.displaced(m.to(cuda), k).view), c0) and gx2.guards_intact()


# ------------------------------------------------------------------ ppm.hip
def test_ppm_kernels(cuda):
    """ppm_pool (with its copy into a displaced destination), ppm_pool_adjoint and ppm_resize_adjoint at 16 x 32, judged
    as tests/test_psp_gpu.py judges the aligned calls."""
    from dcfp_amd import ops
    g = torch.Generator().manual_seed(13)
    N, Cc, H, W = 2, 5, 16, 32
    sizes = [1, 2, 3, 6]
    levels = [(s, s) for s in sizes]
    x = torch.randn(N, Cc, H, W, generator=g)
    xd = x.to(cuda)
    outs0 = ops.ppm_pool(xd, levels, True)
    for s, o in zip(sizes, outs0):
        ref = F.adaptive_avg_pool2d(x.double(), s)
        assert max_err(o, ref) <= 2e-6 * max(1.0, ref.abs().max().item())
    dp = torch.cat([torch.randn(N * Cc * s * s, generator=g) for s in sizes]).to(cuda)
    gfe = torch.randn(N, Cc, H, W, generator=g)
    x64 = x.double().requires_grad_(True)
    loss, off = (x64 * gfe.double()).sum(), 0
    for s in sizes:
        n = N * Cc * s * s
        loss = loss + (F.adaptive_avg_pool2d(x64, s) * dp[off:off + n].double().cpu().view(N, Cc, s, s)).sum()
        off += n
    loss.backward()
    dx0 = ops.ppm_pool_adjoint(dp, levels, (N, Cc, H, W), g=gfe.to(cuda))
    assert rel_err(dx0, x64.grad) <= 1e-6
    widths = [3, 2, 4, 1]
    dyc = torch.randn(N, sum(widths), H, W, generator=g)
    ps = [torch.zeros(N, c, s, s, dtype=torch.float64, requires_grad=True) for c, s in zip(widths, sizes)]
    cat = torch.cat([F.interpolate(p_, size=(H, W), mode="bilinear", align_corners=True) for p_ in ps], 1)
    (cat * dyc.double()).sum().backward()
    r0 = ops.ppm_resize_adjoint(dyc.to(cuda), widths, levels, True)
    for a, p_ in zip(r0, ps):
        assert rel_err(a, p_.grad) <= 1e-6
    for k in (1, 2, 3):
        gx = al.displaced(xd, k)
        gd = al.displaced_slice((N, Cc, H, W), k, 2, Cc + 3, device=cuda)
        outs = ops.ppm_pool(gx.view, levels, True, dst=gd.view)
        torch.cuda.synchronize()
        assert gx.guards_intact() and gd.guards_intact() and gd.unwritten() == 0
        assert torch.equal(gd.view, xd)                                       # the copy is bit-exact
        for s, o in zip(sizes, outs):
            ref = F.adaptive_avg_pool2d(x.double(), s)
            assert max_err(o, ref) <= 2e-6 * max(1.0, ref.abs().max().item())
        gg = al.displaced(gfe.to(cuda), k)
        gp = al.displaced(dp, (k % 3) + 1)
        dx = ops.ppm_pool_adjoint(gp.view, levels, (N, Cc, H, W), g=gg.view)
        assert torch.equal(dx, dx0) and gg.guards_intact() and gp.guards_intact()      # (per element: the same bits)
        gs = al.displaced_slice((N, Cc, H, W), k, 1, Cc + 2, device=cuda, src=gfe.to(cuda))
        assert torch.equal(ops.ppm_pool_adjoint(dp, levels, (N, Cc, H, W), g=gs.view), dx0)
        gy = al.displaced(dyc.to(cuda), k)
        r = ops.ppm_resize_adjoint(gy.view, widths, levels, True)
        assert all(torch.equal(a, b) for a, b in zip(r, r0)) and gy.guards_intact()     # fixed summation order


# ------------------------------------------------------------------ documented refusals still refuse
def test_documented_refusals(cuda):
    """dcfp_ohem_keep_mask_u8 with a displaced gt_prob and dcfp_gather_tiles_f32 with a displaced `tiles` return
    DCFP_E_BADDESC and write nothing."""
    from dcfp_amd import _lib
    L, st = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    n = 4096
    gp = al.displaced(torch.rand(n, device=cuda), 1)
    thr = torch.full((1,), 0.5, device=cuda)
    keep = torch.full((n,), 7, dtype=torch.uint8, device=cuda)
    assert L.dcfp_ohem_keep_mask_u8(P(gp.view), P(thr), n, P(keep), st) == _lib.E_BADDESC
    torch.cuda.synchronize()
    assert gp.guards_intact() and bool((keep == 7).all())
    ok = torch.rand(n, device=cuda)
    assert L.dcfp_ohem_keep_mask_u8(P(ok), P(thr), n, P(keep), st) == 0 and torch.equal(keep.bool(), ok <= thr)
    image = torch.randn(1, 3, 20, 24, device=cuda)
    ys, xs = (C.c_int32 * 2)(0, 8), (C.c_int32 * 2)(0, 8)
    gt = al.displaced_empty((4, 1, 3, 16, 16), 1, device=cuda)
    rc = L.dcfp_gather_tiles_f32(P(image), 1, 3, 20, 24, ys, 2, xs, 2, 16, 16, 0, P(gt.view), st)
    torch.cuda.synchronize()
    assert rc == _lib.E_BADDESC and gt.guards_intact() and gt.unwritten() == gt.view.numel()


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "--child":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    _child(sys.argv[2])
