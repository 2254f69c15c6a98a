"""The Winograd paths on ragged maps (H or W no multiple of 2d): tiles without an output inside the image are not
enumerated, and in the fused forward / dgrad kernel tiles whose second output row / column lies outside the image run
12 or 9 of the 16 components (csrc/wino_plan.h, conv_winograd2.hip).  For every shape forward, dgrad, accumulate-dgrad
and the weight gradient are checked against an fp64 CPU conv at the tolerances of tests/test_conv_large_gpu.py, and
forward / dgrad / accumulate-dgrad must be the SAME BITS as a run with DCFP_WINO_RAGGED=0 (the full grid, all 16
components): the valid outputs keep their operations and their order.  The weight gradient's split-K chunks move with
the tile count, so it is only bit-equal where the plan does not change (the control shape).

The library latches its switches on first use: each setting runs once, in a child process, for all cases."""
import math
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

N = 2
CASES = {
    # name: (Cin, Cout, H, W, d, pitched)
    "d4_10x20": (64, 64, 10, 20, 4, False),        # all four component classes, plus empty tile rows
    "d6_14x32": (64, 64, 14, 32, 6, False),        # the full / half column boundary (13) is rounded up to the quads
    "d2_9x12_pitched": (64, 64, 9, 12, 2, True),
    "d1_7x12_pitched": (64, 64, 7, 12, 1, True),
    "d4_16x16_control": (64, 64, 16, 16, 4, False),     # no half or empty tiles: the plan is the full grid
    "d4_10x20_c56_m72": (56, 72, 10, 20, 4, False),    # channel counts off the 64-blocks and the 16-channel K-steps
}
CONTROL = "d4_16x16_control"


def _inputs(name):
    import torch
    Cin, Cout, H, W, d, _ = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    x = torch.randn(N, Cin, H, W, generator=g)
    x = torch.relu(x) + 0.05 * x
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    dy = torch.randn(N, Cout, H, W, generator=g) * 1e-2
    seed = torch.randn(N, Cin, H, W, generator=g)
    return x, w, dy, seed


def _child(path):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from dcfp_amd import _lib, ops
    dev = torch.device("cuda:0")
    out = {}
    for name, (Cin, Cout, H, W, d, pitched) in CASES.items():
        x, w, dy, seed = (t.to(dev) for t in _inputs(name))
        xin, dyin, pitch = x, dy, 0
        if pitched:
            pitch = ops.conv_pitch(tuple(x.shape), tuple(w.shape), 1, d, d)
            assert pitch, name
            xin = ops.new_pitched(tuple(x.shape), pitch, dev); xin.copy_(x)
            dyin = ops.new_pitched(tuple(dy.shape), pitch, dev); dyin.copy_(dy)
        desc = ops._desc(x.shape, w.shape, 1, d, d, pitch, pitch)
        names = [ops.conv_kernel_name(desc, k) for k in (_lib.CONV_FWD, _lib.CONV_DGRAD, _lib.CONV_WGRAD)]
        y = ops.conv2d_fwd(xin, w, None, 1, d, d)
        dx = ops.conv2d_dgrad(dyin, w, tuple(x.shape), 1, d, d)
        dxa = seed.clone()
        ops.conv2d_dgrad(dyin, w, tuple(x.shape), 1, d, d, out=dxa, accumulate=True)
        dw = ops.conv2d_wgrad(dyin, xin, tuple(w.shape), 1, d, d)[0]
        torch.cuda.synchronize()
        out[name] = {"kernels": names, "y": y.cpu(), "dx": dx.cpu(), "dxa": dxa.cpu(), "dw": dw.cpu(),
                     "frac": [ops.conv_executed_fraction(desc, k) for k in (_lib.CONV_FWD, _lib.CONV_DGRAD, _lib.CONV_WGRAD)]}
    torch.save(out, path)


_RUNS = {}


def _run(tmp_path_factory, ragged):
    """One child process per setting, for all cases; DCFP_CONV_WINOGRAD=2 takes the Winograd kernels wherever they apply."""
    import torch
    if ragged not in _RUNS:
        path = str(tmp_path_factory.mktemp("wino_ragged") / f"ragged{ragged}.pt")
        env = dict(os.environ, DCFP_WINO_RAGGED=ragged, DCFP_CONV_WINOGRAD="2", DCFP_WINO_FUSED="2", DCFP_WINO_WGRAD_FUSED="2",
                   DCFP_CONV_MATH="f32")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _RUNS[ragged] = torch.load(path)
    return _RUNS[ragged]


_REF = {}


def _reference(name):
    """fp64 CPU conv, once per case."""
    import torch
    import torch.nn.functional as F
    if name not in _REF:
        d = CASES[name][4]
        x, w, dy, seed = _inputs(name)
        x64 = x.double().requires_grad_(True)
        w64 = w.double().requires_grad_(True)
        y64 = F.conv2d(x64, w64, None, 1, d, d)
        y64.backward(dy.double())
        _REF[name] = (y64.detach(), x64.grad, x64.grad + seed.double(), w64.grad)
    return _REF[name]


def _rel(a, b):
    return ((a.double() - b).norm() / b.norm()).item()


@pytest.mark.parametrize("name", list(CASES))
def test_ragged_map_against_fp64_and_the_full_grid(cuda, tmp_path_factory, name):
    import torch
    Cin, Cout, H, W, d, pitched = CASES[name]
    new, old = _run(tmp_path_factory, "1")[name], _run(tmp_path_factory, "0")[name]
    for res in (new, old):       # the Winograd kernels ran: fused forward / dgrad, fused weight gradient
        assert res["kernels"][0].startswith("winograd_f2x2_3x3 fused"), res["kernels"]
        assert res["kernels"][1].startswith("winograd_f2x2_3x3 fused"), res["kernels"]
        assert res["kernels"][2].startswith("winograd_f2x2_3x3 wgrad fused"), res["kernels"]
    y64, dx64, dxa64, dw64 = _reference(name)
    tol = 3e-6 * max(1.0, math.sqrt(Cin * 9) / 8)           # tests/test_conv_large_gpu.py:276-292
    errs = {k: (_rel(new[k], ref), _rel(old[k], ref)) for k, ref in (("y", y64), ("dx", dx64), ("dxa", dxa64), ("dw", dw64))}
    print(name, "rel-L2 vs fp64 (ragged, full grid):", errs, "executed fraction:", new["frac"], old["frac"])
    for res in (new, old):
        assert _rel(res["y"], y64) < tol
        assert _rel(res["dx"], dx64) < max(tol, 1e-5)
        assert _rel(res["dxa"], dxa64) < max(tol, 1e-5)
        assert _rel(res["dw"], dw64) < 2e-5
    assert torch.equal(new["y"], old["y"])
    assert torch.equal(new["dx"], old["dx"])
    assert torch.equal(new["dxa"], old["dxa"])
    if name == CONTROL:
        assert torch.equal(new["dw"], old["dw"])
        assert new["frac"] == old["frac"]
    else:                        # no more tiles enumerated than the full grid has (fewer where it has empty ones)
        assert all(a <= b for a, b in zip(new["frac"], old["frac"])), (new["frac"], old["frac"])


if __name__ == "__main__" and "--child" in sys.argv:
    _child(sys.argv[sys.argv.index("--child") + 1])
