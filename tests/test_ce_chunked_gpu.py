"""The cell kernel of the fused upsample + CE backward in class chunks (`ce_bwd_cells_kernel<ALIGN, kCeChunk>`, every
class count but 19; 19 is the same kernel with one chunk of 19): fp64 parity, exact independence of the class chunks,
determinism, equal bits of the plain and the weighted route, the plan query and the `DCFP_CE_BWD_CELLS=0` route.

Class counts are placed around the chunk width CT, read from `ops.ce_backward_plan`: CT+1 (a tail chunk of one class),
2CT-1 (a tail chunk one short), 2CT (no tail), 2CT+1, and the datasets' 59 / 150 / 171.  Geometries stress the 7 x 15
tile of low-resolution outputs: one source pixel, exactly one tile, one row / column past it, non-integer ratios over
several tiles, the identity, a fully ignored image.

Tolerance, the rule of test_loss_eval_kernels_gpu.py: the kernel's norm-relative distance to the fp64 reference is at
most max(floor, 3 x yardstick); yardstick = the distance of the same formula evaluated by torch in fp32 on the same
inputs; floor 3e-5 for the CE gradients, 2e-5 for the GSRL criterion's.  Every comparison prints one `PARITY` line."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

IGN = 255
CE_GFLOOR, GSRL_GFLOOR = 3e-5, 2e-5
PLAN_SHAPE = (2, 8, 16, 64, 128)           # N, h, w, H, W of the plan queries that only ask for CT

# (N, h, w, H, W, align_corners, index of a fully ignored image or -1)
GEOMS = [
    (2, 1, 1, 9, 11, True, -1),            # one source pixel: scale 0 under align
    (2, 7, 15, 56, 120, True, -1),         # x8, exactly one 7 x 15 tile
    (2, 8, 16, 64, 128, False, -1),        # one row / column past the tile: 2 x 2 tiles
    (2, 15, 46, 97, 301, True, -1),        # non-integer ratio, 3 x 4 tiles
    (1, 14, 31, 120, 250, False, -1),      # non-integer ratio, 2 x 3 tiles, batch of one
    (2, 14, 30, 14, 30, True, -1),         # the identity, 2 x 2 full tiles
    (3, 9, 17, 40, 70, False, 1),          # one fully ignored image
]
COUNTS = ["CT+1", "2CT-1", "2CT", "2CT+1", "59", "150", "171"]


def _ct():
    from dcfp_amd import ops
    N, h, w, H, W = PLAN_SHAPE
    variant, ct, chunks = ops.ce_backward_plan(N, 59, h, w, H, W)
    assert variant == "cells_chunked" and ct > 1 and chunks == -(-59 // ct), (variant, ct, chunks)
    return ct


def _count(name, ct):
    return {"CT+1": ct + 1, "2CT-1": 2 * ct - 1, "2CT": 2 * ct, "2CT+1": 2 * ct + 1}.get(name) or int(name)


def _seed(*parts):
    return random.Random(repr(parts)).getrandbits(31)


def _up(z, size, align):
    return F.interpolate(z, size=size, mode="bilinear", align_corners=align)


def _nrel(a, b):
    a = a.double().cpu(); b = b.double().cpu()
    d, n = float((a - b).norm()), float(b.norm())
    return d / n if n > 0 else d


def _held(group, case, err, yard, floor):
    bound = max(floor, 3.0 * yard)
    msg = f"PARITY {group} {case} dlogits: kernel {err:.3e} fp32-yardstick {yard:.3e} bound {bound:.3e}"
    print(msg)
    assert err <= bound, msg


def _inputs(geom, Cc, seed, lo=0, hi=None):
    """logits, labels uniform in [lo, hi) with ~15 % ignored (and the geometry's ignored image)"""
    N, h, w, H, W, align, dead = geom
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, Cc, h, w, generator=g) * 2.5
    lab = torch.randint(lo, Cc if hi is None else hi, (N, H, W), generator=g)
    lab[torch.rand(N, H, W, generator=g) < 0.15] = IGN
    if dead >= 0:
        lab[dead] = IGN
    return g, z, lab


def _keep_case(dev, geom, Cc, seed, lo=0, hi=None):
    """plain CE with a pixel_keep mask -> (kernel error, fp32 yardstick, finite and zero where it must be)"""
    from dcfp_amd import ops
    N, h, w, H, W, align, dead = geom
    g, z, lab = _inputs(geom, Cc, seed, lo, hi)
    keep = (torch.rand(N, H, W, generator=g) < 0.6).to(torch.uint8)
    if not bool(((keep != 0) & (lab != IGN)).any()):
        keep.view(-1)[int((lab.view(-1) != IGN).nonzero()[0])] = 1

    def ref(dt):
        zr = z.detach().clone().to(dt).requires_grad_(True)
        relabelled = lab.clone()
        relabelled[keep == 0] = IGN
        F.cross_entropy(_up(zr, (H, W), align), relabelled, ignore_index=IGN).backward()
        return zr.grad
    g64, g32 = ref(torch.float64), ref(torch.float32)
    zg = z.to(dev).requires_grad_(True)
    ops.upsample_cross_entropy(zg, lab.to(dev), (H, W), align, IGN, pixel_keep=keep.to(dev)).backward()
    ok = bool(torch.isfinite(zg.grad).all()) and (dead < 0 or bool((zg.grad[dead] == 0).all()))
    return _nrel(zg.grad, g64), _nrel(g32, g64), ok


def _wce_case(dev, geom, Cc, seed, lo=0, hi=None):
    """weighted CE under a different upstream gradient per image -> the same triple"""
    from dcfp_amd import ops
    N, h, w, H, W, align, dead = geom
    g, z, lab = _inputs(geom, Cc, seed, lo, hi)
    wgt = torch.rand(lab.shape, generator=g) * 2.0 + 0.05
    wgt[torch.rand(lab.shape, generator=g) < 0.3] = 0.0
    coef = torch.rand(N, generator=g) + 0.5

    def ref(dt):
        zr = z.detach().clone().to(dt).requires_grad_(True)
        l = F.cross_entropy(_up(zr, (H, W), align), lab, ignore_index=IGN, reduction="none")
        ((l * wgt.to(dt)).sum(dim=(1, 2)) * coef.to(dt)).sum().backward()
        return zr.grad
    g64, g32 = ref(torch.float64), ref(torch.float32)
    zg = z.to(dev).requires_grad_(True)
    out = ops.upsample_weighted_ce(zg, lab.to(dev), wgt.to(dev), (H, W), align, IGN)
    (out[:, 0] * coef.to(dev)).sum().backward()
    ok = bool(torch.isfinite(zg.grad).all()) and (dead < 0 or bool((zg.grad[dead] == 0).all()))
    return _nrel(zg.grad, g64), _nrel(g32, g64), ok


_KINDS = {"keep": _keep_case, "wce": _wce_case}


def _gid(geom):
    N, h, w, H, W, align, dead = geom
    return f"{N}x{h}x{w}-{H}x{W}-a{int(align)}" + (f"-dead{dead}" if dead >= 0 else "")


# every geometry with every class count; the kind alternates, so that each geometry and each count meets both
PARITY_CASES = [(g, c, ["keep", "wce"][(i + j) % 2]) for i, g in enumerate(GEOMS) for j, c in enumerate(COUNTS)]


@pytest.mark.parametrize("geom,count,kind", PARITY_CASES, ids=[f"{_gid(g)}-C{c}-{k}" for g, c, k in PARITY_CASES])
def test_fp64_parity(cuda, geom, count, kind):
    from dcfp_amd import ops
    ct = _ct()
    Cc = _count(count, ct)
    N, h, w, H, W, _, _ = geom
    assert ops.ce_backward_plan(N, Cc, h, w, H, W) == ("cells_chunked", ct, -(-Cc // ct))
    err, yard, ok = _KINDS[kind](cuda, geom, Cc, _seed("parity", geom, count, kind))
    _held(kind, f"{_gid(geom)}-C{Cc}", err, yard, CE_GFLOOR)
    assert ok, "gradient not finite, or a fully ignored image with a non-zero gradient"


@pytest.mark.parametrize("kind", ["keep", "wce"])
@pytest.mark.parametrize("where", ["tail", "chunk0"])
@pytest.mark.parametrize("count", ["2CT+1", "59", "171"])
def test_labels_in_one_chunk(cuda, count, where, kind):
    """every label in the tail chunk (whose phantom classes must stay out of it), or every label in chunk 0"""
    ct = _ct()
    Cc = _count(count, ct)
    tail0 = (Cc - 1) // ct * ct
    lo, hi = (tail0, Cc) if where == "tail" else (0, ct)
    geom = GEOMS[2]
    err, yard, ok = _KINDS[kind](cuda, geom, Cc, _seed("one-chunk", count, where, kind), lo, hi)
    _held(kind, f"{_gid(geom)}-C{Cc}-labels-{where}", err, yard, CE_GFLOOR)
    assert ok


class _DS:
    ignore_label = IGN; num_classes = 59; class_weights = None


@pytest.mark.parametrize("Cc", [59, 171])
def test_gsrl_criterion(cuda, Cc):
    """the whole GSRL criterion (main + deep-supervision head, two launches of the weighted backward) against fp64"""
    from dcfp_amd.loss.criterion import build_criterions
    from oracle.gsrl import gsrl_loss
    geom = GEOMS[4]
    N, h, w, H, W, align, _ = geom
    g, z0, lab = _inputs(geom, Cc, _seed("gsrl", Cc))
    zs = [z0, torch.randn(z0.shape, generator=g) * 1.5]
    bal = torch.rand(N, H, W, generator=g) * 2.0 + 0.1
    bal[torch.rand(N, H, W, generator=g) < 0.6] = 0.0

    def ref(dt):
        zr = [t.detach().clone().to(dt).requires_grad_(True) for t in zs]
        gsrl_loss([_up(t, (H, W), align) for t in zr], lab, bal.to(dt), IGN, 0.4, 3, 9).backward()
        return [t.grad for t in zr]
    g64, g32 = ref(torch.float64), ref(torch.float32)
    crit = build_criterions("gsrl", _DS(), {"ds_weight": 0.4, "k": 3, "gamma": 9})
    zg = [t.to(cuda).requires_grad_(True) for t in zs]
    crit.forward_lowres(zg, {"ori": lab.to(cuda), "weight": bal.to(cuda)}, (H, W), align)["loss"].backward()
    for i in range(2):
        _held("gsrl", f"{_gid(geom)}-C{Cc}-head{i}", _nrel(zg[i].grad, g64[i]), _nrel(g32[i], g64[i]), GSRL_GFLOOR)
        assert torch.isfinite(zg[i].grad).all()


# ------------------------------------------------------------------------------ the C entry points, called directly
def _direct(dev, kind, z, lab, lse, extra, scale, size, align, fill=float("nan")):
    """dcfp_upsample_{ce,wce}_bwd_f32 on a given lse map; the output buffer starts as `fill`"""
    from dcfp_amd import _lib
    N, Cc, h, w = z.shape
    H, W = size
    dl = torch.full(z.shape, fill, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = _lib.lib().dcfp_upsample_ce_bwd_f32 if kind == "keep" else _lib.lib().dcfp_upsample_wce_bwd_f32
    _lib.check(fn(p(z), p(lab), p(extra), IGN, N, Cc, h, w, H, W, int(align), p(lse), p(scale), p(dl), st), kind)
    torch.cuda.synchronize()
    return dl


def _direct_inputs(dev, kind, geom, Cc, seed):
    from dcfp_amd import ops
    N, h, w, H, W, align, _ = geom
    g, z, lab = _inputs(geom, Cc, seed)
    z, lab = z.to(dev).contiguous(), lab.to(dev).contiguous()
    _, lse, _ = ops.upsample_ce_forward(z, lab, (H, W), align, IGN)
    if kind == "keep":
        extra = (torch.rand(N, H, W, generator=g) < 0.6).to(torch.uint8).to(dev)
        scale = torch.full((1,), 1.0 / (N * H * W), dtype=torch.float32, device=dev)
    else:
        extra = (torch.rand(N, H, W, generator=g) * 2.0).to(dev)
        scale = (torch.rand(N, generator=g) + 0.5).to(dev)
    return z, lab, lse, extra, scale


@pytest.mark.parametrize("kind", ["keep", "wce"])
@pytest.mark.parametrize("count", ["2CT+1", "59"])
def test_chunk_isolation_exact(cuda, count, kind):
    """With the lse map fixed, a chunk's gradient is a function of its own logits only: perturbing chunk 0 leaves
    every other chunk bit-identical, and perturbing the tail chunk leaves every chunk before it bit-identical."""
    ct = _ct()
    Cc = _count(count, ct)
    tail0 = (Cc - 1) // ct * ct
    geom = GEOMS[3]
    size, align = (geom[3], geom[4]), geom[5]
    z, lab, lse, extra, scale = _direct_inputs(cuda, kind, geom, Cc, _seed("isolation", count, kind))
    base = _direct(cuda, kind, z, lab, lse, extra, scale, size, align)
    assert torch.isfinite(base).all()
    for lo, hi in ((0, ct), (tail0, Cc)):
        z2 = z.clone()
        z2[:, lo:hi] += 0.37
        got = _direct(cuda, kind, z2, lab, lse, extra, scale, size, align)
        inside = torch.zeros(Cc, dtype=torch.bool, device=cuda)
        inside[lo:hi] = True
        assert torch.equal(got[:, ~inside], base[:, ~inside]), (lo, hi)
        assert not torch.equal(got[:, inside], base[:, inside]), (lo, hi)      # the perturbation did reach the kernel


@pytest.mark.parametrize("kind", ["keep", "wce"])
@pytest.mark.parametrize("count", ["CT+1", "171"])
def test_deterministic_and_fully_written(cuda, count, kind):
    Cc = _count(count, _ct())
    geom = GEOMS[3]
    size, align = (geom[3], geom[4]), geom[5]
    args = _direct_inputs(cuda, kind, geom, Cc, _seed("determinism", count, kind))
    a = _direct(cuda, kind, *args, size, align)
    b = _direct(cuda, kind, *args, size, align)
    assert not torch.isnan(a).any() and not torch.isnan(b).any()       # the buffer started as NaN: every element written
    assert torch.equal(a, b)


@pytest.mark.parametrize("count", ["19", "CT+1", "59"])
@pytest.mark.parametrize("geom", [GEOMS[2], GEOMS[3]], ids=_gid)
def test_keep_and_weighted_routes_equal_bits(cuda, geom, count):
    """Plain CE without a keep mask and weighted CE under an all-ones weight map and one scale for every image are the
    same function; both entry points go through one launcher and one kernel, where the weight multiplies by exactly 1:
    their dlogits are the same bits."""
    Cc = _count(count, _ct())
    N, h, w, H, W, align, _ = geom
    z, lab, lse, _, _ = _direct_inputs(cuda, "keep", geom, Cc, _seed("routes", _gid(geom), count))
    ones = torch.ones((N, H, W), dtype=torch.float32, device=cuda)
    scale = torch.full((N,), 1.0 / (N * H * W), dtype=torch.float32, device=cuda)
    plain = _direct(cuda, "keep", z, lab, lse, None, scale[:1], (H, W), align)
    weighted = _direct(cuda, "wce", z, lab, lse, ones, scale, (H, W), align)
    assert torch.isfinite(plain).all() and bool((plain != 0).any())
    assert torch.equal(plain, weighted)


# ------------------------------------------------------------------------------------------------------ the plan
def test_plan(cuda):
    from dcfp_amd import ops
    N, h, w, H, W = PLAN_SHAPE
    ct = _ct()
    assert ops.ce_backward_plan(N, 19, h, w, H, W) == ("cells19", 19, 1)
    for Cc in (59, 150, 171):
        assert ops.ce_backward_plan(N, Cc, h, w, H, W) == ("cells_chunked", ct, -(-Cc // ct))
    with pytest.raises(RuntimeError):
        ops.ce_backward_plan(0, 59, h, w, H, W)


def test_c19_control(cuda):
    """C == 19 keeps its own instantiation (`cells19`: one chunk of 19 classes, no tail), held to fp64 as before"""
    from dcfp_amd import ops
    geom = GEOMS[2]
    N, h, w, H, W, _, _ = geom
    assert ops.ce_backward_plan(N, 19, h, w, H, W) == ("cells19", 19, 1)
    for kind in ("keep", "wce"):
        err, yard, ok = _KINDS[kind](cuda, geom, 19, _seed("control", kind))
        _held(kind, f"{_gid(geom)}-C19", err, yard, CE_GFLOOR)
        assert ok


def _child():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from dcfp_amd import ops
    assert os.environ.get("DCFP_CE_BWD_CELLS") == "0"
    dev = torch.device("cuda:0")
    geom = GEOMS[2]
    N, h, w, H, W, _, _ = geom
    out = {}
    for Cc in (59, 150, 171):
        out[str(Cc)] = {"plan": ops.ce_backward_plan(N, Cc, h, w, H, W),
                        "keep": _keep_case(dev, geom, Cc, _seed("cells0", Cc, "keep")),
                        "wce": _wce_case(dev, geom, Cc, _seed("cells0", Cc, "wce"))}
    out["19"] = {"plan": ops.ce_backward_plan(N, 19, h, w, H, W)}
    torch.cuda.synchronize()
    print("CE_CHUNKED_RESULT " + json.dumps(out))


def test_cells_off_selects_per_output(cuda):
    """DCFP_CE_BWD_CELLS=0 (read once per process: a fresh child): the per-output kernels at every class count, still
    within the fp64 bound"""
    env = dict(os.environ, DCFP_CE_BWD_CELLS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("CE_CHUNKED_RESULT ")][-1]
    res = json.loads(line[len("CE_CHUNKED_RESULT "):])
    assert sorted(res) == ["150", "171", "19", "59"]
    for Cc, item in res.items():
        assert item["plan"] == ["per_output", 0, 0], (Cc, item["plan"])
        for kind in ("keep", "wce"):
            if kind in item:
                err, yard, ok = item[kind]
                _held(f"{kind}-cells0", f"{_gid(GEOMS[2])}-C{Cc}", err, yard, CE_GFLOOR)
                assert ok


if __name__ == "__main__" and len(sys.argv) == 2 and sys.argv[1] == "--child":
    _child()
