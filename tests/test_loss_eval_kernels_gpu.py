"""Per-kernel fp64 parity of the loss / evaluation kernels of `upsample_ce.hip` and `ohem.hip`: GSRL margin, k x k max
filter, per-pixel-weighted CE (forward, both outputs, gradient under per-image upstream gradients), the whole GSRL
criterion, CE with a `pixel_keep` mask, the OHEM zoom and keep-mask kernels, the fused argmax and the confusion matrix.

Shapes come from the kernel geometry: the 19-class cell kernel's 7 x 15 tile of low-resolution outputs (heights 1, 2, 7,
8, 14, 15, widths 1, 2, 15, 16, 30, 31, 46, several tile rows and columns at once), both `align_corners`, integer /
non-integer ratios and ratios above 16, the identity, one-pixel outputs under align (scale 0), class counts on both sides
of the C == 19 register kernels, ~15 % ignored labels, one fully ignored image, a batch of one, and sizes that take every
grid-stride loop round twice.

Tolerance of the float-valued groups: the kernel's distance to the fp64 reference must be within
max(floor, 3 x yardstick), yardstick = the distance of the SAME formula evaluated by torch in fp32 on the same inputs
(what fp32 arithmetic of this formula costs; factor 3 as everywhere in this suite), floor = the tolerance of the nearest
existing comparison (CE 3e-6 loss / 3e-5 gradient, GSRL 2e-6 / 2e-5, a probability 2e-6 absolute).  Every comparison
prints `PARITY <group> <case> <what> err yardstick bound`.  Exact groups (max filter, keep mask, confusion matrix, zoomed
labels, argmax ties) use `equal`."""
import ctypes as C
import json
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

IGN = 255
CLASSES = [19, 1, 2, 7, 20, 60, 150]       # 19: the register kernels; 20: the generic path next to them

# (N, h, w, H, W, align_corners, index of a fully ignored image or -1)
GEOMS = [
    (2, 1, 1, 9, 11, True, -1),            # one source pixel: scale 0 under align
    (2, 1, 15, 1, 120, True, -1),          # H == 1 under align; exactly one tile column, x8
    (3, 7, 1, 50, 1, True, 1),             # W == 1 under align; exactly one tile row
    (2, 2, 2, 40, 70, False, -1),          # x20 / x35: a cell owns far more than 8 x 8 pixels
    (1, 2, 1, 35, 18, False, -1),          # batch of one, x17.5 / x18
    (2, 1, 2, 8, 16, False, 0),            # x8
    (2, 7, 15, 56, 120, True, -1),         # x8, exactly one 7 x 15 tile
    (2, 8, 16, 64, 128, False, 1),         # x8, one row / column past the tile: 2 x 2 tiles
    (2, 14, 30, 14, 30, True, -1),         # identity (CriterionDSN.forward), 2 x 2 full tiles
    (3, 15, 31, 15, 31, False, 2),         # identity, 3 x 3 tiles, the last ones one wide / high
    (2, 15, 46, 97, 301, True, 0),         # non-integer ratio, 3 tile rows x 4 tile columns
    (1, 14, 31, 120, 250, False, -1),      # non-integer ratio, 2 x 3 tiles, batch of one
    (2, 8, 30, 140, 500, True, -1),        # x17.5 / x16.7 across 2 x 2 tiles
    (2, 7, 46, 56, 368, False, -1),        # x8, 1 x 4 tiles
    (2, 2, 16, 33, 130, True, -1),         # x16.5 / x8.1, 1 x 2 tiles
]


def _cid(geom, Cc):
    N, h, w, H, W, align, dead = geom
    return f"{N}x{Cc}x{h}x{w}-{H}x{W}-a{int(align)}" + (f"-dead{dead}" if dead >= 0 else "")


def _cycled(shift, skip=()):
    """every geometry with a class count, cycling through CLASSES (15 geometries: every count at least twice)."""
    out = []
    for i, g in enumerate(GEOMS):
        Cc = CLASSES[(i + shift) % len(CLASSES)]
        out.append((g, 19 if Cc in skip else Cc))
    return out


def _with_19(shift):
    """every geometry at C == 19 (the register kernels) and at one other class count."""
    others = [c for c in CLASSES if c != 19]
    return [(g, 19) for g in GEOMS] + [(g, others[(i + shift) % len(others)]) for i, g in enumerate(GEOMS)]


def _ids(cases):
    return [_cid(g, c) for g, c in cases]


def _seed(*parts):
    return random.Random(repr(parts)).getrandbits(31)


def _up(z, size, align):
    return F.interpolate(z, size=size, mode="bilinear", align_corners=align)


def _inputs(geom, Cc, seed):
    N, h, w, H, W, align, dead = geom
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(N, Cc, h, w, generator=g) * 2.5
    lab = torch.randint(0, Cc, (N, H, W), generator=g)
    lab[torch.rand(N, H, W, generator=g) < 0.15] = IGN
    if dead >= 0:
        lab[dead] = IGN
    return g, z, lab


def _abs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max()) if a.numel() else 0.0


def _rel1(a, b):
    """largest |a - b| / max(1, |b|): the form of the suite's loss comparisons"""
    a = a.double().cpu().reshape(-1); b = b.double().cpu().reshape(-1)
    return float(((a - b).abs() / b.abs().clamp(min=1.0)).max())


def _nrel(a, b):
    """norm-relative distance (absolute where the reference is exactly zero)"""
    a = a.double().cpu(); b = b.double().cpu()
    d, n = float((a - b).norm()), float(b.norm())
    return d / n if n > 0 else d


def _held(group, case, what, err, yard, floor):
    bound = max(floor, 3.0 * yard)
    msg = f"PARITY {group} {case} {what}: kernel {err:.3e} fp32-yardstick {yard:.3e} bound {bound:.3e}"
    print(msg)
    assert err <= bound, msg


CE_FLOOR, CE_GFLOOR = 3e-6, 3e-5          # test_random_upsample_ce
GSRL_FLOOR, GSRL_GFLOOR = 2e-6, 2e-5      # test_gsrl_loss_vs_reference_golden
PROB_FLOOR = 2e-6                         # th_gpu in the OHEM tests


# ---------------------------------------------------------------------------------------------------- 1. margin
def _margin_ref(z, size, align, dt):
    p = torch.softmax(_up(z.to(dt), size, align), 1)
    if p.shape[1] == 1:
        return p[:, 0]                     # no second class: p1 - 0 = 1
    top = p.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def _margin_check(cuda, z, size, align, case):
    from dcfp_amd import ops
    got = ops.upsample_margin(z.to(cuda), size, align).cpu()
    ref = _margin_ref(z, size, align, torch.float64)
    assert tuple(got.shape) == tuple(ref.shape)
    _held("margin", case, "p1-p2", _abs(got, ref), _abs(_margin_ref(z, size, align, torch.float32), ref), PROB_FLOOR)
    return got


MARGIN_CASES = _cycled(0)


@pytest.mark.parametrize("geom,Cc", MARGIN_CASES, ids=_ids(MARGIN_CASES))
def test_margin(cuda, geom, Cc):
    N, h, w, H, W, align, _ = geom
    _, z, _ = _inputs(geom, Cc, _seed("margin", geom, Cc))
    got = _margin_check(cuda, z, (H, W), align, _cid(geom, Cc))
    if Cc == 1:
        assert torch.equal(got, torch.ones_like(got))


@pytest.mark.parametrize("align", [True, False])
def test_margin_exact_top2_tie(cuda, align):
    """Two classes share the largest logit plane: their interpolated logits are the same fp32 expression of the same
    values, so p1 == p2 and the margin is exactly 0 on every pixel."""
    g = torch.Generator().manual_seed(_seed("margin-tie", align))
    z = torch.randn(2, 7, 8, 16, generator=g) * 2.5
    z[:, 4] = z.amax(1) + 0.75
    z[:, 2] = z[:, 4]
    got = _margin_check(cuda, z, (61, 130), align, f"tie-a{int(align)}")
    assert torch.equal(got, torch.zeros_like(got))


def test_margin_grid_stride(cuda):
    """N*H*W = 1 064 960 > 4096 x 256 threads: the launch goes round its loop twice."""
    g = torch.Generator().manual_seed(_seed("margin-large"))
    z = torch.randn(2, 7, 80, 104, generator=g) * 2.5
    assert 2 * 640 * 832 > 4096 * 256
    _margin_check(cuda, z, (640, 832), True, "2x7x80x104-640x832")


# ------------------------------------------------------------------------------------------------ 2. max filter
@pytest.mark.parametrize("k", [1, 3, 5, 9, 15])
@pytest.mark.parametrize("shape", [(2, 33, 47), (1, 1, 40), (3, 40, 1), (2, 1, 1), (2, 4, 6), (1, 3, 20), (1, 20, 7),
                                   (1, 8, 8), (2, 14, 15)], ids=lambda s: "x".join(map(str, s)))
def test_maxfilter(cuda, shape, k):
    """maps smaller than k in one or both directions, one row / one column, +-inf entries; no rounding: equal."""
    from dcfp_amd import ops
    g = torch.Generator().manual_seed(_seed("maxfilter", shape, k))
    x = torch.randn(shape, generator=g)
    r = torch.rand(shape, generator=g)
    x[r < 0.05] = float("inf")
    x[r > 0.85] = float("-inf")
    want = F.max_pool2d(x[:, None], k, 1, k // 2)[:, 0]
    got = ops.maxfilter2d(x.to(cuda), k).cpu()
    assert got.shape == want.shape and torch.equal(got, want), (shape, k, int((got != want).sum()))


def test_maxfilter_grid_stride_and_even_k(cuda):
    from dcfp_amd import ops
    g = torch.Generator().manual_seed(_seed("maxfilter-large"))
    x = torch.randn(2, 700, 800, generator=g)                       # 1 120 000 > 4096 x 256
    assert torch.equal(ops.maxfilter2d(x.to(cuda), 3).cpu(), F.max_pool2d(x[:, None], 3, 1, 1)[:, 0])
    for k in (0, 2, 4, 8):
        with pytest.raises(RuntimeError):
            ops.maxfilter2d(x[:, :9, :9].to(cuda), k)


# ------------------------------------------------------------------------------------------------ 3. weighted CE
# Routing, by function name in upsample_ce.hip (ops.ce_backward_plan reports it).  dcfp_upsample_wce_bwd_f32 and
# dcfp_upsample_ce_bwd_f32 both go through launch_ce_bwd, the first with pix_weight and scale_per_image = 1, the second
# with pixel_keep and scale_per_image = 0: C == 19 -> ce_bwd_cells_kernel<*,19>, or upsample_ce_bwd_classes_kernel<*,19>
# when the process started with DCFP_CE_BWD_CELLS=0; any other C > 1 -> ce_bwd_cells_kernel<*,kCeChunk>, or
# upsample_ce_bwd_kernel under DCFP_CE_BWD_CELLS=0; C == 1 -> upsample_ce_bwd_kernel.
def _wce_weights(g, lab):
    """non-negative weights, zero on a random 30 % of the pixels, independent of the labels: non-zero on ignored ones"""
    wgt = torch.rand(lab.shape, generator=g) * 2.0 + 0.05
    wgt[torch.rand(lab.shape, generator=g) < 0.3] = 0.0
    return wgt


def _wce_ref(z, lab, wgt, coef, size, align, dt):
    zr = z.detach().clone().to(dt).requires_grad_(True)
    l = F.cross_entropy(_up(zr, size, align), lab, ignore_index=IGN, reduction="none")
    w = wgt.to(dt)
    num, den = (l * w).sum(dim=(1, 2)), w.sum(dim=(1, 2))
    (num * coef.to(dt)).sum().backward()
    return num.detach(), den, zr.grad


def _wce_measure(dev, geom, Cc, seed):
    """-> {what: (kernel error, fp32 yardstick)} and whether an ignored image got an exactly zero gradient"""
    from dcfp_amd import ops
    N, h, w, H, W, align, dead = geom
    g, z, lab = _inputs(geom, Cc, seed)
    wgt = _wce_weights(g, lab)
    ign = (lab.view(-1) == IGN).nonzero()
    if ign.numel():
        wgt.view(-1)[int(ign[0])] = 1.5                                    # (tiny maps) at least one such pixel
    coef = torch.rand(N, generator=g) + 0.5                              # a different upstream gradient per image
    num64, den64, g64 = _wce_ref(z, lab, wgt, coef, (H, W), align, torch.float64)
    num32, den32, g32 = _wce_ref(z, lab, wgt, coef, (H, W), align, torch.float32)
    zg = z.to(dev).requires_grad_(True)
    out = ops.upsample_weighted_ce(zg, lab.to(dev), wgt.to(dev), (H, W), align, IGN)
    assert tuple(out.shape) == (N, 2)
    (out[:, 0] * coef.to(dev)).sum().backward()
    res = {"sum w*ce": (_rel1(out[:, 0].detach(), num64), _rel1(num32, num64)),
           "sum w": (_rel1(out[:, 1].detach(), den64), _rel1(den32, den64)),
           "dlogits": (_nrel(zg.grad, g64), _nrel(g32, g64))}
    dead_ok = True
    if dead >= 0:
        dead_ok = float(out[dead, 0]) == 0.0 and bool((zg.grad[dead] == 0).all())
    return res, dead_ok and bool(torch.isfinite(zg.grad).all())


def _wce_assert(res, ok, case, group="wce"):
    for what, (err, yard) in res.items():
        _held(group, case, what, err, yard, CE_GFLOOR if what == "dlogits" else CE_FLOOR)
    assert ok, f"{case}: gradient not finite, or a fully ignored image with a non-zero loss / gradient"


WCE_CASES = _with_19(0)
WCE_LARGE = ((2, 46, 50, 368, 400, False, -1), 19)       # H*W = 147 200 > 512 x 256 per image: the forward strides


@pytest.mark.parametrize("geom,Cc", WCE_CASES + [WCE_LARGE], ids=_ids(WCE_CASES + [WCE_LARGE]))
def test_weighted_ce(cuda, geom, Cc):
    res, ok = _wce_measure(cuda, geom, Cc, _seed("wce", geom, Cc))
    _wce_assert(res, ok, _cid(geom, Cc))


# -------------------------------------------------------------------------------------- 4. the whole GSRL criterion
class _DS:
    ignore_label = IGN; num_classes = 19; class_weights = None


def _gsrl_cases():
    # C == 1 is left to groups 1 and 3: the criterion's formula needs a second-largest probability (`top[:, 1]`).
    out = []
    for i, (geom, Cc) in enumerate(_cycled(6, skip=(1,))):
        out.append((geom, Cc, [1, 3, 9][i % 3], [9, 0.5][(i // 3) % 2], i % 2 == 0))
    return out


GSRL_CASES = _gsrl_cases()


@pytest.mark.parametrize("geom,Cc,k,gamma,two_heads", GSRL_CASES,
                         ids=[f"{_cid(g, c)}-k{k}-g{gm}-h{1 + int(t)}" for g, c, k, gm, t in GSRL_CASES])
def test_gsrl_criterion(cuda, geom, Cc, k, gamma, two_heads):
    from dcfp_amd import ops
    from dcfp_amd.loss.criterion import build_criterions
    from oracle.gsrl import gsrl_loss
    N, h, w, H, W, align, dead = geom
    case = f"{_cid(geom, Cc)}-k{k}-g{gamma}-h{1 + int(two_heads)}"
    g, z0, lab = _inputs(geom, Cc, _seed("gsrl", geom, Cc, k))
    zs = [z0] + ([torch.randn(z0.shape, generator=g) * 1.5] if two_heads else [])
    bal = torch.rand(N, H, W, generator=g) * 2.0 + 0.1                   # sparse balance weights: the dilation matters
    bal[torch.rand(N, H, W, generator=g) < 0.6] = 0.0

    def ref(dt):
        zr = [t.detach().clone().to(dt).requires_grad_(True) for t in zs]
        loss = gsrl_loss([_up(t, (H, W), align) for t in zr], lab, bal.to(dt), IGN, 0.4, k, gamma)
        loss.backward()
        return loss.detach(), [t.grad for t in zr]
    l64, g64 = ref(torch.float64)
    l32, g32 = ref(torch.float32)
    crit = build_criterions("gsrl", _DS(), {"ds_weight": 0.4, "k": k, "gamma": gamma})
    zg = [t.to(cuda).requires_grad_(True) for t in zs]
    labels = {"ori": lab.to(cuda), "weight": bal.to(cuda)}
    loss = crit.forward_lowres(zg, labels, (H, W), align)["loss"]
    loss.backward()
    _held("gsrl", case, "loss", _rel1(loss.detach(), l64), _rel1(l32, l64), GSRL_FLOOR)
    for i in range(len(zs)):
        _held("gsrl", case, f"dlogits{i}", _nrel(zg[i].grad, g64[i]), _nrel(g32[i], g64[i]), GSRL_GFLOOR)
        assert torch.isfinite(zg[i].grad).all()
    if dead >= 0:
        # a restatement of forward_lowres' weight map (the criterion returns only the batch mean): it is zero on every
        # ignored pixel, so the image's term is exactly 0 / (0 + 1e-8); the criterion itself is held by the fp64 loss
        # parity above and by the exactly zero gradient below
        with torch.no_grad():
            wmap = ops.maxfilter2d(labels["weight"], k)
            wmap = (1 + gamma * (1 - ops.upsample_margin(zg[0].detach(), (H, W), align))) * wmap
            wmap[labels["ori"] == IGN] = 0.0
            out = ops.upsample_weighted_ce(zg[0].detach(), labels["ori"], wmap, (H, W), align, IGN)
        assert float(out[dead, 0]) == 0.0 and float(out[dead, 1]) == 0.0, out
        for t in zg:
            assert bool((t.grad[dead] == 0).all())


# ------------------------------------------------------------------------------------------- 5. CE with pixel_keep
def _keep_ref(z, lab, keep, size, align, dt):
    zr = z.detach().clone().to(dt).requires_grad_(True)
    relabelled = lab.clone()
    relabelled[keep == 0] = IGN
    loss = F.cross_entropy(_up(zr, size, align), relabelled, ignore_index=IGN)
    loss.backward()
    return loss.detach(), zr.grad


def _keep_measure(dev, geom, Cc, seed):
    from dcfp_amd import ops
    N, h, w, H, W, align, dead = geom
    g, z, lab = _inputs(geom, Cc, seed)
    keep = (torch.rand(N, H, W, generator=g) < 0.6).to(torch.uint8)
    if not bool(((keep != 0) & (lab != IGN)).any()):
        keep.view(-1)[int((lab.view(-1) != IGN).nonzero()[0])] = 1       # (tiny maps) keep at least one labelled pixel
    l64, g64 = _keep_ref(z, lab, keep, (H, W), align, torch.float64)
    l32, g32 = _keep_ref(z, lab, keep, (H, W), align, torch.float32)
    zg = z.to(dev).requires_grad_(True)
    loss = ops.upsample_cross_entropy(zg, lab.to(dev), (H, W), align, IGN, pixel_keep=keep.to(dev))
    loss.backward()
    res = {"loss": (_rel1(loss.detach(), l64), _rel1(l32, l64)), "dlogits": (_nrel(zg.grad, g64), _nrel(g32, g64))}
    ok = bool(torch.isfinite(zg.grad).all()) and (dead < 0 or bool((zg.grad[dead] == 0).all()))
    return res, ok


KEEP_CASES = _with_19(3)


@pytest.mark.parametrize("geom,Cc", KEEP_CASES, ids=_ids(KEEP_CASES))
def test_ce_pixel_keep(cuda, geom, Cc):
    res, ok = _keep_measure(cuda, geom, Cc, _seed("keep", geom, Cc))
    _wce_assert(res, ok, _cid(geom, Cc), "ce-keep")


@pytest.mark.parametrize("Cc", [19, 7])
def test_ce_pixel_keep_nothing_kept(cuda, Cc):
    from dcfp_amd import ops
    _, z, lab = _inputs(GEOMS[7], Cc, _seed("keep-none", Cc))
    out = ops.upsample_cross_entropy(z.to(cuda), lab.to(cuda), (64, 128), False, IGN,
                                     pixel_keep=torch.zeros(lab.shape, dtype=torch.uint8, device=cuda))
    assert math.isnan(out.item())          # mean over zero kept pixels, like test_upsample_ce_all_ignored


def _c19(cases):
    return [(g, c) for g, c in cases if c == 19]


def _child(which):
    """The C == 19 cases once more in a process that starts with DCFP_CE_BWD_CELLS=0 (the library reads it once)."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert os.environ.get("DCFP_CE_BWD_CELLS") == "0"
    dev = torch.device("cuda:0")
    out = {}
    if which == "wce":
        for geom, Cc in _c19(WCE_CASES + [WCE_LARGE]):
            out[_cid(geom, Cc)] = _wce_measure(dev, geom, Cc, _seed("wce", geom, Cc))
    else:
        for geom, Cc in _c19(KEEP_CASES):
            out[_cid(geom, Cc)] = _keep_measure(dev, geom, Cc, _seed("keep", geom, Cc))
    torch.cuda.synchronize()
    print("LOSS_EVAL_RESULT " + json.dumps(out))


@pytest.mark.parametrize("which", ["wce", "keep"])
def test_c19_per_output_kernel(cuda, which):
    """DCFP_CE_BWD_CELLS=0: upsample_ce_bwd_classes_kernel<*,19>, weighted / per-image and with pixel_keep, held to
    fp64 at the tolerance of the cell kernel (two summation orders: not compared with each other bit for bit)."""
    env = dict(os.environ, DCFP_CE_BWD_CELLS="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("LOSS_EVAL_RESULT ")][-1]
    res = json.loads(line[len("LOSS_EVAL_RESULT "):])
    cases = _c19(WCE_CASES + [WCE_LARGE]) if which == "wce" else _c19(KEEP_CASES)
    assert sorted(res) == sorted(_cid(g, c) for g, c in cases)
    for case, (errs, ok) in res.items():
        _wce_assert({k: tuple(v) for k, v in errs.items()}, ok, case, f"{'wce' if which == 'wce' else 'ce-keep'}-cells0")


# ---------------------------------------------------------------------------------------------------- 6. OHEM zoom
def _zoom(dev, z, lab, size, align, f):
    """dcfp_ohem_zoom_gt_prob_f32 with the arguments OhemCrossEntropy2d.threshold_device builds"""
    from dcfp_amd import _lib, ops
    zg, lg = z.to(dev).contiguous(), lab.to(dev).contiguous()
    _, lse, gtp = ops.upsample_ce_forward(zg, lg, size, align, IGN, want_gt_prob=True)
    N, Cc, h, w = z.shape
    H, W = size
    H8, W8 = int(round(H * (1.0 / f))), int(round(W * (1.0 / f)))
    pred8 = torch.full((N, H8, W8), -7.0, dtype=torch.float32, device=dev)
    lab8 = torch.full((N, H8, W8), -7, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().dcfp_ohem_zoom_gt_prob_f32(
        C.c_void_p(zg.data_ptr()), C.c_void_p(lg.data_ptr()), C.c_void_p(lse.data_ptr()), N, Cc, h, w, H, W,
        int(bool(align)), H8, W8, C.c_void_p(pred8.data_ptr()), C.c_void_p(lab8.data_ptr()),
        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ohem_zoom")
    return pred8.cpu(), lab8.cpu(), gtp.cpu(), lse


# (N, C, h, w, H, W, align, factor): 20 / 28 / 36 and 12 / 52 land on x.5 (Python rounds half to even: 2, 4, 4, 2, 6);
# factor 2 with 6 and 10 puts scipy's source coordinate on an exact half (2.5, 4.5)
ZOOM_CASES = [
    (2, 19, 3, 4, 20, 28, True, 8),
    (2, 7, 5, 5, 36, 20, False, 8),
    (1, 19, 2, 3, 12, 52, True, 8),
    (2, 20, 2, 9, 9, 75, False, 8),        # H8 == 1
    (2, 2, 1, 3, 11, 8, True, 8),          # H8 == 1 and W8 == 1
    (2, 19, 3, 5, 6, 10, True, 2),
    (1, 2, 6, 10, 6, 10, False, 2),        # identity, factor 2
    (2, 7, 5, 3, 10, 6, False, 2),
    (2, 60, 9, 13, 65, 97, True, 8),
    (1, 150, 8, 8, 61, 43, False, 8),
    (3, 1, 4, 4, 30, 30, True, 8),
]


@pytest.mark.parametrize("case", ZOOM_CASES, ids=lambda c: "x".join(map(str, c[:4])) + f"-{c[4]}x{c[5]}-a{int(c[6])}-f{c[7]}")
def test_ohem_zoom(cuda, case):
    import scipy.ndimage as nd
    from oracle import ohem as oohem
    from dcfp_amd.loss.ohem import OhemCrossEntropy2d
    N, Cc, h, w, H, W, align, f = case
    tag = "x".join(map(str, case[:4])) + f"-{H}x{W}-a{int(align)}-f{f}"
    g = torch.Generator().manual_seed(_seed("zoom", case))
    z = torch.randn(N, Cc, h, w, generator=g) * 2.5
    lab = torch.randint(0, Cc, (N, H, W), generator=g)
    lab[torch.rand(N, H, W, generator=g) < 0.15] = IGN
    pred8, lab8, _, lse = _zoom(cuda, z, lab, (H, W), align, f)
    lz = nd.zoom(lab.numpy(), (1.0, 1.0 / f, 1.0 / f), order=0)
    assert tuple(lab8.shape) == lz.shape                                  # H8 = round(H / f), as scipy sizes it
    assert np.array_equal(lab8.numpy(), lz.astype(np.int32)), int((lab8.numpy() != lz).sum())
    valid = lz != IGN

    def ref(dt):
        prob = torch.softmax(_up(z.to(dt), (H, W), align), 1).numpy()
        pz = nd.zoom(prob, (1.0, 1.0, 1.0 / f, 1.0 / f), order=1)
        return prob, np.take_along_axis(pz, np.minimum(lz, Cc - 1)[:, None], 1)[:, 0].astype(np.float64)
    prob64, p64 = ref(torch.float64)
    prob32, p32 = ref(torch.float32)
    err = float(np.abs(pred8.numpy().astype(np.float64) - p64)[valid].max()) if valid.any() else 0.0
    yard = float(np.abs(p32 - p64)[valid].max()) if valid.any() else 0.0
    _held("ohem-zoom", tag, "pred8", err, yard, PROB_FLOOR)
    # the production sizing and the select on top of it: threshold_device against the scipy restatement
    mk = f * f * (int(valid.sum()) // 2)
    th64 = oohem.find_threshold(prob64, lab.numpy(), IGN, 0.05, mk, f)
    th32 = oohem.find_threshold(prob32, lab.numpy(), IGN, 0.05, mk, f)
    crit = OhemCrossEntropy2d(ignore_label=IGN, thresh=0.05, min_kept=mk, factor=f)
    th = crit.find_threshold(z.to(cuda), lab.to(cuda), lse, (H, W), align)
    _held("ohem-zoom", tag, "threshold", abs(th - float(th64)), abs(float(th32) - float(th64)), PROB_FLOOR)


def test_ohem_zoom_factor1_grid_stride(cuda):
    """factor 1: the zoom is the identity, so pred8 is the CE forward's gt_prob and lab8 the labels - at
    N*H*W = 1 064 960 > 4096 x 256 the kernel goes round its grid-stride loop twice."""
    N, Cc, h, w, H, W = 2, 7, 80, 104, 640, 832
    g = torch.Generator().manual_seed(_seed("zoom-f1"))
    z = torch.randn(N, Cc, h, w, generator=g) * 2.5
    lab = torch.randint(0, Cc, (N, H, W), generator=g)
    lab[torch.rand(N, H, W, generator=g) < 0.15] = IGN
    pred8, lab8, gtp, _ = _zoom(cuda, z, lab, (H, W), True, 1)
    assert torch.equal(lab8.long(), lab)
    valid = lab != IGN

    def ref(dt):
        p = torch.softmax(_up(z.to(dt), (H, W), True), 1)
        return p.gather(1, lab.clamp(max=Cc - 1)[:, None])[:, 0].double()
    p64, p32 = ref(torch.float64), ref(torch.float32)
    yard = _abs(p32[valid], p64[valid])
    _held("ohem-zoom", "f1-2x7x80x104-640x832", "pred8 vs fp64", _abs(pred8[valid], p64[valid]), yard, PROB_FLOOR)
    _held("ohem-zoom", "f1-2x7x80x104-640x832", "gt_prob vs fp64", _abs(gtp[valid], p64[valid]), yard, PROB_FLOOR)
    _held("ohem-zoom", "f1-2x7x80x104-640x832", "pred8 vs gt_prob", _abs(pred8[valid], gtp[valid]), yard, PROB_FLOOR)


# ---------------------------------------------------------------------------------------------------- 7. keep mask
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1023, 1000003, 4200003])
def test_ohem_keep_mask(cuda, n):
    """float4 / uchar4 body and the n % 4 tail, values equal to the threshold, thresholds 0 and 1; 4 200 003 goes
    round the 4096 x 256 x 4 grid-stride loop.  The eight bytes behind the mask must stay untouched."""
    from dcfp_amd import _lib
    g = torch.Generator().manual_seed(_seed("keepmask", n))
    for thr in (0.0, 1.0, 0.7, float(torch.rand(1, generator=g))):
        t32 = torch.tensor([thr], dtype=torch.float32)
        v = torch.rand(n + 8, generator=g)
        r = torch.rand(n + 8, generator=g)
        v[r < 0.25] = t32[0]                                               # exactly the threshold
        v[(r >= 0.25) & (r < 0.30)] = 0.0
        v[(r >= 0.30) & (r < 0.35)] = 1.0
        buf, tdev = v.to(cuda), t32.to(cuda)                               # allocations are 16-byte aligned
        assert buf.data_ptr() % 16 == 0
        gtp = buf[:n]
        keep = torch.full((n + 8,), 0xAB, dtype=torch.uint8, device=cuda)
        _lib.check(_lib.lib().dcfp_ohem_keep_mask_u8(
            C.c_void_p(gtp.data_ptr()), C.c_void_p(tdev.data_ptr()), n, C.c_void_p(keep.data_ptr()),
            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ohem_keep_mask")
        keep = keep.cpu()
        assert torch.equal(keep[:n], (v[:n] <= t32[0]).to(torch.uint8)), (n, thr)
        assert bool((keep[n:] == 0xAB).all()), (n, thr)


# ------------------------------------------------------------------------------------------------------- 8. argmax
def _argmax_check(cuda, z, size, align, case):
    """the rule of test_inference_path_vs_oracle: equal wherever the fp64 top-2 gap exceeds 1e-4 of the logits' scale,
    and that must be more than 0.99 of the pixels (a condition on the case, not a tolerance)"""
    from dcfp_amd import ops
    got = ops.upsample_argmax(z.to(cuda), size, align)
    assert got.dtype == torch.int32
    got = got.cpu().long()
    up = _up(z.double(), size, align)
    want = up.argmax(1)
    if z.shape[1] == 1:
        decisive = torch.ones_like(want, dtype=torch.bool)
    else:
        top2 = up.topk(2, dim=1).values
        decisive = (top2[:, 0] - top2[:, 1]) > 1e-4 * up.abs().max()
    share = float(decisive.double().mean())
    print(f"PARITY argmax {case} decisive share {share:.5f}, mismatches {int((got != want)[decisive].sum())}")
    assert share > 0.99, (case, share)
    assert bool((got[decisive] == want[decisive]).all()), (case, int((got != want)[decisive].sum()))


ARGMAX_CASES = _cycled(3)


@pytest.mark.parametrize("geom,Cc", ARGMAX_CASES, ids=_ids(ARGMAX_CASES))
def test_argmax(cuda, geom, Cc):
    N, h, w, H, W, align, _ = geom
    _, z, _ = _inputs(geom, Cc, _seed("argmax", geom, Cc))
    _argmax_check(cuda, z, (H, W), align, _cid(geom, Cc))


def test_argmax_grid_stride(cuda):
    g = torch.Generator().manual_seed(_seed("argmax-large"))
    z = torch.randn(2, 7, 80, 104, generator=g) * 2.5                       # N*H*W = 1 064 960 > 4096 x 256
    _argmax_check(cuda, z, (640, 832), False, "2x7x80x104-640x832")


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("Cc", [2, 19, 150])
def test_argmax_first_maximum_wins(cuda, Cc, align):
    """integer logits with duplicated maxima at h == H, w == W (the interpolation is exact): np.argmax on every pixel"""
    from dcfp_amd import ops
    g = torch.Generator().manual_seed(_seed("argmax-ties", Cc, align))
    z = torch.randint(-2, 3, (2, Cc, 15, 31), generator=g).float()
    want = np.argmax(z.numpy(), axis=1)
    assert (np.sort(z.numpy(), axis=1)[:, -1] == np.sort(z.numpy(), axis=1)[:, -2]).mean() > 0.15
    got = ops.upsample_argmax(z.to(cuda), (15, 31), align).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())


# --------------------------------------------------------------------------------------------- 9. confusion matrix
def _conf_data(n, Cc, seed, dirty=True):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, Cc, n).astype(np.int64)
    pred = rng.integers(0, Cc, n).astype(np.int32)
    r = rng.random(n)
    gt[r < 0.10] = IGN
    if dirty:                       # what both kernels document they drop
        gt[(r >= 0.10) & (r < 0.13)] = Cc + 3 if Cc + 3 != IGN else Cc + 4        # >= C, not the ignore value
        gt[(r >= 0.13) & (r < 0.16)] = -1
        pred[(r >= 0.16) & (r < 0.19)] = Cc
        pred[(r >= 0.19) & (r < 0.22)] = -2
        pred[(r >= 0.22) & (r < 0.25)] = Cc + 7
    return gt, pred


def _conf_ref(gt, pred, Cc):
    keep = (gt != IGN) & (gt >= 0) & (gt < Cc) & (pred >= 0) & (pred < Cc)
    return np.bincount(gt[keep] * Cc + pred[keep].astype(np.int64), minlength=Cc * Cc).reshape(Cc, Cc)


@pytest.mark.parametrize("Cc", [1, 2, 19, 64, 65, 150, 1024])
def test_confusion_matrix(cuda, Cc):
    """C <= 64: the LDS histogram kernel; above: confusion_global_kernel.  n = 300 001 > 1024 x 256: the grid strides.
    A second call with out= adds to the first."""
    from dcfp_amd import ops
    total = np.zeros((Cc, Cc), dtype=np.int64)
    out = None
    for n in (300001, 1000, 1):
        gt, pred = _conf_data(n, Cc, _seed("conf", Cc, n))
        want = _conf_ref(gt, pred, Cc)
        got = ops.confusion_matrix(torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda), Cc, IGN)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (Cc, n)
        total += want
        out = ops.confusion_matrix(torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda), Cc, IGN, out=out)
        assert np.array_equal(out.cpu().numpy(), total), (Cc, n)
    assert total.sum() > 0


def test_confusion_matrix_limits(cuda):
    from dcfp_amd import ops
    gt, pred = _conf_data(100, 19, 1)
    p, g = torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda)
    with pytest.raises(RuntimeError):
        ops.confusion_matrix(p, g, 1025, IGN)
    # n = 0 leaves the matrix as it is
    seed = ops.confusion_matrix(p, g, 19, IGN)
    before = seed.clone()
    out = ops.confusion_matrix(p[:0], g[:0], 19, IGN, out=seed)
    assert torch.equal(out, before)
    assert int(ops.confusion_matrix(p[:0], g[:0], 19, IGN).sum()) == 0
    empty = ops.confusion_matrix(torch.empty(0, dtype=torch.int32, device=cuda),
                                 torch.empty(0, dtype=torch.int64, device=cuda), 19, IGN)
    assert tuple(empty.shape) == (19, 19) and int(empty.sum()) == 0


def test_confusion_matrix_both_kernels_agree(cuda):
    """the same 64-class data through the LDS kernel (C = 64) and the global one (C = 65)"""
    from dcfp_amd import ops
    gt, pred = _conf_data(300001, 64, _seed("conf-agree"), dirty=False)
    p, g = torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda)
    c64 = ops.confusion_matrix(p, g, 64, IGN).cpu().numpy()
    c65 = ops.confusion_matrix(p, g, 65, IGN).cpu().numpy()
    assert np.array_equal(c64, _conf_ref(gt, pred, 64))
    assert np.array_equal(c65[:64, :64], c64) and c65[64].sum() == 0 and c65[:, 64].sum() == 0


if __name__ == "__main__" and "--child" in sys.argv:
    _child(sys.argv[sys.argv.index("--child") + 1])
