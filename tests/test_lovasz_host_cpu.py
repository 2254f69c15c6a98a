"""Host side of the Lovasz-Softmax fine-tune loss, no GPU: the torch restatement of the binned definition
(tests/_lovasz_ref.py) against the exact sort-based loss - the two-sided bound, equality at ties, the telescoping of
the bin weights - the all-ignored batch, the `lovasz` criterion's construction and errors, and every error code of the
C entries."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lovasz_ref as lr  # noqa: E402

BINS = [64, 1024, 4096]
# (probability shape, logit scale): the fixtures of the definition's CPU check
FIXTURES = [((2, 19, 33, 65), 3.0), ((1, 2, 17, 17), 1.0), ((2, 59, 20, 30), 5.0), ((1, 19, 64, 64), 0.1)]
_CASES = {}


class _DS:
    ignore_label = 255
    num_classes = 19
    class_weights = None


def _case(k):
    if k not in _CASES:
        shape, scale = FIXTURES[k]
        logits = lr.make_logits(shape, scale, 100 + k)
        size = shape[2:]
        labels = lr.make_labels(logits, size, True, 200 + k)
        _CASES[k] = (logits, labels, size, lr.exact(logits, labels, size, True, 255, torch.float64))
    return _CASES[k]


# ------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize("B", BINS)
@pytest.mark.parametrize("k", range(len(FIXTURES)))
def test_binned_loss_within_the_bound_of_the_exact_loss(k, B):
    logits, labels, size, (L, gL) = _case(k)
    loss, grad = lr.binned(logits, labels, size, True, 255, B, torch.float64)
    L, loss = float(L), float(loss)
    print(f"LOVASZ fixture {k} B={B}: exact {L:.9f} exact-binned {L - loss:.3e} grad nrel {lr.nrel(grad, gL):.3e}")
    assert L - 1.0 / B - 2.0 ** -21 <= loss <= L + 2.0 ** -21
    assert 0.0 < loss < 1.0
    # the gradient is a subgradient choice at ties, not the sort's: close at 64 bins, closer at 4096
    assert lr.nrel(grad, gL) <= (0.05 if B == 64 else 0.02)


def test_fp32_restatement_agrees_with_fp64():
    logits, labels, size, _ = _case(1)
    l64, g64 = lr.binned(logits, labels, size, True, 255, 1024, torch.float64)
    l32, g32 = lr.binned(logits, labels, size, True, 255, 1024, torch.float32)
    assert abs(float(l32) - float(l64)) <= 1e-5 and lr.nrel(g32, g64) <= 1e-3


@pytest.mark.parametrize("B", BINS)
def test_equal_to_the_exact_loss_when_errors_are_tied(B):
    """errors k / 64, k < 64: on the 2^-20 grid, one value per bin at every B >= 64 - the sort's ties are the bins"""
    g = torch.Generator().manual_seed(7)
    N, Cc, H, W = 2, 5, 12, 20
    e = torch.randint(0, 64, (N, Cc, H, W), generator=g).double() / 64
    labels = torch.randint(0, Cc, (N, H, W), generator=g)
    labels[torch.rand(N, H, W, generator=g) < 0.2] = 255
    valid, fg = lr.masks(labels, Cc, 255)
    q = lr.quantise(e)
    assert torch.equal(q.double(), e * 2 ** 20)
    loss = lr.loss_of_histogram(lr.histogram(q, lr.bins_of(q, B), fg, valid, B), torch.float64)
    want = lr.exact_from_errors(e, fg, valid)
    assert abs(float(loss) - float(want)) <= 1e-13 and float(want) > 0.1


@pytest.mark.parametrize("B", BINS)
def test_bin_weights_telescope_to_the_jaccard_index(B):
    logits, labels, size, _ = _case(0)
    valid, fg = lr.masks(labels, logits.shape[1], 255)
    q = lr.quantise(lr.errors(lr.probs(logits, size, True, torch.float64), fg))
    nF, nB, SF, SB = lr.histogram(q, lr.bins_of(q, B), fg, valid, B)
    wF, wB, present = lr.weights(nF, nB, torch.float64)
    assert bool(present.any()) and bool((wF >= 0).all()) and bool((wB >= 0).all())
    inc = nF * wF + nB * wB                                            # Jaccard increment per bin
    run = torch.flip(torch.cumsum(torch.flip(inc, [1]), 1), [1])       # summed from bin B - 1 down to b
    G = nF.sum(1, keepdim=True)
    F_to = torch.flip(torch.cumsum(torch.flip(nF, [1]), 1), [1])
    B_to = torch.flip(torch.cumsum(torch.flip(nB, [1]), 1), [1])
    jac = 1 - (G - F_to).double() / (G + B_to).double().clamp(min=1)
    rows = present.nonzero().flatten()
    assert float((run[rows] - jac[rows]).abs().max()) <= 1e-12
    assert float((run[rows, 0] - 1).abs().max()) <= 1e-12              # every pixel passed: I = 0, J = 1
    assert float(inc[~present].abs().sum()) == 0.0


def test_all_ignored_gives_zero_without_nan():
    logits = lr.make_logits((2, 5, 4, 6), 2.0, 1)
    labels = torch.full((2, 9, 13), 255)
    labels[0, 0, 0] = 7                                                 # no class either
    for dtype in (torch.float64, torch.float32):
        loss, grad = lr.binned(logits, labels, (9, 13), True, 255, 64, dtype)
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    loss, grad = lr.exact(logits, labels, (9, 13), True, 255, torch.float64)
    assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the criterion
def test_criterion_builds_and_refuses_bad_parameters():
    from dcfp_amd.loss.criterion import (CombinedCriterion, CriterionDSN, CriterionGsrlDSN, CriterionLovasz,
                                         build_criterions)
    crit = build_criterions("gsrl,lovasz", _DS(), {"ds_weight": 0.4, "lovasz_weight": 0.5, "lovasz_bins": 256})
    assert isinstance(crit, CombinedCriterion)
    assert [type(c) for c in crit.criterions] == [CriterionGsrlDSN, CriterionLovasz]
    lv = crit.criterions[1]
    assert (lv.lovasz_weight, lv.lovasz_bins, lv.ignore_index) == (0.5, 256, 255)
    assert [type(c) for c in build_criterions("ce,lovasz", _DS(), {}).criterions] == [CriterionDSN, CriterionLovasz]
    alone = build_criterions("lovasz", _DS(), {})
    assert isinstance(alone, CriterionLovasz) and (alone.lovasz_weight, alone.lovasz_bins) == (1.0, 1024)
    assert build_criterions("lovasz", _DS(), {"lovasz_weight": 0.0}).lovasz_weight == 0.0
    for bins in (0, 32, 100, 1000, 8192, -64, 1024.5, "1024", True):
        with pytest.raises(ValueError, match="lovasz_bins"):
            build_criterions("lovasz", _DS(), {"lovasz_bins": bins})
    for weight in (-1.0, -1e-9, float("nan")):
        with pytest.raises(ValueError, match="lovasz_weight"):
            build_criterions("lovasz", _DS(), {"lovasz_weight": weight})


def test_lovasz_ops_have_no_cpu_path():
    from dcfp_amd import ops
    z = torch.zeros(1, 3, 2, 2)
    lab = torch.zeros(1, 5, 5, dtype=torch.int64)
    for fn in (ops.lovasz_softmax, ops.lovasz_histogram, ops.lovasz_errors):
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(z, lab, (5, 5), True)
    from dcfp_amd.loss.criterion import build_criterions
    crit = build_criterions("lovasz", _DS(), {})
    for labels in (lab, {"ori": lab}):
        with pytest.raises(RuntimeError, match="CUDA"):
            crit.forward_lowres([z], labels, (5, 5), True)
        with pytest.raises(RuntimeError, match="CUDA"):
            crit([z], labels)


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_abi_argument_errors_need_no_gpu():
    from dcfp_amd import _lib
    L = _lib.lib()
    BAD, UNS, WS = _lib.E_BADDESC, _lib.E_UNSUPPORTED, _lib.E_WORKSPACE
    p = C.c_void_p(4096)                     # never dereferenced: every call below returns before any HIP call
    shape = dict(N=2, Cc=19, h=9, w=9, H=65, W=65)
    BIG = 1 << 30

    def hist(logits=p, labels=p, bins=1024, lse=p, ws=p, nbytes=BIG, **kw):
        s = dict(shape, **kw)
        return L.dcfp_lovasz_hist_f32(logits, labels, 255, s["N"], s["Cc"], s["h"], s["w"], s["H"], s["W"], 1, bins, lse,
                                      ws, nbytes, None)

    def scan(Cc=19, bins=1024, ws=p, nbytes=BIG, out=p, table=p):
        return L.dcfp_lovasz_scan_f32(Cc, bins, ws, nbytes, out, table, None)

    def bwd(bins=1024, **kw):
        ptr = {k: kw.pop(k, p) for k in ("logits", "labels", "lse", "table", "scale", "asum", "dl")}
        s = dict(shape, **kw)
        return L.dcfp_lovasz_bwd_f32(ptr["logits"], ptr["labels"], 255, s["N"], s["Cc"], s["h"], s["w"], s["H"], s["W"],
                                     1, bins, ptr["lse"], ptr["table"], ptr["scale"], ptr["asum"], ptr["dl"], None)

    def errs(logits=p, labels=p, out=p, **kw):
        s = dict(shape, **kw)
        return L.dcfp_lovasz_errors_u32(logits, labels, 255, s["N"], s["Cc"], s["h"], s["w"], s["H"], s["W"], 1, out, None)

    # null pointers
    assert hist(logits=None) == BAD and hist(labels=None) == BAD and hist(lse=None) == BAD
    assert scan(out=None) == BAD and scan(table=None) == BAD
    for k in ("logits", "labels", "lse", "table", "scale", "asum", "dl"):
        assert bwd(**{k: None}) == BAD, k
    assert errs(logits=None) == BAD and errs(labels=None) == BAD and errs(out=None) == BAD
    # sizes
    for key in shape:
        for v in (0, -3):
            assert hist(**{key: v}) == BAD and bwd(**{key: v}) == BAD and errs(**{key: v}) == BAD, key
    assert scan(Cc=0) == BAD and scan(Cc=-1) == BAD
    # bins: a power of two in 64 .. 4096
    for bins in (0, -1024, 32, 63, 96, 1000, 4095, 8192):
        assert hist(bins=bins) == BAD and scan(bins=bins) == BAD and bwd(bins=bins) == BAD, bins
        assert L.dcfp_lovasz_workspace_bytes(19, bins) == 0
    for bins in (64, 128, 256, 512, 1024, 2048, 4096):
        need = 19 * bins * 40 + 19 * 16
        assert L.dcfp_lovasz_workspace_bytes(19, bins) == need
        # workspace: null or too small
        assert hist(bins=bins, nbytes=need - 1) == WS and hist(bins=bins, ws=None) == WS
        assert scan(bins=bins, nbytes=need - 1) == WS and scan(bins=bins, ws=None) == WS
    # more than 255 classes, 2^31 pixels or more
    assert hist(Cc=256) == UNS and bwd(Cc=256) == UNS and errs(Cc=256) == UNS and scan(Cc=256) == UNS
    assert L.dcfp_lovasz_workspace_bytes(256, 1024) == 0 and L.dcfp_lovasz_workspace_bytes(0, 1024) == 0
    assert L.dcfp_lovasz_workspace_bytes(255, 4096) == 255 * 4096 * 40 + 255 * 16
    for kw in (dict(N=2, H=32768, W=32768), dict(N=8, H=16384, W=16384), dict(N=1, H=46341, W=46341)):
        assert hist(**kw) == UNS and bwd(**kw) == UNS and errs(**kw) == UNS
