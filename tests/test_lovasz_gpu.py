"""ops.lovasz_softmax / lovasz_histogram / lovasz_errors (dcfp_amd/csrc/lovasz.hip) stage by stage, so that a
bin flipped by fp32 rounding can neither hide nor fake a failure:

  1 errors     |q_dev - e64 2^20| <= 0.5 + tau 2^20, tau = 4 x the largest |e_fp32 - e_fp64| of the torch restatement on
               that input; 0xFFFFFFFF exactly at the pixels that do not count
  2 histogram  bit-equal to the integer bincount of q_dev (all four tensors), the same bits on a second call
  3 loss       within 1e-6 relative of the fp64 formulas on the device's own histogram (only the last roundings differ),
               and L - 1/B - 2^-21 - tau - r <= loss <= L + 2^-21 + tau + r against the exact sort-based loss L on fp64
               probabilities: the per-class weights are non-negative and sum to at most 1, so errors that move by at most
               tau move the loss by at most tau; r = 2^-23 |loss| is the rounding of the result to fp32
  4 gradient   within max(3e-5 norm-relative, 3 x the fp32 restatement) of fp64 autograd that uses the device's bins and
               histogram; grad_output = 0.37; a non-contiguous logits tensor; the same bits on a second call

Shapes come from the kernels' geometry.  A histogram workgroup owns at least 2048 pixels (49 x 113 x 2 and 65 x 129 x 2
are 6 and 9 of them, the last partial, one straddling two images) and keeps 4096 / B classes in LDS at a time: 64 | 65
classes at B = 64, 4 | 5 at 1024 and 1 | 2 at 4096 are the two sides of that class-count threshold; the scan gives a
thread B / 256 bins at B > 256 and leaves threads idle at B = 64.  The backward's gather works on tiles of 7 x 15
low-resolution outputs (7 x 15 is one tile, 9 x 17 four, 1 x 130 nine in a row, 16 x 16 and 8 x 8 partial ones) and on
windows of 20 classes: 19 is a partial window, 20 a full one, 21 a full one and a window of one class, 59 / 64 / 150 /
171 several full ones and a tail."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lovasz_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu

IGNORE = 255
# name -> (logits shape, size, align_corners, logit scale, bins)
CASES = {
    "1x1x3x5": ((1, 1, 3, 5), (9, 17), True, 3.0, (64, 1024, 4096)),             # one class: the 4096-bin chunk is full
    "1x2x3x5": ((1, 2, 3, 5), (9, 17), True, 3.0, (64, 1024, 4096)),             # ... and one class more than fits
    "2x19x7x15": ((2, 19, 7, 15), (49, 113), True, 3.0, (64, 1024, 4096)),
    "2x19x9x17": ((2, 19, 9, 17), (65, 129), True, 3.0, (1024,)),
    "2x19x16x16-identity": ((2, 19, 16, 16), (16, 16), True, 3.0, (1024,)),
    "2x19x8x8-noalign": ((2, 19, 8, 8), (64, 64), False, 3.0, (64, 1024)),
    "1x59x5x9": ((1, 59, 5, 9), (33, 65), True, 5.0, (64, 1024, 4096)),
    "2x150x3x5": ((2, 150, 3, 5), (17, 33), True, 3.0, (1024,)),
    "2x171x3x5": ((2, 171, 3, 5), (17, 33), True, 3.0, (64, 4096)),
    "3x19x1x130": ((3, 19, 1, 130), (1, 1033), True, 3.0, (1024,)),
    "1x4x3x5": ((1, 4, 3, 5), (9, 17), True, 2.0, (1024,)),                       # the last class count of one chunk ...
    "1x5x3x5": ((1, 5, 3, 5), (9, 17), True, 2.0, (1024,)),                       # ... and the first of two
    "1x20x3x5": ((1, 20, 3, 5), (9, 17), True, 3.0, (1024,)),                     # one full window of the backward ...
    "1x21x3x5": ((1, 21, 3, 5), (9, 17), True, 3.0, (1024,)),                     # ... and a window of one class after it
    "1x64x3x5": ((1, 64, 3, 5), (9, 17), True, 3.0, (64,)),
    "1x65x3x5": ((1, 65, 3, 5), (9, 17), True, 3.0, (64,)),
    "near-uniform": ((1, 19, 8, 8), (29, 29), True, 0.1, (64, 1024)),
}
SPECIAL = ("ignored30", "foreign-labels", "one-pixel-class", "one-class", "all-ignored", "pm80", "perfect")
PARAMS = [(k, b) for k, v in CASES.items() for b in v[4]] + [(k, b) for k in SPECIAL for b in (64, 1024)]
_INPUTS, _REFS, _DEV = {}, {}, {}


def _inputs(name):
    """(logits, labels, size, align_corners) on the CPU, made once per case and left unchanged"""
    if name in _INPUTS:
        return _INPUTS[name]
    seed = sum(map(ord, name))
    if name in CASES:
        shape, size, ac, scale, _ = CASES[name]
        logits = lr.make_logits(shape, scale, seed)
        labels = lr.make_labels(logits, size, ac, seed + 1)
    else:
        shape, size, ac = (2, 19, 7, 15), (49, 113), True
        logits = lr.make_logits(shape, 3.0, seed)
        labels = lr.make_labels(logits, size, ac, seed + 1, ignored=0.3 if name == "ignored30" else 0.1)
        if name == "foreign-labels":                # values that are neither a class nor ignore_index
            g = torch.Generator().manual_seed(seed + 2)
            r = torch.rand(labels.shape, generator=g)
            labels[r < 0.05] = 19
            labels[(r >= 0.05) & (r < 0.1)] = -1
            labels[(r >= 0.1) & (r < 0.15)] = 300
            labels[(r >= 0.15) & (r < 0.17)] = -(1 << 40)
        elif name == "one-pixel-class":
            labels[labels == 7] = 3
            labels[1, 20, 50] = 7
        elif name == "one-class":
            labels[labels != IGNORE] = 11
        elif name == "all-ignored":
            labels[:] = IGNORE
        elif name == "pm80":                        # errors of exactly 0 and 1: q = 2^20 goes to bin B - 1
            logits = logits * (80.0 / logits.abs().max())
        elif name == "perfect":                     # identity upsample, the label's logit 40 above the others
            shape, size = (2, 19, 16, 16), (16, 16)
            labels = torch.randint(0, 19, (2, 16, 16), generator=torch.Generator().manual_seed(seed))
            labels[0, :2] = IGNORE
            logits = 40.0 * torch.nn.functional.one_hot(labels.clamp(max=18), 19).permute(0, 3, 1, 2).float()
    _INPUTS[name] = (logits, labels, size, ac)
    return _INPUTS[name]


def _ref(name):
    """CPU side that does not depend on B: masks, e in fp64, tau, the exact loss"""
    if name not in _REFS:
        logits, labels, size, ac = _inputs(name)
        valid, fg = lr.masks(labels, logits.shape[1], IGNORE)
        e64 = lr.errors(lr.probs(logits, size, ac, torch.float64), fg)
        e32 = lr.errors(lr.probs(logits, size, ac, torch.float32), fg)
        v = valid.unsqueeze(1).expand_as(fg)
        tau = 4.0 * float((e32.double() - e64)[v].abs().max()) if bool(v.any()) else 0.0
        _REFS[name] = dict(valid=valid, fg=fg, v=v, e64=e64, tau=tau, exact=lr.exact(logits, labels, size, ac, IGNORE,
                                                                                      torch.float64)[0])
    return _REFS[name]


def _dev(cuda, name, B):
    """everything the device computes for a case, once: q, the histogram (twice), loss and gradient (twice)"""
    from dcfp_amd import ops
    if (name, B) not in _DEV:
        logits, labels, size, ac = _inputs(name)
        x, lab = logits.to(cuda).requires_grad_(True), labels.to(cuda)
        q = ops.lovasz_errors(x, lab, size, ac, IGNORE)
        hist = [tuple(t.cpu() for t in ops.lovasz_histogram(x, lab, size, ac, IGNORE, B)) for _ in range(2)]
        out = []
        for gout in (None, None, 0.37):
            x.grad = None
            loss = ops.lovasz_softmax(x, lab, size, ac, IGNORE, B)
            assert loss.dim() == 0 and loss.dtype == torch.float32
            loss.backward() if gout is None else loss.backward(torch.tensor(gout, device=cuda))
            out.append((loss.detach().cpu(), x.grad.detach().cpu().clone()))
        _DEV[(name, B)] = dict(q=q.cpu(), hist=hist, runs=out)
    return _DEV[(name, B)]


@pytest.mark.parametrize("name", list(CASES) + list(SPECIAL))
def test_stage1_errors(cuda, name):
    ref, dev = _ref(name), _dev(cuda, name, 1024 if name in SPECIAL else CASES[name][4][0])
    q, v = dev["q"], ref["v"]
    assert q.dtype == torch.int64 and q.shape == ref["e64"].shape
    assert bool((q[~v] == lr.INVALID).all()) and bool((q[v] <= 1 << lr.Q).all())
    if not bool(v.any()):
        return
    err = float((q[v].double() - ref["e64"][v] * 2.0 ** lr.Q).abs().max())
    bound = 0.5 + ref["tau"] * 2.0 ** lr.Q
    print(f"LOVASZ {name} stage1: |q - e64 2^20| max {err:.4f} bound {bound:.4f} (tau {ref['tau']:.3e})")
    assert err <= bound
    if name == "pm80":
        assert int((q[v] == 1 << lr.Q).sum()) > 0 and int((q[v] == 0).sum()) > 0


@pytest.mark.parametrize("name,B", PARAMS)
def test_stage2_histogram(cuda, name, B):
    ref, dev = _ref(name), _dev(cuda, name, B)
    q = torch.where(ref["v"], dev["q"], torch.zeros_like(dev["q"]))
    want = lr.histogram(q, lr.bins_of(q, B), ref["fg"], ref["valid"], B)
    first, second = dev["hist"]
    for got, again, exp, dtype in zip(first, second, want, (torch.int32, torch.int32, torch.int64, torch.int64)):
        assert got.dtype == dtype and got.shape == exp.shape
        assert torch.equal(got.to(torch.int64), exp)
        assert torch.equal(got, again)
    assert int(first[0].sum()) == int(ref["valid"].sum())
    assert int(first[1].sum()) == int(ref["valid"].sum()) * (q.shape[1] - 1)
    if name == "pm80":
        assert int(first[1][:, B - 1].sum()) > 0          # q = 2^20 lands in the last bin, not beyond it


@pytest.mark.parametrize("name,B", PARAMS)
def test_stage3_loss(cuda, name, B):
    ref, dev = _ref(name), _dev(cuda, name, B)
    loss = float(dev["runs"][0][0])
    hist = tuple(t.to(torch.int64) for t in dev["hist"][0])
    want = float(lr.loss_of_histogram(hist, torch.float64))
    L, tau = float(ref["exact"]), ref["tau"]
    print(f"LOVASZ {name} B={B} stage3: device {loss:.9f} fp64-on-its-histogram {want:.9f} exact {L:.9f} tau {tau:.2e}")
    assert loss == loss and abs(loss - want) <= 1e-6 * abs(want)
    r = 2.0 ** -23 * abs(loss)
    assert L - 1.0 / B - 2.0 ** -21 - tau - r <= loss <= L + 2.0 ** -21 + tau + r
    if name == "all-ignored":
        assert loss == 0.0
    if name == "perfect":
        assert loss < 1.0 / B
    if name == "one-class":
        assert int((hist[0].sum(1) > 0).sum()) == 1


@pytest.mark.parametrize("name,B", PARAMS)
def test_stage4_gradient(cuda, name, B):
    ref, dev = _ref(name), _dev(cuda, name, B)
    logits, labels, size, ac = _inputs(name)
    q = torch.where(ref["v"], dev["q"], torch.zeros_like(dev["q"]))
    bins = lr.bins_of(q, B)
    hist = tuple(t.to(torch.int64) for t in dev["hist"][0])
    g64 = lr.binned(logits, labels, size, ac, IGNORE, B, torch.float64, bins=bins, hist=hist)[1]
    g32 = lr.binned(logits, labels, size, ac, IGNORE, B, torch.float32, bins=bins, hist=hist)[1]
    (l1, g1), (l2, g2), (l3, g3) = dev["runs"]
    err, yard = lr.nrel(g1, g64), lr.nrel(g32, g64)
    bound = max(lr.CE_GFLOOR, 3.0 * yard)
    print(f"LOVASZ {name} B={B} stage4: kernel {err:.3e} fp32-yardstick {yard:.3e} bound {bound:.3e}")
    assert bool(torch.isfinite(g1).all()) and err <= bound
    assert torch.equal(l1, l2) and torch.equal(g1, g2)                  # the same bits on a second call
    assert torch.equal(l1, l3)
    assert lr.nrel(g3, 0.37 * g64) <= bound
    assert float((g3 - g1 * torch.tensor(0.37)).abs().max()) <= 2.0 ** -22 * float(g1.abs().max())
    if name == "all-ignored" or logits.shape[1] == 1:                   # one class: p = 1, nothing to move
        assert float(g1.abs().max()) == 0.0
    else:
        assert float(g64.norm()) > 0


@pytest.mark.parametrize("name,B", [("2x19x9x17", 1024), ("1x59x5x9", 64), ("2x19x8x8-noalign", 1024)])
def test_non_contiguous_logits(cuda, name, B):
    from dcfp_amd import ops
    logits, labels, size, ac = _inputs(name)
    N, Cc, h, w = logits.shape
    wide = torch.zeros(N, Cc, h, 2 * w, device=cuda)
    wide[..., ::2] = logits.to(cuda)
    view = wide[..., ::2].requires_grad_(True)
    assert not view.is_contiguous()
    loss = ops.lovasz_softmax(view, labels.to(cuda), size, ac, IGNORE, B)
    loss.backward()
    want_loss, want_grad = _dev(cuda, name, B)["runs"][0]
    assert torch.equal(loss.detach().cpu(), want_loss) and torch.equal(view.grad.cpu(), want_grad)
    assert torch.equal(ops.lovasz_errors(view, labels.to(cuda), size, ac, IGNORE).cpu(), _dev(cuda, name, B)["q"])


def test_a_call_between_forward_and_backward_changes_nothing(cuda):
    """the weight table belongs to the autograd node: another call's histogram does not reach it"""
    from dcfp_amd import ops
    logits, labels, size, ac = _inputs("2x19x7x15")
    other, olab, osize, oac = _inputs("2x19x9x17")
    x = logits.to(cuda).requires_grad_(True)
    loss = ops.lovasz_softmax(x, labels.to(cuda), size, ac, IGNORE, 1024)
    ops.lovasz_softmax(other.to(cuda), olab.to(cuda), osize, oac, IGNORE, 1024)
    loss.backward()
    want_loss, want_grad = _dev(cuda, "2x19x7x15", 1024)["runs"][0]
    assert torch.equal(loss.detach().cpu(), want_loss) and torch.equal(x.grad.cpu(), want_grad)


def test_memory_stays_far_below_the_probabilities(cuda):
    from dcfp_amd import ops
    shape, size = (2, 19, 33, 65), (257, 513)
    logits = lr.make_logits(shape, 3.0, 5).to(cuda).requires_grad_(True)
    labels = torch.randint(0, 19, (2,) + size, generator=torch.Generator().manual_seed(6)).to(cuda)
    ops.lovasz_softmax(logits, labels, size, True, IGNORE, 1024).backward()      # (workspace and allocator warm)
    logits.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = ops.lovasz_softmax(logits, labels, size, True, IGNORE, 1024)
    loss.backward()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    full = 2 * 19 * 257 * 513 * 4
    print(f"LOVASZ memory: peak growth {grown} B, N*C*H*W*4 = {full} B")
    assert bool(torch.isfinite(loss)) and grown < full / 4


def test_argument_errors(cuda):
    from dcfp_amd import ops
    z = torch.zeros(2, 3, 4, 5, device=cuda)
    lab = torch.zeros(2, 9, 11, dtype=torch.int64, device=cuda)
    for fn in (ops.lovasz_softmax, ops.lovasz_histogram):
        for bins in (0, 32, 100, 8192):
            with pytest.raises(ValueError, match="bins"):
                fn(z, lab, (9, 11), True, IGNORE, bins)
    for fn in (ops.lovasz_softmax, ops.lovasz_histogram, ops.lovasz_errors):
        with pytest.raises(RuntimeError, match="float32"):
            fn(z.double(), lab, (9, 11), True)
        with pytest.raises(RuntimeError, match="int64"):
            fn(z, lab.int(), (9, 11), True)
        with pytest.raises(RuntimeError, match="shape"):
            fn(z, lab, (9, 12), True)
        with pytest.raises(ValueError, match="255"):
            fn(torch.zeros(1, 256, 2, 2, device=cuda), lab[:1], (9, 11), True)
