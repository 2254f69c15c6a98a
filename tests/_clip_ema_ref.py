"""Shared by test_clip_ema_host_cpu.py and test_clip_ema_gpu.py: a numpy / torch-CPU restatement of what
dcfp_amd/csrc/clip_ema.hip computes, one rounding per operation, and the tensor layout of the kernel tests.

    sqnorm = sum_i double(g_i)^2           sequentially in fp64 (each square is exact: 48 significant bits)
    norm   = float(math.sqrt(sqnorm))
    coef   = min(1, fl(max_norm / fl(norm + 1e-6f)))           (a NaN stays a NaN)
    g'     = fl(g * coef)                                      then the plain optimizer's lines on g'
    ema    = fma(w, fl(p_new - ema), ema),  w = float(1 - double(decay)) < 0.5      (torch.lerp's first form)

A plain helper module like tests/_adamw_cases.py: no fixtures, no tests."""
import math

import numpy as np
import torch

CHUNK = 16384
SIZES = [1, 3, 4, 5, 16383, 16384, 16385, 40000]
GROUP_OF = [0, 0, 0, 0, 1, 1, 0, 1]                 # two param groups (different weight decay)
NO_GRAD = 1                                         # index into SIZES of the parameter whose grad is None
SENT = np.float32(-12345.678)
F = np.float32


def sqnorm64(arrays):
    """Sequential fp64 sum of the exact squares, tensor by tensor: (total, [per tensor])."""
    per = [math.fsum((np.asarray(a, np.float64).ravel() ** 2).tolist()) for a in arrays]
    return math.fsum(per), per


def norm32(sqnorm):
    with np.errstate(over="ignore"):
        return F(math.sqrt(sqnorm)) if not math.isnan(sqnorm) else F(np.nan)


def coef32(norm, max_norm):
    """torch's clip coefficient from an fp32 norm: two fp32 operations and the clamp."""
    with np.errstate(over="ignore", invalid="ignore"):
        c = F(max_norm) / (F(norm) + F(1e-6))
    assert c.dtype == np.float32
    return F(1.0) if c > F(1.0) else c


def lerp32(ema, p, decay):
    """torch.lerp(ema, p, 1 - decay) for a weight < 0.5: ema + w * (p - ema), the product and sum fused (one rounding),
    evaluated in fp64 - exact for an fp32 product plus an fp32 addend up to the final rounding's double-rounding, which
    the callers avoid by comparing against torch.lerp itself; this form is for the CPU sanity test only."""
    w = F(1.0 - float(decay))
    assert w < F(0.5)
    d = (p.astype(np.float32) - ema.astype(np.float32)).astype(np.float32)
    return (w.astype(np.float64) * d.astype(np.float64) + ema.astype(np.float64)).astype(np.float32)


def sgd32(p, g, buf, coef, lr, momentum, wd):
    """Clipped SGD per operation in fp32, the kernel's lines: g' = fl(g*coef); g'' = fma(wd, p, g');
    buf = fma(buf, momentum, g''); p = fma(-lr, buf, p).  The fmas are formed in fp64 and rounded once (an fp32 product
    is exact in fp64; the sum's double rounding can differ in the last bit in rare cases, so callers compare to 1 ulp)."""
    f64 = np.float64
    g1 = (g * F(coef)).astype(np.float32)
    if wd != 0.0:
        g1 = (f64(F(wd)) * p.astype(f64) + g1.astype(f64)).astype(np.float32)
    b1 = (buf.astype(f64) * f64(F(momentum)) + g1.astype(f64)).astype(np.float32)
    p1 = (-f64(F(lr)) * b1.astype(f64) + p.astype(f64)).astype(np.float32)
    return p1, b1


def adamw32(p, g, m, v, coef, sc):
    """Clipped AdamW: g' = fl(g*coef), then tests/_adamw_cases.restate32 (the kernel's lines without fma)."""
    import _adamw_cases as ac
    return ac.restate32(p, (g * F(coef)).astype(np.float32), m, v, sc)


# ------------------------------------------------------------------------------------------------ the kernel-test layout
def residues():
    """Start residue (floats off a 16-byte boundary) of each tensor: 0..3 in turn, the big ones at 0 and at 1..3."""
    return [i % 4 for i in range(len(SIZES))]


def layout(shift=0):
    """(offsets, total) of the tensors in one flat buffer whose base is 256-byte aligned: tensor i starts at residue
    (residues()[i] + shift) % 4, with at least 5 sentinel floats in front of it."""
    offs, off = [], 0
    for n, r in zip(SIZES, residues()):
        off += 5
        off += ((r + shift) - off) % 4
        offs.append(off)
        off += n
    return offs, off + 8


def chunks_of(sizes):
    first, c = [], 0
    for n in sizes:
        first.append(c)
        c += (n + CHUNK - 1) // CHUNK
    return first, c


def values(kind, seed=0):
    """The gradient value sets of the issue, one fp32 array per tensor of SIZES."""
    rng = np.random.RandomState(1000 + seed)
    out = []
    for i, n in enumerate(SIZES):
        if kind in ("randn", "inf", "nan"):
            a = rng.randn(n).astype(np.float32)
        elif kind == "tiny":
            a = np.full(n, 1e-30, np.float32)
        elif kind == "huge":
            a = np.full(n, 1e25, np.float32)
        else:
            raise KeyError(kind)
        out.append(a)
    if kind == "inf":
        out[6][16384] = np.inf                      # the one element of tensor 6's second chunk
    if kind == "nan":
        out[7][39999] = np.nan                      # a tail element
    return out


def torch_bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        bool((a.detach().reshape(-1).contiguous().view(torch.uint8) == b.detach().reshape(-1).contiguous().view(torch.uint8)).all())
