"""Reference of the binned Lovasz-Softmax loss (dcfp_amd/csrc/lovasz.hip) in torch, the exact sort-based
loss of the paper, and the fixtures the tests share.  A plain helper module like tests/_kd_ref.py: no fixtures, no tests.

The definition (Q = 20, B bins).  A pixel is valid when its label lies in [0, C) and is not ignore_index.  With
z = F.interpolate(logits, size, 'bilinear'), p = softmax_c(z), per valid pixel and class
    f = [label == c],   e = f ? 1 - p_c : p_c,   q = min(2^Q, floor(e 2^Q + 0.5)),   b = min(B - 1, q >> (Q - log2 B)).
Per class and bin: nF / nB = number of pixels with f = 1 / 0, SF / SB = sums of their q.  G = sum_b nF; a class is present
when G > 0.  From bin B - 1 down, F_above / G_above the counts of the higher bins:
    I0 = G - F_above, U0 = G + G_above, I1 = I0 - nF[b], U1 = U0 + nB[b],
    wF[b] = (1/U0 + 1/U1) / 2,   wB[b] = (I0 + I1) / (2 U0 U1),
    loss = mean over present classes of 2^-Q sum_b (wF SF + wB SB);   no class present: 0.
Gradient: the weights are constants, the rounding of e to q is passed straight through.

Everything is evaluated in `dtype` on the CPU: float64 is the reference, float32 - the same ops - the yardstick.
The exact loss (Berman, Triki, Blaschko, CVPR 2018, Algorithm 1 and eq. 9, classes = 'present'): per present class sort
the errors in decreasing order, J_k = 1 - (G - F_k) / (G + K_k) with F_k / K_k the foreground / background pixels among
the first k, loss_c = sum_k e_(k) (J_k - J_(k-1))."""
import torch
import torch.nn.functional as F

Q = 20
CE_GFLOOR = 3e-5           # tests/test_loss_eval_kernels_gpu.py, tests/test_kd_gpu.py
INVALID = 0xFFFFFFFF


def probs(logits, size, align_corners, dtype):
    """softmax of the upsampled logits [N,C,H,W] in `dtype` (differentiable in `logits`)"""
    z = F.interpolate(logits.to(dtype), size=tuple(size), mode="bilinear", align_corners=bool(align_corners))
    return torch.softmax(z, dim=1)


def masks(labels, C, ignore_index):
    """-> (valid [N,H,W] bool, fg [N,C,H,W] bool)"""
    valid = (labels >= 0) & (labels < C) & (labels != ignore_index)
    fg = labels.unsqueeze(1) == torch.arange(C).view(1, C, 1, 1)
    return valid, fg & valid.unsqueeze(1)


def errors(p, fg):
    return torch.where(fg, 1 - p, p)


def quantise(e):
    return torch.clamp(torch.floor(e.detach() * float(1 << Q) + 0.5), max=float(1 << Q)).to(torch.int64)


def bins_of(q, B):
    shift = Q - (B.bit_length() - 1)
    return torch.clamp(q >> shift, max=B - 1)


def histogram(q, b, fg, valid, B):
    """-> (nF, nB, SF, SB), int64 [C, B]"""
    N, C, H, W = q.shape
    out = []
    v = valid.unsqueeze(1).expand_as(fg)
    idx = (torch.arange(C).view(1, C, 1, 1) * B + b)
    for sel in (fg & v, ~fg & v):
        n = torch.bincount(idx[sel], minlength=C * B).reshape(C, B)
        s = torch.zeros(C * B, dtype=torch.int64).scatter_add_(0, idx[sel], q[sel]).reshape(C, B)
        out.append((n, s))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def weights(nF, nB, dtype):
    """-> (wF, wB [C,B] in dtype, zeros for absent classes; present [C] bool)"""
    G = nF.sum(1, keepdim=True)
    above = lambda n: torch.flip(torch.cumsum(torch.flip(n, [1]), 1), [1]) - n      # counts of the higher bins
    I0, U0 = G - above(nF), G + above(nB)
    I1, U1 = I0 - nF, U0 + nB
    present = G[:, 0] > 0
    U0d, U1d = U0.to(dtype).clamp(min=1), U1.to(dtype).clamp(min=1)
    wF = (1 / U0d + 1 / U1d) / 2
    wB = (I0 + I1).to(dtype) / (2 * U0d * U1d)
    keep = present.view(-1, 1).to(dtype)
    return wF * keep, wB * keep, present


def loss_of_histogram(hist, dtype):
    nF, nB, SF, SB = hist
    wF, wB, present = weights(nF, nB, dtype)
    P = int(present.sum())
    if P == 0:
        return torch.zeros((), dtype=dtype)
    per_class = (wF * SF.to(dtype) + wB * SB.to(dtype)).sum(1) / float(1 << Q)
    return per_class.sum() / P


def binned(logits, labels, size, align_corners, ignore_index, B, dtype, bins=None, hist=None):
    """-> (loss, dloss/dlogits) of the definition in `dtype`.  bins [N,C,H,W] and hist = (nF, nB, SF, SB) replace the
    ones this function would compute from its own probabilities (the device's, in the per-stage tests)."""
    x = logits.detach().cpu().to(dtype).clone().requires_grad_(True)
    C = x.shape[1]
    valid, fg = masks(labels.cpu(), C, ignore_index)
    p = probs(x, size, align_corners, dtype)
    e = errors(p, fg)
    q = quantise(e)
    b = bins_of(q, B) if bins is None else bins.cpu()
    if hist is None:
        hist = histogram(q, b, fg, valid, B)
    loss = loss_of_histogram(hist, dtype)
    wF, wB, present = weights(hist[0], hist[1], dtype)
    P = max(int(present.sum()), 1)
    cidx = torch.arange(C).view(1, C, 1, 1).expand_as(b)
    w = torch.where(fg, wF[cidx, b], wB[cidx, b]) * valid.unsqueeze(1)
    (w.detach() * e).sum().div(P).backward()
    return loss.detach(), x.grad.detach()


def exact_from_errors(e, fg, valid):
    """The paper's loss from errors [N,C,H,W] (any dtype; differentiable), classes = 'present'."""
    C = e.shape[1]
    v = valid.reshape(-1)
    losses = []
    for c in range(C):
        ec, fc = e[:, c].reshape(-1)[v], fg[:, c].reshape(-1)[v].to(e.dtype)
        G = fc.sum()
        if float(G) == 0:
            continue
        es, order = torch.sort(ec, descending=True)
        fs = fc[order]
        inter = G - torch.cumsum(fs, 0)
        union = G + torch.cumsum(1 - fs, 0)
        jac = 1 - inter / union
        grad = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append((es * grad).sum())
    if not losses:
        return torch.zeros((), dtype=e.dtype)
    return torch.stack(losses).mean()


def exact(logits, labels, size, align_corners, ignore_index, dtype):
    """-> (loss, dloss/dlogits) of the sort-based loss in `dtype`"""
    x = logits.detach().cpu().to(dtype).clone().requires_grad_(True)
    valid, fg = masks(labels.cpu(), x.shape[1], ignore_index)
    loss = exact_from_errors(errors(probs(x, size, align_corners, dtype), fg), fg, valid)
    if loss.requires_grad:
        loss.backward()
        return loss.detach(), x.grad.detach()
    return loss.detach(), torch.zeros_like(x)


def nrel(a, b):
    """norm-relative distance (absolute where the reference is exactly zero)"""
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    d, n = float((a - b).norm()), float(b.norm())
    return d / n if n > 0 else d


def make_labels(logits, size, align_corners, seed, ignored=0.1, agree=0.6, ignore_index=255):
    """labels [N,H,W]: the prediction's argmax at `agree` of the pixels, a random class elsewhere, `ignored` of them
    ignore_index"""
    g = torch.Generator().manual_seed(seed)
    N, C = logits.shape[:2]
    H, W = size
    lab = torch.randint(0, C, (N, H, W), generator=g)
    pred = probs(logits, size, align_corners, torch.float64).argmax(1)
    take = torch.rand(N, H, W, generator=g) < agree
    lab[take] = pred[take]
    lab[torch.rand(N, H, W, generator=g) < ignored] = ignore_index
    return lab


def make_logits(shape, scale, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale
