"""Reference of the pair-wise similarity distillation (dcfp_amd/csrc/pairwise.hip) in torch, and the
inputs and the tolerance rule of the tests that use it.  A plain helper module like tests/_kd_ref.py: no fixtures, no
tests.

pa_ref(student, teacher, pool, dtype, teacher_channels=None) evaluates, in `dtype` on the CPU,

    nodes   u_p  = mean over the in-range part of the pool x pool window p, per channel
    f_p     = u_p / r_p, r_p^2 = sum_c u_p[c]^2, and f_p = 0 where r_p^2 <= 1e-12 (a dead node)
    L       = 1/(N P^2) sum_n sum_pq (f^S_p . f^S_q - f^T_p . f^T_q)^2
    g_p     = 4/(N P^2) sum_q D_pq f^S_q,  du_p = (g_p - f_p (f_p . g_p)) / r_p (0 for a dead node),
    dS[n,c,y,x] = du_{p(y,x)}[c] / |window_p|

with explicit window loops and the closed-form gradient (no autograd, no avg_pool2d: the tests hold it against those).
The teacher is fp32 [N,Ct,h,w] or fp16 [N,h,w,pitch] (upcast exactly; its first `teacher_channels` channels count).
float64 is the reference; float32 - the same formula, the same ops - is the yardstick.

The rule is the one of tests/test_loss_eval_kernels_gpu.py / _kd_ref.py with their floors: distance to fp64 at most
max(floor, 3 x yardstick), relative (|a - b| / max(1, |b|)) for the loss, norm-relative for the gradient."""
import torch

from _kd_ref import CE_FLOOR, CE_GFLOOR, held, nrel, rel1  # noqa: F401

DEAD = 1e-12
SHARES = []                 # (group, case, what, err / bound) of every check() of this process


def teacher_nchw(teacher, dtype, teacher_channels=None):
    """The teacher as [N,Ct,h,w] in `dtype` (an fp16 NHWC teacher is upcast exactly and cut to its channels)."""
    t = teacher.detach().cpu()
    if t.dtype == torch.float16:
        ct = t.shape[3] if teacher_channels is None else teacher_channels
        return t[..., :ct].permute(0, 3, 1, 2).to(dtype)
    return t.to(dtype)


def nodes(x, pool):
    """(u [N,C,P], window sizes [P], node index of every pixel [h,w]) by explicit window loops"""
    N, C, h, w = x.shape
    hp, wp = -(-h // pool), -(-w // pool)
    u = x.new_zeros(N, C, hp * wp)
    cnt = torch.zeros(hp * wp, dtype=x.dtype)
    index = torch.zeros(h, w, dtype=torch.int64)
    for i in range(hp):
        for j in range(wp):
            y0, y1, x0, x1 = i * pool, min(h, (i + 1) * pool), j * pool, min(w, (j + 1) * pool)
            cnt[i * wp + j] = (y1 - y0) * (x1 - x0)
            u[:, :, i * wp + j] = x[:, :, y0:y1, x0:x1].sum(dim=(2, 3)) / cnt[i * wp + j]
            index[y0:y1, x0:x1] = i * wp + j
    return u, cnt, index


def normalise(u):
    """(f [N,C,P], 1/r [N,1,P] with 0 for a dead node)"""
    r2 = (u * u).sum(dim=1, keepdim=True)
    alive = r2 > DEAD
    inv = torch.where(alive, 1.0 / torch.sqrt(torch.where(alive, r2, torch.ones_like(r2))), torch.zeros_like(r2))
    return u * inv, inv


def pa_ref(student, teacher, pool, dtype, teacher_channels=None):
    """(loss, dL/dstudent) in `dtype`, closed form"""
    s = student.detach().cpu().to(dtype)
    t = teacher_nchw(teacher, dtype, teacher_channels)
    N, C, h, w = s.shape
    us, cnt, index = nodes(s, pool)
    ut, _, _ = nodes(t, pool)
    fs, inv = normalise(us)
    ft, _ = normalise(ut)
    P = us.shape[2]
    D = torch.einsum("ncp,ncq->npq", fs, fs) - torch.einsum("ncp,ncq->npq", ft, ft)
    loss = (D * D).sum() / (N * P * P)
    g = torch.einsum("npq,ncq->ncp", D, fs) * (4.0 / (N * P * P))
    du = (g - fs * (fs * g).sum(dim=1, keepdim=True)) * inv
    ds = (du / cnt)[:, :, index.reshape(-1)].reshape(N, C, h, w)
    return loss, ds


def pa_autograd(student, teacher, pool, dtype, eps=None):
    """(loss, gradient by autograd) of an independent statement: avg_pool2d(ceil_mode, count_include_pad False),
    normalisation, einsum.  eps None: F.normalize (no dead-node rule: for inputs without dead nodes); a number: the
    smooth variant u / sqrt(r^2 + eps^2)."""
    import torch.nn.functional as F
    s = student.detach().cpu().to(dtype).clone().requires_grad_(True)
    t = teacher_nchw(teacher, dtype)

    def gram(x):
        u = F.avg_pool2d(x, pool, pool, ceil_mode=True, count_include_pad=False).flatten(2)
        f = F.normalize(u, dim=1, eps=0.0) if eps is None else u / torch.sqrt((u * u).sum(1, keepdim=True) + eps * eps)
        return torch.einsum("ncp,ncq->npq", f, f)
    D = gram(s) - gram(t)
    loss = (D * D).mean()
    loss.backward()
    return loss.detach(), s.grad.detach()


def check(group, case, loss, grad, ref64, ref32):
    """loss / grad of the code under test against pa_ref in fp64, yardstick the fp32 pair; records the shares"""
    pairs = [("loss", rel1(loss, ref64[0]), rel1(ref32[0], ref64[0]), CE_FLOOR)]
    if grad is not None:
        pairs.append(("dstudent", nrel(grad, ref64[1]), nrel(ref32[1], ref64[1]), CE_GFLOOR))
    for what, err, yard, floor in pairs:
        SHARES.append((group, case, what, err / max(floor, 3.0 * yard)))
        held(group, case, what, err, yard, floor)


def features(shape_s, shape_t, seed, dead=(), scale=1.0):
    """(student [N,Cs,h,w], teacher [N,Ct,h,w]): post-ReLU randn * scale, seeded; the pixels listed in `dead` (n, y, x)
    are set to zero in every channel of the student."""
    g = torch.Generator().manual_seed(seed)
    s = torch.relu(torch.randn(*shape_s, generator=g)) * scale
    t = torch.relu(torch.randn(*shape_t, generator=g)) * scale
    for n, y, x in dead:
        s[n, :, y, x] = 0.0
    return s, t


def assert_nodes_clear_of_threshold(x, pool):
    """The condition on the inputs: a node is exactly zero, or its norm is at least 1e-3 - rounding cannot move a node
    across the dead-node threshold r^2 = 1e-12."""
    u, _, _ = nodes(x.detach().cpu().double(), pool)
    r = (u * u).sum(dim=1).sqrt()
    assert bool(((r == 0) | (r >= 1e-3)).all()), float(r[r > 0].min())
    return int((r == 0).sum())
