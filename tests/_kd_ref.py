"""Reference of the distillation losses (dcfp_amd/csrc/kd.hip) in torch, and the tolerance rule of the
tests that use it.  A plain helper module like tests/_parity.py: no fixtures, no tests.

kd_ref(student, teacher, T, mode, dtype) evaluates

    pixel:    L = T^2/(N h w) * sum_{n,y,x} sum_c p_t (log p_t - log p_s),   p = softmax_c(logits / T)
    channel:  L = T^2/(N C)   * sum_{n,c} sum_{y,x} q_t (log q_t - log q_s), q = softmax_{y,x}(logits / T)

in `dtype` on the CPU and returns (loss, dL/dstudent by autograd).  float64 is the reference; float32 - the same formula,
the same ops - is the yardstick: what fp32 arithmetic of this formula costs on these inputs.

The rule is the one of tests/test_loss_eval_kernels_gpu.py, with that file's floors: the kernel's distance to fp64 is at
most max(floor, 3 x yardstick), relative (|a - b| / max(1, |b|)) for the loss with CE_FLOOR, norm-relative for the
gradient with CE_GFLOOR; every comparison prints a PARITY line."""
import torch

CE_FLOOR, CE_GFLOOR = 3e-6, 3e-5          # tests/test_loss_eval_kernels_gpu.py

MODES = ("pixel", "channel")


def kd_ref(student, teacher, T, mode, dtype):
    s = student.detach().cpu().to(dtype).clone().requires_grad_(True)
    t = teacher.detach().cpu().to(dtype)
    N, C, h, w = s.shape
    if mode == "pixel":
        ls, lt, count = torch.log_softmax(s / T, dim=1), torch.log_softmax(t / T, dim=1), N * h * w
    elif mode == "channel":
        ls = torch.log_softmax(s.reshape(N, C, h * w) / T, dim=2)
        lt = torch.log_softmax(t.reshape(N, C, h * w) / T, dim=2)
        count = N * C
    else:
        raise ValueError(mode)
    loss = (lt.exp() * (lt - ls)).sum() * (T * T / count)
    loss.backward()
    return loss.detach(), s.grad.detach()


def rel1(a, b):
    """|a - b| / max(1, |b|): the form of the suite's loss comparisons"""
    a, b = float(a), float(b)
    return abs(a - b) / max(1.0, abs(b))


def nrel(a, b):
    """norm-relative distance (absolute where the reference is exactly zero)"""
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    d, n = float((a - b).norm()), float(b.norm())
    return d / n if n > 0 else d


def held(group, case, what, err, yard, floor):
    bound = max(floor, 3.0 * yard)
    msg = f"PARITY {group} {case} {what}: kernel {err:.3e} fp32-yardstick {yard:.3e} bound {bound:.3e}"
    print(msg)
    assert err == err and err <= bound, msg


def check(group, case, loss, grad, ref64, ref32):
    """loss / grad of the code under test against (loss, grad) of kd_ref in fp64, yardstick the fp32 pair."""
    held(group, case, "loss", rel1(loss, ref64[0]), rel1(ref32[0], ref64[0]), CE_FLOOR)
    if grad is not None:
        held(group, case, "dlogits", nrel(grad, ref64[1]), nrel(ref32[1], ref64[1]), CE_GFLOOR)


def logits(shape, seed, scale=2.5):
    """(student, teacher): randn * scale, seeded"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale, torch.randn(*shape, generator=g) * scale
