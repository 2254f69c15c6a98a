"""GPU: the bilinear resize kernels of csrc/resize.hip (the DeepLabv3+ decoder's concat) against fp64 ATen F.interpolate
and its autograd: both align_corners modes, up- and downscaling, a 1x1 source, writes into a channel slice of a
row-pitched buffer (the other channels and the pitch tail untouched), bit-identity with ops.upsample_bilinear on dense
operands, the adjoint read from a slice of a wider tensor, accumulate = 1, run-to-run bit-identity."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [((9, 9), (17, 17)), ((33, 65), (65, 129)), ((64, 128), (128, 256)), ((1, 1), (13, 21)), ((17, 17), (9, 9))]


def _src(N, C, h, w, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, C, h, w, generator=g, dtype=torch.float64).to(dev)


def _pitched(N, Ctot, H, W, pitch, dev):
    from dcfp_amd import ops
    buf = ops.new_pitched((N, Ctot, H, W), pitch, dev)
    return buf


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_forward_into_pitched_slice(cuda, align, src, dst):
    from dcfp_amd import ops
    (h, w), (H, W) = src, dst
    N, C, lo, hi, Ctot = 2, 5, 3, 8, 11
    x64 = _src(N, C, h, w, cuda)
    ref = F.interpolate(x64, size=(H, W), mode="bilinear", align_corners=align)
    pitch = W + 4 + (-(W + 4)) % 4
    buf = _pitched(N, Ctot, H, W, pitch, cuda)
    buf.fill_(7.25)                                           # sentinels in every live float
    full = buf.as_strided((N, Ctot, H, pitch), buf.stride())  # the rows including their tail (zero since allocation)
    assert float(full[..., W:].abs().max()) == 0.0
    ops.resize_bilinear_into(x64.float(), buf[:, lo:hi], align)
    torch.cuda.synchronize()
    got = buf[:, lo:hi].double()
    err = (got - ref).abs().max().item()
    assert err <= 1e-5 * max(1.0, ref.abs().max().item()), err
    assert bool((buf[:, :lo] == 7.25).all()) and bool((buf[:, hi:] == 7.25).all())
    assert float(full[..., W:].abs().max()) == 0.0            # the pitch tail was not written
    # dense operands: the same bits as the existing upsample kernel
    dense = torch.empty(N, C, H, W, device=cuda)
    ops.resize_bilinear_into(x64.float(), dense, align)
    assert torch.equal(dense, ops.upsample_bilinear(x64.float(), (H, W), align))
    assert (dense.double() - got).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("src,dst", SHAPES)
def test_adjoint_vs_fp64_autograd(cuda, align, src, dst):
    from dcfp_amd import ops
    (h, w), (H, W) = src, dst
    N, C, Cwide, lo = 2, 5, 12, 4
    x64 = _src(N, C, h, w, cuda, 1).requires_grad_(True)
    g = torch.Generator().manual_seed(2)
    wide = torch.randn(N, Cwide, H, W, generator=g).to(cuda)          # dy is a channel slice of it, read in place
    dy = wide[:, lo:lo + C]
    F.interpolate(x64, size=(H, W), mode="bilinear", align_corners=align).backward(dy.double())
    ref = x64.grad
    got = ops.resize_bilinear_adjoint(dy, (h, w), align)
    rel = ((got.double() - ref).norm() / ref.norm()).item()
    # (bound: 1e-6, or twice ATen's own fp32 error where its fp32 source coordinates - the index math both follow - cost
    #  more: at 64 -> 128 a coordinate near 64 carries ~4e-6 of rounding)
    x32 = x64.detach().float().requires_grad_(True)
    F.interpolate(x32, size=(H, W), mode="bilinear", align_corners=align).backward(dy)
    aten = ((x32.grad.double() - ref).norm() / ref.norm()).item()
    assert rel <= max(1e-6, 2 * aten), (rel, aten)
    again = ops.resize_bilinear_adjoint(dy, (h, w), align)
    assert torch.equal(got, again)                                   # fixed summation order
    # the per-element gather kernel on a contiguous copy (the A/B baseline): same sums up to rounding
    base = ops.UpsampleBilinearFn.backward(type("Ctx", (), {"cfg": (N, C, h, w, H, W, int(align))})(), dy.contiguous())[0]
    assert ((got - base).double().norm() / base.double().norm()).item() <= max(1e-6, 2 * aten)
    # accumulate = 1 adds into dx
    acc = torch.full((N, C, h, w), 0.5, device=cuda)
    ops.resize_bilinear_adjoint(dy, (h, w), align, out=acc, accumulate=True)
    assert torch.equal(acc, got + 0.5)


def test_adjoint_from_pitched_slice(cuda):
    """dy as a channel slice of a row-pitched buffer (the concat's layout) reads the same values as a dense copy."""
    from dcfp_amd import ops
    N, C, Ctot, h, w, H, W = 2, 6, 10, 33, 65, 65, 129
    buf = ops.new_pitched((N, Ctot, H, W), W + 7 + (-(W + 7)) % 4, cuda)
    g = torch.Generator().manual_seed(3)
    buf.copy_(torch.randn(N, Ctot, H, W, generator=g).to(cuda))
    dy = buf[:, 2:2 + C]
    assert ops._rows(dy)[1] == buf.stride(2)
    for align in (True, False):
        a = ops.resize_bilinear_adjoint(dy, (h, w), align)
        b = ops.resize_bilinear_adjoint(dy.contiguous(), (h, w), align)
        assert torch.equal(a, b)
