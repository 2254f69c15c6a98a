"""GPU: the two kernels of csrc/heads_f16.hip, each against fp64 ATen on the same fp16 inputs (N(0, 3^2) values).

Bounds, per element, derived (not fitted):
  resize:  2 * ((6 + 2 max(h, w)) 2^-24 S + 2^-11 |ref| + 2^-24), S = the same interpolation of |x|: four products and
           three adds in fp32, the fp32 error of the source coordinate (it grows with the source index, hence the
           max(h, w) term - the formula is for these small maps only), the one rounding of the output, the project's
           factor 2.
  pyramid: 2 * ((n + 1) 2^-24 A + 2^-11 |ref| + 2^-24), n = the pixel count of the level's largest window, A = the
           window mean of |x|: any fixed fp32 summation order of n terms, the division, the one rounding, factor 2.
The worst error / bound of every case is printed."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C8S = (8, 40, 520)
RESIZES = [(9, 9, 17, 17), (6, 6, 9, 9), (3, 3, 9, 9), (2, 2, 9, 9), (6, 6, 5, 5), (5, 7, 13, 10)]
MAPS = [(9, 9), (5, 6), (8, 8), (17, 23)]
SIZES = [(1, 2, 3, 6), (1, 8)]
N = 2


def _lib():
    from dcfp_amd import _lib
    return _lib, _lib.lib()


def _nhwc(n, h, w, c8, pitch, off, seed, cuda):
    """fp16 [n, h, w, pitch] of N(0, 9) values everywhere, and the fp64 NCHW view of channels off .. off + c8 - 1."""
    g = torch.Generator().manual_seed(seed)
    x = (3.0 * torch.randn(n, h, w, pitch, generator=g)).to(torch.float16)
    return x.to(cuda), x[..., off:off + c8].double().permute(0, 3, 1, 2).contiguous()


def _resize(L, x, c8, y, y_off, align):
    n, h, w, xp = x.shape
    _, H, W, yp = y.shape
    st = L.dcfp_resize_bilinear_nhwc_f16(C.c_void_p(x.data_ptr()), n, h, w, c8, xp, C.c_void_p(y.data_ptr()), H, W, yp,
                                         y_off, int(align), None)
    assert st == 0, st
    torch.cuda.synchronize()


@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("h,w,H,W", RESIZES)
def test_resize_against_fp64(h, w, H, W, align, cuda, capsys):
    _, L = _lib()
    for c8 in C8S:
        xp, y_off = c8 + 16, 24
        yp = y_off + c8 + 8
        x, x64 = _nhwc(N, h, w, c8, xp, 0, 100 * h + 10 * H + c8, cuda)
        pattern = (torch.arange(N * H * W * yp, dtype=torch.int32) % 2039).to(torch.int16).view(N, H, W, yp)
        y = pattern.view(torch.float16).clone().to(cuda)
        _resize(L, x, c8, y, y_off, align)
        ref = F.interpolate(x64, size=(H, W), mode="bilinear", align_corners=align)
        S = F.interpolate(x64.abs(), size=(H, W), mode="bilinear", align_corners=align)
        bound = 2 * ((6 + 2 * max(h, w)) * 2.0 ** -24 * S + 2.0 ** -11 * ref.abs() + 2.0 ** -24)
        yc = y.cpu()
        got = yc[..., y_off:y_off + c8].double().permute(0, 3, 1, 2)
        ratio = float(((got - ref).abs() / bound).max())
        with capsys.disabled():
            print(f"resize {h}x{w}->{H}x{W} align {int(align)} C8 {c8}: worst error / bound {ratio:.3f}")
        assert torch.isfinite(got).all() and ratio <= 1.0, ratio
        # outside the slice the destination keeps its bits
        keep = torch.ones(yp, dtype=torch.bool)
        keep[y_off:y_off + c8] = False
        assert torch.equal(yc.view(torch.int16)[..., keep], pattern[..., keep])
        # two runs give the same bits
        y2 = pattern.view(torch.float16).clone().to(cuda)
        _resize(L, x, c8, y2, y_off, align)
        assert torch.equal(y2.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("align", [True, False])
def test_resize_of_a_1x1_map_is_the_broadcast_bit_for_bit(align, cuda):
    _, L = _lib()
    H = W = 9
    for c8 in C8S:
        xp, y_off = c8 + 8, 16
        yp = y_off + c8 + 8
        x, _ = _nhwc(N, 1, 1, c8, xp, 0, 7 + c8, cuda)
        x[0, 0, 0, 0], x[1, 0, 0, 1] = -0.0, 6.1e-5                  # a negative zero and a subnormal-range value
        a = torch.zeros(N, H, W, yp, dtype=torch.float16, device=cuda)
        b = torch.zeros_like(a)
        _resize(L, x, c8, a, y_off, align)
        st = L.dcfp_broadcast_nhwc_f16(C.c_void_p(x.data_ptr()), xp, C.c_void_p(b.data_ptr()), N, H * W, c8, yp, y_off,
                                       None)
        assert st == 0
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert torch.equal(a[:, :, :, y_off:y_off + c8], x[:, :, :, :c8].expand(N, H, W, c8))


def _pyramid(L, x, c8, x_off, sizes, cuda, ws=None):
    n, H, W, xp = x.shape
    k = len(sizes)
    sz = (C.c_int * k)(*sizes)
    pitches = [c8 + 8 * (i % 2) for i in range(k)]                   # dense maps, some with a wider pitch
    ys = [torch.full((n, s, s, p), 77.0, dtype=torch.float16, device=cuda) for s, p in zip(sizes, pitches)]
    need = int(L.dcfp_pyramid_pool_nhwc_f16_workspace_bytes(n, H, W, c8, k, sz))
    assert need > 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    st = L.dcfp_pyramid_pool_nhwc_f16(C.c_void_p(x.data_ptr()), n, H, W, c8, xp, x_off, k, sz,
                                      (C.c_void_p * k)(*[y.data_ptr() for y in ys]), (C.c_int * k)(*pitches),
                                      C.c_void_p(ws.data_ptr()), need, None)
    assert st == 0, st
    torch.cuda.synchronize()
    return ys


@pytest.mark.parametrize("sizes", SIZES)
@pytest.mark.parametrize("H,W", MAPS)
def test_pyramid_pool_against_fp64(H, W, sizes, cuda, capsys):
    _, L = _lib()
    for c8 in C8S:
        x_off = 16
        xp = x_off + c8 + 8
        x, x64 = _nhwc(N, H, W, c8, xp, x_off, 1000 * H + 10 * W + c8 + len(sizes), cuda)
        ys = _pyramid(L, x, c8, x_off, sizes, cuda)
        again = _pyramid(L, x, c8, x_off, sizes, cuda)
        for s, y, y2 in zip(sizes, ys, again):
            ref = F.adaptive_avg_pool2d(x64, s)
            A = F.adaptive_avg_pool2d(x64.abs(), s)
            n_win = max(-(-(i + 1) * H // s) - i * H // s for i in range(s)) * \
                max(-(-(j + 1) * W // s) - j * W // s for j in range(s))
            bound = 2 * ((n_win + 1) * 2.0 ** -24 * A + 2.0 ** -11 * ref.abs() + 2.0 ** -24)
            yc = y.cpu()
            got = yc[..., :c8].double().permute(0, 3, 1, 2)
            ratio = float(((got - ref).abs() / bound).max())
            with capsys.disabled():
                print(f"pyramid {H}x{W} sizes {sizes} level {s} C8 {c8}: worst error / bound {ratio:.3f} "
                      f"(largest window {n_win} pixels)")
            assert torch.isfinite(got).all() and ratio <= 1.0, (s, ratio)
            assert bool((yc[..., c8:] == 77.0).all())                # channels past C8 are not touched
            assert torch.equal(y2.view(torch.int16), y.view(torch.int16))   # two runs: the same bits


def test_pyramid_pool_does_not_write_past_its_workspace(cuda):
    _lib_, L = _lib()
    H, W, c8, sizes = 17, 23, 40, (1, 2, 3, 6)
    x, _ = _nhwc(N, H, W, c8, c8, 0, 5, cuda)
    sz = (C.c_int * 4)(*sizes)
    need = int(L.dcfp_pyramid_pool_nhwc_f16_workspace_bytes(N, H, W, c8, 4, sz))
    ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=cuda)
    _pyramid(L, x, c8, 0, sizes, cuda, ws=ws)
    assert bool((ws[need:] == 0x5A).all())
