"""GPU: the kernels of csrc/conv_f16.hip one by one against fp64.

Inputs and weights are drawn in fp32 and rounded to fp16 FIRST; the fp64 reference is computed from the rounded
values, so the kernel and the reference see identical numbers.  Products of two fp16 values are exact in fp32, hence
the kernel's error is fp32 accumulation plus the single output rounding: with K = Cin*kh*kw and
S = conv(|x|, |w|) + |shift| + |residual|,
    |y - ref| <= 2 * ((K + 2) * 2^-24 * S + 2^-11 * |ref| + 2^-24)        per element
(the 2^-11 term dropped for the fp32-output classifier variant; the factor 2 covers a pre-rounding value that sits on
a rounding boundary).  Derived, not tuned.  The maxpool, the converter and the broadcast are exact (bitwise); the
average pool is held to 2 * ((HW + 1) * 2^-24 * mean|x| + 2^-11 * |ref|)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B5A      # an fp16 bit pattern no kernel output below equals by accident (60224.0)


def _r8(c):
    return (c + 7) // 8 * 8


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nhwc16(x, pitch=None):
    """fp16-valued [N,C,H,W] (CPU) -> NHWC fp16 with `pitch` channels (zeros in the padding)."""
    N, Cc, H, W = x.shape
    out = torch.zeros((N, H, W, pitch or _r8(Cc)), dtype=torch.float16)
    out[..., :Cc] = x.permute(0, 2, 3, 1).to(torch.float16)
    return out


def _pack(w):
    """fp16-valued [Cout,Cin,k,k] -> [Cout8][kh][kw][Cin8] fp16, zeros in the padding."""
    co, ci, kh, kw = w.shape
    out = torch.zeros((_r8(co), kh, kw, _r8(ci)), dtype=torch.float16)
    out[:co, :, :, :ci] = w.permute(0, 2, 3, 1).to(torch.float16)
    return out


def _draw(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(torch.float16).to(torch.float64)


def _case(cuda, N, cin, cout, H, W, k, stride, pad, dil, relu=True, residual=False, y_pitch=None, y_off=0, f32=False,
          seed=0):
    from dcfp_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(1000 + seed)
    Kred = cin * k * k
    x = _draw((N, cin, H, W), gen)
    w = _draw((cout, cin, k, k), gen, Kred ** -0.5)
    shift = (torch.randn(cout, generator=gen) * 0.5).float()
    ref = F.conv2d(x, w, None, stride, pad, dil)
    S = F.conv2d(x.abs(), w.abs(), None, stride, pad, dil) + shift.double().abs().view(1, -1, 1, 1)
    ref = ref + shift.double().view(1, -1, 1, 1)
    Ho, Wo = ref.shape[2:]
    res = None
    if residual:
        res = _draw((N, cout, Ho, Wo), gen)
        ref, S = ref + res, S + res.abs()
    if relu and not f32:
        ref = F.relu(ref)
    cout8 = _r8(cout)
    sh = torch.zeros(cout8)
    sh[:cout] = shift
    y_pitch = y_pitch or cout8
    d = _lib.ConvF16Desc(N, H, W, _r8(cin), _r8(cin), cout if f32 else cout8, k, stride, pad, dil, Ho, Wo,
                         0 if f32 else y_pitch, y_off, cout8 if residual else 0, 0, int(relu))
    xd, wd, shd = _nhwc16(x).to(cuda), _pack(w).to(cuda), sh.to(cuda)
    if f32:
        y = torch.full((N, cout, Ho, Wo), float("nan"), device=cuda)
        st = L.dcfp_conv2d_fwd_f16_nhwc_to_f32_nchw(C.byref(d), _p(xd), _p(wd), _p(shd), _p(y), _stream())
        assert st == 0, st
        got = y.double().cpu()
        bound = 2 * ((Kred + 2) * 2.0 ** -24 * S + 2.0 ** -24)
    else:
        y = torch.full((N, Ho, Wo, y_pitch), SENTINEL, dtype=torch.int16, device=cuda).view(torch.float16)
        rd = _nhwc16(res).to(cuda) if residual else None
        st = L.dcfp_conv2d_fwd_f16_nhwc(C.byref(d), _p(xd), _p(wd), _p(shd), _p(rd), _p(y), _stream())
        assert st == 0, st
        yc = y.cpu()
        got = yc[..., y_off:y_off + cout].permute(0, 3, 1, 2).double()
        # padded output channels hold exact zeros; everything outside the slice keeps its bytes
        assert (yc[..., y_off + cout:y_off + cout8].view(torch.int16) == 0).all()
        outside = torch.cat([yc[..., :y_off], yc[..., y_off + cout8:]], dim=-1).view(torch.int16)
        assert (outside == SENTINEL).all()
        bound = 2 * ((Kred + 2) * 2.0 ** -24 * S + 2.0 ** -11 * ref.abs() + 2.0 ** -24)
    err = (got - ref).abs()
    assert torch.isfinite(got).all()
    worst = float((err / bound).max())
    print(f"conv_f16 {cin}->{cout} k{k} s{stride} d{dil} {H}x{W}: max err {float(err.max()):.3e}, "
          f"worst err/bound {worst:.3f}")
    assert worst <= 1.0, worst


CASES = {
    "1x1_ragged_pixel_tile": dict(N=2, cin=64, cout=256, H=9, W=13, k=1, stride=1, pad=0, dil=1),
    "1x1_stride2_downsample": dict(N=2, cin=256, cout=512, H=17, W=17, k=1, stride=2, pad=0, dil=1, relu=False),
    "3x3_pruned_widths": dict(N=2, cin=47, cout=95, H=9, W=13, k=3, stride=1, pad=1, dil=1),
    "3x3_stride2_stem": dict(N=2, cin=3, cout=64, H=65, W=65, k=3, stride=2, pad=1, dil=1),
    "3x3_dilation2": dict(N=2, cin=128, cout=64, H=9, W=13, k=3, stride=1, pad=2, dil=2),
    "3x3_dilation12": dict(N=2, cin=128, cout=64, H=9, W=13, k=3, stride=1, pad=12, dil=12),
    "3x3_k_tail": dict(N=1, cin=264, cout=72, H=5, W=7, k=3, stride=1, pad=1, dil=1),
    "1x1_residual_relu": dict(N=2, cin=64, cout=256, H=9, W=13, k=1, stride=1, pad=0, dil=1, residual=True),
    "1x1_channel_slice": dict(N=2, cin=64, cout=256, H=9, W=13, k=1, stride=1, pad=0, dil=1, y_pitch=1280, y_off=256),
    "1x1_classifier_f32_nchw": dict(N=2, cin=256, cout=19, H=9, W=13, k=1, stride=1, pad=0, dil=1, f32=True),
}


@pytest.mark.parametrize("tag", list(CASES))
def test_conv_f16_against_fp64(cuda, tag):
    _case(cuda, seed=list(CASES).index(tag), **CASES[tag])


@pytest.mark.parametrize("N,Cc,H,W,pitch", [(2, 24, 13, 17, 24), (1, 8, 6, 8, 16), (2, 64, 33, 33, 64)])
def test_maxpool_nhwc_f16_is_exact(cuda, N, Cc, H, W, pitch):
    from dcfp_amd import _lib
    gen = torch.Generator().manual_seed(7)
    x = _draw((N, Cc, H, W), gen)
    ref = F.max_pool2d(x, 3, 2, 1)
    Ho, Wo = ref.shape[2:]
    xd = _nhwc16(x, pitch).to(cuda)
    y = torch.full((N, Ho, Wo, pitch), SENTINEL, dtype=torch.int16, device=cuda).view(torch.float16)
    st = _lib.lib().dcfp_maxpool3x3s2_nhwc_f16(_p(xd), _p(y), N, H, W, Cc, pitch, Ho, Wo, pitch, _stream())
    assert st == 0, st
    yc = y.cpu()
    want = ref.permute(0, 2, 3, 1).to(torch.float16)
    assert torch.equal(yc[..., :Cc].view(torch.int16), want.contiguous().view(torch.int16))
    assert (yc[..., Cc:].view(torch.int16) == SENTINEL).all()


@pytest.mark.parametrize("N,Cc,H,W", [(2, 3, 9, 13), (1, 19, 5, 7), (2, 3, 65, 65)])
def test_input_converter_is_exact(cuda, N, Cc, H, W):
    from dcfp_amd import _lib
    x = torch.randn((N, Cc, H, W), generator=torch.Generator().manual_seed(3)) * 3
    c8 = _r8(Cc)
    y = torch.full((N, H, W, c8), SENTINEL, dtype=torch.int16, device=cuda).view(torch.float16)
    st = _lib.lib().dcfp_nchw_f32_to_nhwc_f16(_p(x.to(cuda)), _p(y), N, Cc, H, W, c8, _stream())
    assert st == 0, st
    want = torch.zeros((N, H, W, c8), dtype=torch.float16)
    want[..., :Cc] = x.permute(0, 2, 3, 1).to(torch.float16)
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16))


def test_broadcast_into_a_channel_slice_is_exact(cuda):
    from dcfp_amd import _lib
    N, c8, H, W, pitch, off = 2, 152, 9, 13, 1280, 1024
    v = torch.zeros((N, 160), dtype=torch.float16)
    v[:, :c8] = torch.randn((N, c8), generator=torch.Generator().manual_seed(5)).to(torch.float16)
    y = torch.full((N, H, W, pitch), SENTINEL, dtype=torch.int16, device=cuda).view(torch.float16)
    st = _lib.lib().dcfp_broadcast_nhwc_f16(_p(v.to(cuda)), 160, _p(y), N, H * W, c8, pitch, off, _stream())
    assert st == 0, st
    yc = y.cpu()
    want = v[:, :c8].view(N, 1, 1, c8).expand(N, H, W, c8).contiguous()
    assert torch.equal(yc[..., off:off + c8].contiguous().view(torch.int16), want.view(torch.int16))
    outside = torch.cat([yc[..., :off], yc[..., off + c8:]], dim=-1).view(torch.int16)
    assert (outside == SENTINEL).all()


@pytest.mark.parametrize("N,Cc,H,W", [(2, 264, 9, 13), (2, 264, 70, 70), (1, 2048, 17, 17)])
def test_avgpool_nhwc_f16_against_fp64(cuda, N, Cc, H, W):
    """fp32 accumulation, one rounding: 2 * ((HW + 1) * 2^-24 * mean|x| + 2^-11 * |ref|).  70 x 70 takes the split
    (several partial sums per image) path, 9 x 13 the single one."""
    from dcfp_amd import _lib
    L = _lib.lib()
    x = _draw((N, Cc, H, W), torch.Generator().manual_seed(11)) + 0.25
    x = x.to(torch.float16).double()
    HW = H * W
    ref = x.mean(dim=(2, 3))
    bound = 2 * ((HW + 1) * 2.0 ** -24 * x.abs().mean(dim=(2, 3)) + 2.0 ** -11 * ref.abs())
    nbytes = int(L.dcfp_avgpool_nhwc_f16_workspace_bytes(N, Cc, HW))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    y = torch.full((N, Cc), SENTINEL, dtype=torch.int16, device=cuda).view(torch.float16)
    st = L.dcfp_avgpool_nhwc_f16(_p(_nhwc16(x).to(cuda)), _p(y), N, HW, Cc, Cc, Cc, _p(ws), nbytes, _stream())
    assert st == 0, st
    err = (y.cpu().double() - ref).abs()
    worst = float((err / bound).max())
    print(f"avgpool_f16 {Cc} x {H}x{W}: max err {float(err.max()):.3e}, worst err/bound {worst:.3f}")
    assert worst <= 1.0, worst
