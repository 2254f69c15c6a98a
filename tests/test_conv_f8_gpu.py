"""GPU: the kernels of csrc/conv_f8.hip one by one against fp64.

Operands are drawn and quantised to e4m3 FIRST; the fp64 reference is computed from the quantised values, so the kernel
and the reference see identical numbers.  Products of two e4m3 values are exact in fp32, hence the conv's error is fp32
accumulation, the epilogue's few fp32 operations and the single output rounding: with K = Cin*k*k and
S = conv(|x|, |w|) * |mul| + |add| + |res_mul * res|,
    fp8 output:  |y - ref| <= 2 * ((K + 2) * 2^-24 * S + 2^-4 * |ref| + 2^-10)     where |ref| <= 448
                 y == +-448 exactly                                                 where |ref| >= 480
    fp32 output: |y - ref| <= 2 * ((K + 2) * 2^-24 * S + 2^-24)
(2^-4: half a unit of e4m3's 3-bit mantissa; 2^-10: half its subnormal spacing; the factor 2 covers a pre-rounding
value on a rounding boundary).  Derived, not tuned.  `mul` is drawn so that between 0.1 % and 5 % of the outputs
saturate (asserted on the reference).  The maxpool is exact, the cast and the broadcast are bitwise equal to
clamp().to(float8_e4m3fn) on the CPU, the average pool is held to
2 * ((HW + 1) * 2^-24 * mean|x| * scale + 2^-11 * |ref|)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
SENTINEL = 0x5A        # a byte pattern written before the call; it must survive outside the slice


def _r8(c):
    return (c + 7) // 8 * 8


def _r16(c):
    return (c + 15) // 16 * 16


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _q(t):
    """The one conversion rule: clamp in fp32, round to nearest even."""
    return t.float().clamp(-448.0, 448.0).to(F8)


def _draw8(shape, gen, scale=1.0):
    """e4m3-valued fp64 numbers."""
    return _q(torch.randn(shape, generator=gen) * scale).double()


def _nhwc8(x, pitch=None):
    """e4m3-valued [N,C,H,W] (CPU) -> NHWC e4m3 bytes with `pitch` channels (zeros in the padding)."""
    N, Cc, H, W = x.shape
    out = torch.zeros((N, H, W, pitch or _r16(Cc)), dtype=torch.uint8).view(F8)
    out[..., :Cc] = x.permute(0, 2, 3, 1).to(F8)
    return out


def _pack8(w):
    """e4m3-valued [Cout,Cin,k,k] -> [Cout8][kh][kw][Cin16] e4m3, zeros in the padding."""
    co, ci, kh, kw = w.shape
    out = torch.zeros((_r8(co), kh, kw, _r16(ci)), dtype=torch.uint8).view(F8)
    out[:co, :, :, :ci] = w.permute(0, 2, 3, 1).to(F8)
    return out


def _case(cuda, N, cin, cout, H, W, k, stride, pad, dil, relu=True, residual=False, y_pitch=None, y_off=0, f32=False,
          seed=0):
    from dcfp_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(2000 + seed)
    Kred = cin * k * k
    x = _draw8((N, cin, H, W), gen, 2.0)
    w = _draw8((cout, cin, k, k), gen, 1.0)
    acc = F.conv2d(x, w, None, stride, pad, dil)
    Sacc = F.conv2d(x.abs(), w.abs(), None, stride, pad, dil)
    Ho, Wo = acc.shape[2:]
    # mul: per channel, so that |acc * mul| passes 448 at about the 99th percentile of |acc| (f32 output: no clamp)
    level = float(torch.quantile(acc.abs().flatten()[:1 << 20], 0.99))
    mul = ((0.2 if f32 else 448.0) / level * (0.8 + 0.4 * torch.rand(cout, generator=gen))).float()
    add = (torch.randn(cout, generator=gen) * 8.0).float()
    bc = lambda v: v.double().view(1, -1, 1, 1)  # noqa: E731
    ref = acc * bc(mul) + bc(add)
    S = Sacc * bc(mul).abs() + bc(add).abs()
    res, res_mul = None, 0.375
    if residual:
        res = _draw8((N, cout, Ho, Wo), gen, 100.0)
        ref, S = ref + res_mul * res, S + (res_mul * res).abs()
    if relu and not f32:
        ref = F.relu(ref)
    cout8, cout16 = _r8(cout), _r16(cout)
    mu, ad = torch.zeros(cout8), torch.zeros(cout8)
    mu[:cout], ad[:cout] = mul, add
    y_pitch = y_pitch or cout16
    d = _lib.ConvF8Desc(N, H, W, _r16(cin), _r16(cin), cout, k, stride, pad, dil, Ho, Wo, 0 if f32 else y_pitch, y_off,
                        cout16 if residual else 0, 0, int(relu), res_mul if residual else 0.0)
    xd, wd, mud, add_ = _nhwc8(x).to(cuda), _pack8(w).to(cuda), mu.to(cuda), ad.to(cuda)
    if f32:
        y = torch.full((N, cout, Ho, Wo), float("nan"), device=cuda)
        st = L.dcfp_conv2d_fwd_f8_nhwc_to_f32_nchw(C.byref(d), _p(xd), _p(wd), _p(mud), _p(add_), _p(y), _stream())
        assert st == 0, st
        got = y.double().cpu()
        assert torch.isfinite(got).all()
        err = (got - ref).abs()
        bound = 2 * ((Kred + 2) * 2.0 ** -24 * S + 2.0 ** -24)
        worst = float((err / bound).max())
        sat = 0.0
    else:
        y = torch.full((N, Ho, Wo, y_pitch), SENTINEL, dtype=torch.uint8, device=cuda)
        rd = _nhwc8(res).to(cuda) if residual else None
        st = L.dcfp_conv2d_fwd_f8_nhwc(C.byref(d), _p(xd), _p(wd), _p(mud), _p(add_), _p(rd), _p(y), _stream())
        assert st == 0, st
        yc = y.cpu()
        got = yc[..., y_off:y_off + cout].contiguous().view(F8).permute(0, 3, 1, 2).double()
        assert torch.isfinite(got).all()
        # padded output channels hold exact zeros; everything outside the slice keeps its bytes
        assert (yc[..., y_off + cout:y_off + cout16] == 0).all()
        outside = torch.cat([yc[..., :y_off], yc[..., y_off + cout16:]], dim=-1)
        assert (outside == SENTINEL).all()
        sat = float((ref.abs() > 448.0).double().mean())
        assert 0.001 <= sat <= 0.05, sat                      # (a property of the case, checked on the reference)
        inside, over = ref.abs() <= 448.0, ref.abs() >= 480.0
        assert bool(over.any())
        assert torch.equal(got[over], 448.0 * ref[over].sign())
        err = (got - ref).abs()
        bound = 2 * ((Kred + 2) * 2.0 ** -24 * S + 2.0 ** -4 * ref.abs() + 2.0 ** -10)
        worst = float((err / bound)[inside].max())
    print(f"conv_f8 {cin}->{cout} k{k} s{stride} d{dil} {H}x{W}: max err {float(err.max()):.3e}, "
          f"worst err/bound {worst:.3f}, saturated {100 * sat:.2f} %")
    assert worst <= 1.0, worst


# the shapes of tests/test_conv_f16_gpu.py: the smallest that reach every tail of the kernel
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
def test_conv_f8_against_fp64(cuda, tag):
    _case(cuda, seed=list(CASES).index(tag), **CASES[tag])


def test_conv_f8_descriptor_checks_do_not_need_a_launch(cuda):
    from dcfp_amd import _lib
    L = _lib.lib()
    ok = dict(N=1, H=8, W=8, Cin16=16, x_pitch=16, Cout=16, K=1, stride=1, pad=0, dil=1, Hout=8, Wout=8, y_pitch=32,
              y_off=16, res_pitch=0, res_off=0, relu=0, res_mul=0.0)
    buf = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    vec = torch.zeros(16, device=cuda)

    def call(**kw):
        d = _lib.ConvF8Desc(**{**ok, **kw})
        return L.dcfp_conv2d_fwd_f8_nhwc(C.byref(d), _p(buf), _p(buf), _p(vec), _p(vec), None, _p(buf), _stream())
    assert call() == 0
    for bad in (dict(Cin16=8), dict(x_pitch=24), dict(y_off=8), dict(y_pitch=24), dict(y_off=32), dict(Hout=7)):
        assert call(**bad) == _lib.E_BADDESC, bad
    for bad in (dict(K=5, Hout=4, Wout=4), dict(stride=3)):
        assert call(**bad) == _lib.E_UNSUPPORTED, bad


@pytest.mark.parametrize("N,Cc,H,W,pitch", [(2, 32, 13, 17, 48), (1, 16, 6, 8, 32), (2, 64, 33, 33, 64)])
def test_maxpool_nhwc_f8_is_exact(cuda, N, Cc, H, W, pitch):
    from dcfp_amd import _lib
    x = _draw8((N, Cc, H, W), torch.Generator().manual_seed(7), 30.0)
    ref = F.max_pool2d(x, 3, 2, 1)
    Ho, Wo = ref.shape[2:]
    xd = _nhwc8(x, pitch).to(cuda)
    y = torch.full((N, Ho, Wo, pitch), SENTINEL, dtype=torch.uint8, device=cuda)
    st = _lib.lib().dcfp_maxpool3x3s2_nhwc_f8(_p(xd), _p(y), N, H, W, Cc, pitch, Ho, Wo, pitch, _stream())
    assert st == 0, st
    yc = y.cpu()
    want = ref.permute(0, 2, 3, 1).to(F8).contiguous().view(torch.uint8)
    assert torch.equal(yc[..., :Cc].contiguous(), want)
    assert (yc[..., Cc:] == SENTINEL).all()


def _cast_ref(x16, scale):
    return _q(x16.float() * torch.tensor(np.float32(scale))).view(torch.uint8)


@pytest.mark.parametrize("Cc,x_pitch,scale", [(47, 48, 3.0), (64, 72, 1.0), (3, 8, 0.0123)])
def test_cast_f16_to_f8_is_bitwise(cuda, Cc, x_pitch, scale):
    from dcfp_amd import _lib
    P, y_pitch, y_off = 2 * 9 * 13, 128, 32
    x = torch.zeros((P, x_pitch), dtype=torch.float16)
    x[:, :Cc] = (torch.randn((P, Cc), generator=torch.Generator().manual_seed(13)) * 100).to(torch.float16)
    x[0, :3] = torch.tensor([2.0 ** -9, 2.0 ** -10, 465.0][:min(3, Cc)], dtype=torch.float16)   # subnormal, tie, > 448
    x[1, :3] = torch.tensor([-500.0, 448.0, 0.0][:min(3, Cc)], dtype=torch.float16)
    x[:, Cc:] = 77.0                                     # garbage beyond C in the source must not reach the output
    y = torch.full((P, y_pitch), SENTINEL, dtype=torch.uint8, device=cuda)
    st = _lib.lib().dcfp_cast_nhwc_f16_to_f8(_p(x.to(cuda)), x_pitch, _p(y), y_pitch, y_off, P, Cc, scale, _stream())
    assert st == 0, st
    yc = y.cpu()
    c16 = _r16(Cc)
    assert torch.equal(yc[:, y_off:y_off + Cc].contiguous(), _cast_ref(x[:, :Cc], scale))
    assert (yc[:, y_off + Cc:y_off + c16] == 0).all()
    assert (torch.cat([yc[:, :y_off], yc[:, y_off + c16:]], dim=1) == SENTINEL).all()
    if scale == 1.0:
        assert yc[0, y_off:y_off + 3].view(F8).float().tolist() == [2.0 ** -9, 0.0, 448.0]


def test_broadcast_f16_to_f8_into_a_channel_slice_is_bitwise(cuda):
    from dcfp_amd import _lib
    N, Cc, H, W, pitch, off, vp, scale = 2, 152, 9, 13, 1280, 1024, 160, 0.61
    v = torch.full((N, vp), 77.0, dtype=torch.float16)
    v[:, :Cc] = (torch.randn((N, Cc), generator=torch.Generator().manual_seed(5)) * 400).to(torch.float16)
    y = torch.full((N, H, W, pitch), SENTINEL, dtype=torch.uint8, device=cuda)
    st = _lib.lib().dcfp_broadcast_nhwc_f16_to_f8(_p(v.to(cuda)), vp, _p(y), N, H * W, Cc, pitch, off, scale, _stream())
    assert st == 0, st
    yc = y.cpu()
    want = _cast_ref(v[:, :Cc], scale).view(N, 1, 1, Cc).expand(N, H, W, Cc)
    assert torch.equal(yc[..., off:off + Cc], want)
    assert (yc[..., off + Cc:off + _r16(Cc)] == 0).all()
    assert (torch.cat([yc[..., :off], yc[..., off + _r16(Cc):]], dim=-1) == SENTINEL).all()


@pytest.mark.parametrize("N,Cc,H,W", [(2, 272, 9, 13), (2, 272, 70, 70)])
def test_avgpool_f8_to_f16_against_fp64(cuda, N, Cc, H, W):
    """fp32 sums in a fixed order, times the scale, one rounding.  70 x 70 takes the split (several partial sums per
    image) path, 9 x 13 the single one."""
    from dcfp_amd import _lib
    L = _lib.lib()
    x = _q(torch.randn((N, Cc, H, W), generator=torch.Generator().manual_seed(11)) * 50 + 10).double()
    HW, scale = H * W, float(np.float32(0.173))
    ref = x.mean(dim=(2, 3)) * scale
    bound = 2 * ((HW + 1) * 2.0 ** -24 * x.abs().mean(dim=(2, 3)) * scale + 2.0 ** -11 * ref.abs())
    nbytes = int(L.dcfp_avgpool_nhwc_f16_workspace_bytes(N, Cc, HW))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    y = torch.full((N, Cc + 8), 0x7B5A, dtype=torch.int16, device=cuda).view(torch.float16)
    st = L.dcfp_avgpool_nhwc_f8_to_f16(_p(_nhwc8(x).to(cuda)), _p(y), N, HW, Cc, Cc, Cc + 8, scale, _p(ws), nbytes,
                                       _stream())
    assert st == 0, st
    yc = y.cpu()
    assert (yc[:, Cc:].view(torch.int16) == 0x7B5A).all()
    err = (yc[:, :Cc].double() - ref).abs()
    worst = float((err / bound).max())
    print(f"avgpool_f8 {Cc} x {H}x{W}: max err {float(err.max()):.3e}, worst err/bound {worst:.3f}")
    assert worst <= 1.0, worst
    assert L.dcfp_avgpool_nhwc_f8_to_f16(_p(_nhwc8(x).to(cuda)), _p(y), N, HW, Cc, Cc, Cc + 8, scale, _p(ws),
                                         nbytes - 1, _stream()) == _lib.E_WORKSPACE
