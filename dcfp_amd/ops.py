"""Tensor-level wrappers and autograd Functions over the C-ABI (include/dcfp_hip.h).

PyTorch supplies device memory, streams and autograd bookkeeping; every FLOP and byte
moved on the hot path below happens in libdcfp_hip.so.  Inputs must be CUDA (HIP) fp32
tensors — there is deliberately no CPU / eager fallback.
"""
import ctypes as C
import os
import weakref

import torch
import torch.distributed as dist

from . import _lib, arena, syncbn_p2p
from ._lib import ConvDesc, BnRunning, check

_ws_cache = {}
# Bumped whenever parameters are rewritten through raw pointers (FusedSGD.step, load_state_dict):
# caches derived from weights (folded eval-mode BN, permuted conv weights) key on it because
# torch's per-tensor `_version` does not see those writes.
WEIGHT_EPOCH = [0]

# ---- optional per-launch timing (bench.py's roofline leg): when a list is installed, every
# conv / BN C-ABI call is bracketed by events on the stream it is launched on.
_PROFILE = None


def profile_start():
    global _PROFILE
    _PROFILE = []


def profile_stop():
    """Returns [(kind, key, algorithmic_work, milliseconds)] and disables timing."""
    global _PROFILE
    recs, _PROFILE = _PROFILE, None
    torch.cuda.synchronize()
    return [(k, key, work, s.elapsed_time(e)) for (k, key, work, s, e) in (recs or [])]


def _timed(kind, key, work, fn):
    if _PROFILE is None:
        return fn()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    r = fn()
    e.record()
    _PROFILE.append((kind, key, work, s, e))
    return r


def conv_kernel_name(d, which):
    buf = C.create_string_buffer(64)
    n = _lib.lib().dcfp_conv2d_kernel_name(C.byref(d), which, buf, 64)
    return buf.value.decode() if n > 0 else "?"


def conv_executed_fraction(d, which):
    """Share of the nominal multiply-adds the dispatched kernel issues (< 1 where dead kernel rows are skipped)."""
    return float(_lib.lib().dcfp_conv2d_executed_fraction(C.byref(d), which))


def _conv_flops(d):
    return 2.0 * d.N * d.Cout * d.Hout * d.Wout * d.Cin * d.KH * d.KW


def _require(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"dcfp_amd: {name} must be a CUDA/HIP tensor (no CPU fallback exists)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"dcfp_amd: {name} must be float32, got {t.dtype}")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _workspace(tag, nbytes, device):
    """Grow-only scratch per (tag, device); reuse is safe because launches are stream-ordered."""
    key = (tag, device.index, torch.cuda.current_stream().cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _batch_strided(t):
    """Return (tensor, batch_stride) for a [N,C,H,W] tensor whose images are dense
    (a channel slice of a wider tensor qualifies); otherwise a contiguous copy."""
    N, Cc, H, W = t.shape
    st = t.stride()
    if st[3] == 1 and st[2] == W and st[1] == H * W and (N == 1 or st[0] >= Cc * H * W):
        return t, (st[0] if N > 1 else Cc * H * W)
    t = t.contiguous()
    return t, Cc * H * W


def _on_grid(t, nstride):
    """True where the 16-byte paths may touch `t`: it starts on the 16-byte grid and its images are whole quads apart.
    An LDS-DMA conv route needs that of its source, a vector epilogue of its output (include/dcfp_hip.h); a call with an
    operand off the grid runs other kernels, with another layout of the permuted weight copy."""
    return t.data_ptr() % 16 == 0 and nstride % 4 == 0


def _grid_variant(src_ok, out_ok, src_dense=0, out_dense=0, out_px=0):
    """Suffix of the kept-copy key of a conv call (_wp_buffer's variant): calls whose operands sit off the 16-byte grid
    keep a copy of their own, since the kernel they fall back to reads another layout.  src_dense / out_dense / out_px:
    the dense image strides and the output pixels per channel - where those are no whole quads the call with aligned
    operands has no 16-byte path either, and an operand off the grid changes nothing."""
    src_ok = src_ok or src_dense % 4 != 0
    out_ok = out_ok or out_dense % 4 != 0 or out_px % 4 != 0
    return "" if (src_ok and out_ok) else f"@{int(src_ok)}{int(out_ok)}"


def _pitch_of(t):
    """Row pitch of a [N,C,H,W] tensor whose rows are dense but stride(2) > W (a [..., :W] view of a buffer with
    padded rows, channels H*pitch and images C*H*pitch apart); 0 for anything else (dense included)."""
    N, Cc, H, W = t.shape
    st = t.stride()
    if st[3] == 1 and st[2] > W and st[2] % 4 == 0 and st[1] == H * st[2] and (N == 1 or st[0] == Cc * H * st[2]):
        return st[2]
    return 0


_PITCH_BUFFERS = {}


def pitched_buffer(shape, pitch, key, device):
    """[N,C,H,W] view (rows `pitch` floats apart) of a persistent zero-initialised buffer: the kernels write the
    W live floats of a row only, so the tail stays zero for as long as the buffer lives (no per-step fill)."""
    k = (key, tuple(shape), pitch, str(device))
    buf = _PITCH_BUFFERS.get(k)
    if buf is None:
        buf = new_pitched(shape, pitch, device)
        _PITCH_BUFFERS[k] = buf
    return buf


class PitchLease:
    """Held by the autograd node that reads a module's persistent pitched buffer in its backward.  The buffer is busy
    while a lease on it is alive: `release()` (end of that backward) or the death of the node - a grad-enabled forward
    whose graph is dropped without backward, an exception between forward and backward - frees it for the next forward."""
    __slots__ = ("slot", "__weakref__")

    def __init__(self, slot):
        self.slot = slot
        slot["lease"] = weakref.ref(self)

    def release(self):
        if self.slot.get("lease") is not None and self.slot["lease"]() is self:
            self.slot["lease"] = None


def _pitch_busy(slot):
    ref = slot.get("lease")
    return ref is not None and ref() is not None


def owner_pitched(owner, shape, pitch, device, track=True):
    """The persistent row-pitched buffer of a module's output (it lives from the forward to the backward of the
    conv that reads it): (view, lease).  While a graph holds a lease on the buffer, a second forward gets a fresh
    buffer instead (lease None)."""
    slot = getattr(owner, "_dcfp_pitch", None) if owner is not None else None
    if slot is not None and not _pitch_busy(slot) and tuple(slot["y"].shape) == tuple(shape) \
            and _pitch_of(slot["y"]) == pitch and slot["y"].device == device:
        view = slot["y"]
    else:
        view = new_pitched(shape, pitch, device)
        if owner is not None and (slot is None or not _pitch_busy(slot)):
            slot = {"y": view, "lease": None}
            owner._dcfp_pitch = slot
        else:
            slot = None
    return view, (PitchLease(slot) if (slot is not None and track) else None)


def new_pitched(shape, pitch, device):
    """Fresh zeroed row-pitched [N,C,H,W] view.  The allocation starts with a margin of zeros (the contract of
    DcfpConvDesc.x_pitch: the pitch - W floats in front of the first element are readable zeros)."""
    N, Cc, H, W = shape
    lead = 64                                            # floats; keeps the view 256-byte aligned
    flat = torch.zeros(lead + N * Cc * H * pitch, dtype=torch.float32, device=device)
    return flat[lead:].view(N, Cc, H, pitch)[..., :W]


# The 3x3 convs whose taps shift columns by a non-multiple of 4 (dilation 1 / 2) read their shifted operand from a
# row-pitched tensor with a zero tail instead of handling image borders with 4-byte copies (include/dcfp_hip.h
# DcfpConvDesc.x_pitch).  DCFP_PITCHED=0: dense operands everywhere.
PITCHED = os.environ.get("DCFP_PITCHED", "1") not in ("0",)


def conv_pitch(xshape, wshape, stride, pad, dil):
    """Row pitch to use for the x / dy operands of this conv (0: keep them dense)."""
    if not PITCHED or wshape[2] != 3 or stride != 1 or pad != dil or ((pad | dil) & 3) == 0:
        return 0
    W = xshape[3]
    pitch = W + (pad + 3) // 4 * 4
    d = _desc(xshape, wshape, stride, pad, dil, pitch, pitch)
    return pitch if _lib.lib().dcfp_conv2d_pitch_supported(C.byref(d)) else 0


def conv_out_size(size, k, stride, pad, dil):
    return (size + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _desc(xshape, wshape, stride, pad, dil, x_pitch=0, dy_pitch=0):
    N, Cin, H, W = xshape
    Cout, Cin2, KH, KW = wshape
    if Cin2 != Cin:
        raise RuntimeError(f"conv2d: weight expects {Cin2} input channels, got {Cin} (groups unsupported)")
    d = ConvDesc(N, Cin, H, W, Cout, KH, KW, stride, pad, dil,
                 conv_out_size(H, KH, stride, pad, dil), conv_out_size(W, KW, stride, pad, dil),
                 x_pitch, dy_pitch)
    return d


# ------------------------------------------------------------------ conv2d
# The Bottleneck convs emit the batch statistics of their output for the BatchNorm behind them (no
# 4 B/element stats pass): BN -6 ms/step, conv epilogues +1 ms/step since the LDS-DMA kernels merge the
# per-lane partials through LDS instead of 640 swizzles per wave and tile.  DCFP_FUSED_BN_STATS=0: off.
FUSE_BN_STATS = os.environ.get("DCFP_FUSED_BN_STATS", "1") not in ("0",)
# The residual BatchNorm of a Bottleneck keeps its ReLU mask as one bit per element for the backward
# (instead of two re-reads of the 4-byte block output); DCFP_BN_RELU_BITMASK=0 switches it off.
BN_RELU_BITMASK = os.environ.get("DCFP_BN_RELU_BITMASK", "1") not in ("0",)
# =0: the SyncBN backward exchange of the two per-channel sums is waited for before anything else is enqueued (A/B)
SYNCBN_ASYNC = os.environ.get("DCFP_SYNCBN_ASYNC", "1") not in ("0",)


_WP_OWNERS = weakref.WeakSet()     # weight tensors that carry permuted copies (w._dcfp_wp)
_WP_TABLE = {"version": 0, "built": -1, "dev": None, "n": 0, "blocks": 0, "entries": []}


def _wp_buffer(w, which, d, nbytes, variant=""):
    """Persistent buffer for the permuted weight copy Wp of (weight tensor, pass, shape) and whether the
    library may skip rebuilding it (`wp_valid` of include/dcfp_hip.h).  Validity = same storage, same torch
    version counter and same WEIGHT_EPOCH (raw-pointer writes by FusedSGD).  In training every weight changes
    once per step: FusedSGD.step() then calls refresh_wp(), ONE multi-tensor launch that rebuilds every
    registered copy (forward and dgrad layouts of all convs) and re-validates them, instead of a permute
    launch inside each of the 233 conv calls of a step."""
    # (the copy's layout depends on the kernel the shape routes to, which depends on the operand pitches and,
    # for the inference call with its fused epilogue, on the variant: separate entries)
    key = (which, d.N, d.H, d.W, d.stride, d.pad, d.dil, d.x_pitch, d.dy_pitch, variant)
    tag = (w.data_ptr(), w._version, WEIGHT_EPOCH[0], torch.cuda.current_stream().cuda_stream)
    cache = getattr(w, "_dcfp_wp", None)
    if cache is None:
        cache = {}
        try:
            w._dcfp_wp = cache
            _WP_OWNERS.add(w)
        except Exception:        # not an attribute-bearing tensor: no caching
            return _workspace("conv", nbytes, w.device), 0
    ent = cache.get(key)
    if ent is not None and ent[1].numel() >= nbytes:
        if ent[0] == tag:
            return ent[1], 1
        cache[key] = (tag, ent[1], ent[2])
        return ent[1], 0
    if len(cache) > 8:           # shapes keep changing (multi-scale evaluation): do not hoard buffers
        cache.clear()
    buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=w.device)
    cache[key] = (tag, buf, ConvDesc(*[getattr(d, f[0]) for f in ConvDesc._fields_]))
    _WP_TABLE["version"] += 1
    return buf, 0


def _conv_workspace(w, which, d, variant=""):
    """(workspace, wp_valid) of a forward / dgrad call: the conv's own persistent buffer (the permuted weight copy of a
    direct kernel, or the transformed filters of a fused Winograd conv), or - where the library says the workspace is
    pure scratch (three-pass Winograd: transformed operands, hundreds of MB) - one buffer shared by all.  variant: a
    call that does not run what dcfp_conv2d_wp_layout describes for (d, which) keeps a copy of its own, rebuilt on demand."""
    L = _lib.lib()
    nbytes = L.dcfp_conv2d_workspace_bytes(C.byref(d), which)
    if L.dcfp_conv2d_workspace_is_scratch(C.byref(d), which):
        return _workspace("conv_scratch", nbytes, w.device), 0
    return _wp_buffer(w, which, d, nbytes, variant)


def refresh_wp():
    """After an in-place weight update: rebuild every registered Wp copy with one launch and mark them valid
    for the current WEIGHT_EPOCH.  The device table of (weights, copy, layout) records is rebuilt only when
    the set of registered copies changed (first steps of a run)."""
    T = _WP_TABLE
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    if T["built"] != T["version"]:
        ents, recs, first = [], [], 0
        for w in list(_WP_OWNERS):
            if not w.is_cuda or not w.is_contiguous():
                continue
            for key, (tag, buf, desc) in list(w._dcfp_wp.items()):
                if key[-1]:          # inference-variant copies rebuild on demand (their layout is the call's own)
                    continue
                e = _lib.WpEntry()
                if L.dcfp_conv2d_wp_layout(C.byref(desc), key[0], C.byref(e)) != 0:
                    continue
                e.w, e.wp, e.first_block = w.data_ptr(), buf.data_ptr(), first
                first += e.n_blocks
                recs.append(e); ents.append((weakref.ref(w), key))
        T["entries"], T["n"], T["blocks"] = ents, len(recs), first
        if recs:
            arr = (_lib.WpEntry * len(recs))(*recs)
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            T["dev"] = host.to(torch.device("cuda", torch.cuda.current_device()))
        T["built"] = T["version"]
        T["ptrs"] = [e.w for e in recs]
    if not T["n"]:
        return
    live = []
    for (wr, key), ptr in zip(T["entries"], T["ptrs"]):
        w = wr()
        if w is None or w.data_ptr() != ptr or key not in w._dcfp_wp:     # a weight went away / moved: rebuild next time
            T["version"] += 1
            return
        live.append((w, key))
    check(L.dcfp_conv2d_permute_weights_multi_f32(C.c_void_p(T["dev"].data_ptr()), T["n"], T["blocks"],
                                                  C.c_void_p(stream)), "permute_weights_multi")
    for w, key in live:
        _, buf, desc = w._dcfp_wp[key]
        w._dcfp_wp[key] = ((w.data_ptr(), w._version, WEIGHT_EPOCH[0], stream), buf, desc)


def _bn_run(running_mean, running_var, momentum, nbt):
    """DcfpBnRunning for the statistics kernels (None: nothing to update)."""
    upd = running_mean is not None and momentum is not None
    if not upd and nbt is None:
        return None
    r = BnRunning()
    r.running_mean = running_mean.data_ptr() if upd else None
    r.running_var = running_var.data_ptr() if upd else None
    r.num_batches_tracked = nbt.data_ptr() if nbt is not None else None
    r.momentum = float(momentum) if upd else 0.0
    return r


def _rp(run):
    return C.byref(run) if run is not None else None


FANIN_RED_USED = [0]     # BatchNorm backwards that took their sums from a fan-in epilogue (tests / bench)
FANIN_BN_SUMS = os.environ.get("DCFP_FANIN_BN_SUMS", "1") not in ("0",)   # =0: every BatchNorm backward runs its own reduce kernel (A/B)
# =2: the fan-in epilogue reduces bn3's gradient even where the fused BatchNorm backward applies (round-3 behaviour).  By
# default (1) it does so only under SyncBN: the fused backward reads dy and x once anyway (12 B/element, what the
# apply-only pass behind the epilogue sums costs), so the epilogue's extra reads would buy nothing there
FANIN_BN_SUMS_ALWAYS = os.environ.get("DCFP_FANIN_BN_SUMS", "1") == "2"
KEEP_XFORM = os.environ.get("DCFP_KEEP_XFORM", "1") not in ("0",)   # =0: weight gradients transform x again (A/B)


def conv2d_fwd(x, w, bias=None, stride=1, pad=0, dil=1, want_stats=False, bn_run=None, out=None, keep=None):
    """y = conv2d(x, w).  With want_stats the result is (y, stats): stats = (mean, biased var) of y
    per output channel over (N, H, W) - what the BatchNorm that follows needs - taken from partials
    the conv epilogue emits, or None where the library has no fused statistics for the shape; bn_run
    (a BnRunning) lets the kernel that finalises them also update that BatchNorm's running statistics.
    out: optional [N, Cout, Ho, Wo] destination, may be a channel slice of a wider tensor (ASPP concat)."""
    _require(x, "x"); _require(w, "weight")
    xp = _pitch_of(x)
    if not xp:
        x = x.contiguous()
    w = w if w.is_contiguous() else w.contiguous()
    d = _desc(x.shape, w.shape, stride, pad, dil, xp, 0)
    yns = 0
    if out is None:
        y = torch.empty((d.N, d.Cout, d.Hout, d.Wout), dtype=torch.float32, device=x.device)
    else:
        y = out
        st = y.stride()
        if tuple(y.shape) != (d.N, d.Cout, d.Hout, d.Wout) or st[3] != 1 or st[2] != d.Wout or st[1] != d.Hout * d.Wout:
            raise RuntimeError("conv2d_fwd: out must be [N,Cout,Ho,Wo] with dense images (a channel slice is fine)")
        yns = st[0]
    if bias is not None:
        _require(bias, "bias"); bias = bias.contiguous()
    L = _lib.lib()
    x_ok = _on_grid(x, d.Cin * d.H * (xp or d.W))
    y_ok = _on_grid(y, yns or d.Cout * d.Hout * d.Wout)
    if xp and not (x_ok and y_ok):
        # only the LDS-DMA kernels read row-pitched sources, and those need both operands on the 16-byte grid
        x = x.contiguous()
        xp, d = 0, _desc(x.shape, w.shape, stride, pad, dil, 0, 0)
        x_ok = _on_grid(x, d.Cin * d.H * d.W)
    # (a 3x3 conv WITH bias never runs as Winograd: where the same descriptor without bias does, the kept buffer holds
    #  transformed filters, not the direct kernel's permuted copy - the biased call gets a copy of its own)
    wino = d.KH == 3 and conv_kernel_name(d, _lib.CONV_FWD).startswith("winograd")
    variant = ("bias" if (bias is not None and wino) else "") + \
        _grid_variant(x_ok, y_ok, d.Cin * d.H * (xp or d.W), d.Cout * d.Hout * d.Wout, d.Hout * d.Wout)
    ws, valid = _conv_workspace(w, _lib.CONV_FWD, d, variant)
    if wino and not x_ok:
        # (a Winograd conv whose x is off the grid runs a direct kernel: no transformed input to keep, no statistics laid
        #  out by Winograd tiles - the weight gradient transforms x itself, the BatchNorm runs its own statistics kernel)
        keep, want_stats, no_stats = None, False, want_stats
    else:
        no_stats = False
    if keep is not None and KEEP_XFORM and bias is None:
        # Winograd conv whose weight gradient is Winograd too: leave the transformed input in a buffer that `keep`
        # (a dict living in the autograd context) holds until the backward pass (conv2d_wgrad(..., xform=))
        xb = L.dcfp_conv2d_xform_bytes(C.byref(d))
        if xb > 0:
            xf = torch.empty(xb, dtype=torch.uint8, device=x.device)
            slots = L.dcfp_conv2d_fwd_stat_slots(C.byref(d), _p(y), yns) if want_stats else 0
            part = _workspace("bn_stat_partials", slots * d.Cout * 2 * 4, x.device) if slots > 0 else None
            _timed("conv_fwd", d, _conv_flops(d), lambda: check(
                L.dcfp_conv2d_fwd_keep_f32_nchw(C.byref(d), _p(x), _p(w), _p(y), yns, _p(xf), xb, _p(part), _p(ws),
                                                ws.numel(), _stream()), "conv2d_fwd_keep"))
            keep["xform"] = xf
            if part is not None:
                mv = torch.empty((2, d.Cout), dtype=torch.float32, device=x.device)
                check(L.dcfp_bn_stats_from_partials_f32(_p(part), slots, 128, d.Cout, _p(mv[0]), _p(mv[1]),
                                                        _rp(bn_run), _stream()), "bn_stats_from_partials")
                return y, (mv[0], mv[1], bn_run is not None)
            return (y, None) if want_stats else y
    if want_stats and bias is None:
        slots = L.dcfp_conv2d_fwd_stat_slots(C.byref(d), _p(y), yns)
        if slots > 0:
            part = _workspace("bn_stat_partials", slots * d.Cout * 2 * 4, x.device)
            _timed("conv_fwd", d, _conv_flops(d), lambda: check(
                L.dcfp_conv2d_fwd_stats_f32_nchw(C.byref(d), _p(x), _p(w), _p(y), yns, _p(part), _p(ws),
                                                 ws.numel(), valid, _stream()), "conv2d_fwd_stats"))
            mv = torch.empty((2, d.Cout), dtype=torch.float32, device=x.device)
            check(L.dcfp_bn_stats_from_partials_f32(_p(part), slots, 128, d.Cout, _p(mv[0]), _p(mv[1]),
                                                    _rp(bn_run), _stream()), "bn_stats_from_partials")
            return y, (mv[0], mv[1], bn_run is not None)
    _timed("conv_fwd", d, _conv_flops(d), lambda: check(
        L.dcfp_conv2d_fwd_f32_nchw(C.byref(d), _p(x), _p(w), _p(bias), _p(y), yns, _p(ws), ws.numel(), valid,
                                   _stream()), "conv2d_fwd"))
    return (y, None) if (want_stats or no_stats) else y


def conv2d_dgrad(dy, w, xshape, stride, pad, dil, out=None, accumulate=False):
    """dx = conv_transpose(dy, w); with accumulate, `out` (+)= the result in place."""
    _require(dy, "dy")
    w = w if w.is_contiguous() else w.contiguous()
    dp = _pitch_of(dy)
    d = _desc(xshape, w.shape, stride, pad, dil, 0, dp)
    if out is not None:
        if tuple(out.shape) != tuple(xshape) or not out.is_contiguous():
            raise RuntimeError("conv2d_dgrad: out must be a contiguous tensor of the input shape")
        dx = out
    else:
        dx = torch.empty(xshape, dtype=torch.float32, device=dy.device)
        accumulate = False
    dx_ok = _on_grid(dx, d.Cin * d.H * d.W)
    if dp and not (dx_ok and _on_grid(dy, dy.stride(0))):
        dy, dp = dy.contiguous(), 0         # (as in conv2d_fwd: pitched sources are read by the LDS-DMA kernels only)
        d = _desc(xshape, w.shape, stride, pad, dil, 0, 0)
    if dp:
        ns = dy.stride(0)
    else:
        dy, ns = _batch_strided(dy)
    L = _lib.lib()
    ws, valid = _conv_workspace(w, _lib.CONV_DGRAD, d, _grid_variant(
        _on_grid(dy, ns), dx_ok, d.Cout * d.Hout * (dp or d.Wout), d.Cin * d.H * d.W, d.H * d.W))
    _timed("conv_dgrad", d, _conv_flops(d), lambda: check(
        L.dcfp_conv2d_dgrad_f32_nchw(C.byref(d), _p(dy), ns, _p(w), _p(dx), int(bool(accumulate)),
                                     _p(ws), ws.numel(), valid, _stream()), "conv2d_dgrad"))
    return dx


MASKED_FANIN = os.environ.get("DCFP_MASKED_FANIN", "1") not in ("0",)   # =0: the residual gradient is written and re-read (A/B)


def conv2d_dgrad_fanin_ok(dyshape, w, xshape):
    """True where conv2d_dgrad_fanin is available for this 1x1 stride-1 conv."""
    d = _desc(xshape, w.shape, 1, 0, 1)
    return MASKED_FANIN and bool(_lib.lib().dcfp_conv2d_dgrad_fanin_supported(C.byref(d)))


def conv2d_dgrad_fanin(dy, w, xshape, fan_src, fan_mask):
    """dx = dgrad(dy, w) + fan_src * mask (1-bit ReLU mask of bn_apply_relu_mask): the gradient fan-in of a residual
    block without the residual branch's gradient ever being written."""
    _require(dy, "dy"); _require(fan_src, "fan_src")
    w = w if w.is_contiguous() else w.contiguous()
    d = _desc(xshape, w.shape, 1, 0, 1)
    dy, ns = _batch_strided(dy)
    if tuple(fan_src.shape) != tuple(xshape) or not fan_src.is_contiguous():
        raise RuntimeError("conv2d_dgrad_fanin: fan_src must be a contiguous tensor of the input shape")
    # the fan-in epilogue exists on the persistent LDS-DMA kernel only, which the library refuses for operands off the
    # 16-byte grid (nothing in the package produces one here): they are copied onto it
    if not _on_grid(dy, ns):
        dy = dy.clone(memory_format=torch.contiguous_format)
        ns = dy.stride(0)
    if not _on_grid(fan_src, 4):
        fan_src = fan_src.clone()
    dx = torch.empty(xshape, dtype=torch.float32, device=dy.device)
    ws, valid = _conv_workspace(w, _lib.CONV_DGRAD, d)
    _timed("conv_dgrad", d, _conv_flops(d), lambda: check(
        _lib.lib().dcfp_conv2d_dgrad_fanin_f32_nchw(C.byref(d), _p(dy), ns, _p(w), _p(dx), _p(fan_src), _p(fan_mask),
                                                    _p(ws), ws.numel(), valid, _stream()), "conv2d_dgrad_fanin"))
    return dx


def conv2d_dgrad_fanin_red_slots(w, xshape):
    """Slot count of the fan-in form that also emits the previous block's BatchNorm-backward sums (0: not available)."""
    if not (MASKED_FANIN and FANIN_BN_SUMS):
        return 0
    d = _desc(xshape, w.shape, 1, 0, 1)
    return int(_lib.lib().dcfp_conv2d_dgrad_fanin_red_slots(C.byref(d)))


def conv2d_dgrad_fanin_red(dy, w, xshape, fan_src, fan_mask, red_x, red_mask, red_mean, slots):
    """conv2d_dgrad_fanin whose result dx is ALSO reduced, in the epilogue, to the BatchNorm-backward partial sums of the
    residual block that produced this block's input: part[slot][C][2] = (sum g, sum g*(red_x - red_mean)), g = dx * the
    bit of red_mask.  Returns (dx, part); bn_bwd_sums_from_partials finishes them."""
    _require(dy, "dy"); _require(fan_src, "fan_src"); _require(red_x, "red_x")
    w = w if w.is_contiguous() else w.contiguous()
    d = _desc(xshape, w.shape, 1, 0, 1)
    dy, ns = _batch_strided(dy)
    if tuple(fan_src.shape) != tuple(xshape) or not fan_src.is_contiguous():
        raise RuntimeError("conv2d_dgrad_fanin_red: fan_src must be a contiguous tensor of the input shape")
    if tuple(red_x.shape) != tuple(xshape) or not red_x.is_contiguous() or red_mean.numel() != xshape[1]:
        raise RuntimeError("conv2d_dgrad_fanin_red: red_x / red_mean must match the input shape")
    dx = torch.empty(xshape, dtype=torch.float32, device=dy.device)
    part = torch.empty((slots, xshape[1], 2), dtype=torch.float32, device=dy.device)
    ws, valid = _conv_workspace(w, _lib.CONV_DGRAD, d)
    # (its own profile kind: the launch also does the previous block's BatchNorm reduction - bench.py lists it apart)
    _timed("conv_dgrad_red", d, _conv_flops(d), lambda: check(
        _lib.lib().dcfp_conv2d_dgrad_fanin_red_f32_nchw(C.byref(d), _p(dy), ns, _p(w), _p(dx), _p(fan_src), _p(fan_mask),
                                                        _p(red_x), _p(red_mask), _p(red_mean), _p(part), _p(ws),
                                                        ws.numel(), valid, _stream()), "conv2d_dgrad_fanin_red"))
    return dx, part


def bn_bwd_sums_from_partials(part, var, eps, dgamma=None, dbeta=None):
    """(sum_dy, sum_dy_xmu, dgamma) as bn_bwd_reduce returns them, from the partial sums of conv2d_dgrad_fanin_red."""
    slots, Cc, _ = part.shape
    s = torch.empty((2, Cc), dtype=torch.float32, device=part.device)
    if dgamma is None:
        dgamma = torch.empty(Cc, dtype=torch.float32, device=part.device)
    _timed("bn_bwd_reduce", None, 8.0 * part.numel() / 2, lambda: check(
        _lib.lib().dcfp_bn_bwd_sums_from_partials_f32(_p(part), slots, Cc, _p(var), float(eps), _p(s[0]), _p(s[1]),
                                                      _p(dgamma), _p(dbeta), _stream()), "bn_bwd_sums_from_partials"))
    return s[0], s[1], dgamma


def conv2d_wgrad(dy, x, wshape, stride, pad, dil, need_bias=False, dw=None, db=None, xform=None):
    """(dw, db); dw / db: optional destinations (the gradient arena's views).  xform: the transformed input the
    forward call left behind (conv2d_fwd(..., keep=)), taken instead of x where the library says so."""
    _require(dy, "dy"); _require(x, "x")
    xp, dp = _pitch_of(x), _pitch_of(dy)
    if not xp:
        x = x.contiguous()
    d = _desc(x.shape, wshape, stride, pad, dil, xp, dp)
    if dp:
        ns = dy.stride(0)
    else:
        dy, ns = _batch_strided(dy)
    L = _lib.lib()
    nbytes = L.dcfp_conv2d_workspace_bytes(C.byref(d), _lib.CONV_WGRAD)
    ws = _workspace("conv_scratch", nbytes, x.device)     # (shared with the forward / dgrad scratch: same stream)
    if dw is None:
        dw = torch.empty(wshape, dtype=torch.float32, device=x.device)
    elif tuple(dw.shape) != tuple(wshape) or not dw.is_contiguous():
        raise RuntimeError("conv2d_wgrad: dw must be a contiguous tensor of the weight shape")
    if need_bias and db is None:
        db = torch.empty((wshape[0],), dtype=torch.float32, device=x.device)
    if xform is not None and not need_bias and L.dcfp_conv2d_xform_bytes(C.byref(d)) == xform.numel():
        _timed("conv_wgrad", d, _conv_flops(d), lambda: check(
            L.dcfp_conv2d_wgrad_kept_f32_nchw(C.byref(d), _p(dy), ns, _p(xform), xform.numel(), _p(dw), _p(ws), ws.numel(),
                                              _stream()), "conv2d_wgrad_kept"))
        return dw, None
    _timed("conv_wgrad", d, _conv_flops(d), lambda: check(
        L.dcfp_conv2d_wgrad_f32_nchw(C.byref(d), _p(dy), ns, _p(x), _p(dw), _p(db) if need_bias else None, _p(ws),
                                     ws.numel(), _stream()), "conv2d_wgrad"))
    return dw, (db if need_bias else None)


def add_into(dst, src):
    """dst += src through the library (gradient accumulation onto an attached arena view)."""
    check(_lib.lib().dcfp_add_f32(_p(dst), _p(src), _p(dst), dst.numel(), _stream()), "add")


def wgrad_into_param(dy, x, w, bias, stride, pad, dil, keep=None):
    """Weight (and bias) gradient of a conv written where the parameter's gradient lives: returns
    (dw, db) as the autograd Function should return them (None = already accumulated in .grad).
    keep: the dict the forward call filled (conv2d_fwd(..., keep=)); its buffer is released here."""
    tw, kw = arena.grad_target(w)
    tb, kb = arena.grad_target(bias) if bias is not None else (None, 0)
    xform = keep.pop("xform", None) if keep else None
    conv2d_wgrad(dy, x, tuple(w.shape), stride, pad, dil, need_bias=bias is not None, dw=tw, db=tb, xform=xform)
    dw = arena.grad_commit(w, tw, kw, add_into)
    db = arena.grad_commit(bias, tb, kb, add_into) if bias is not None else None
    return dw, db


class Conv2dFn(torch.autograd.Function):
    """nn.Conv2d forward/backward (reference: every conv in networks/backbone/resnet.py,
    networks/tools/aspp.py, networks/deeplabv3.py)."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, dil):
        ctx.keep = {} if ctx.needs_input_grad[1] else None     # (a backward pass will ask for the weight gradient)
        y = conv2d_fwd(x, w, bias, stride, pad, dil, keep=ctx.keep)
        ctx.save_for_backward(x)
        ctx.params = (w, bias)           # the Parameter objects: their gradient slots are looked up on them
        ctx.cfg = (stride, pad, dil)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        w, bias = ctx.params
        stride, pad, dil = ctx.cfg
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = conv2d_dgrad(dy, w, tuple(x.shape), stride, pad, dil)
        if ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2]):
            dw, db = wgrad_into_param(dy, x, w, bias, stride, pad, dil, keep=ctx.keep)
        return dx, dw, db, None, None, None


def conv2d(x, w, bias=None, stride=1, pad=0, dil=1):
    return Conv2dFn.apply(x, w, bias, stride, pad, dil)


# ------------------------------------------------------------- batch norm
def bn_stats(x, run=None):
    _require(x, "x")
    N, Cc, H, W = x.shape
    x, ns = _batch_strided(x)
    L = _lib.lib()
    ws = _workspace("bn", L.dcfp_bn_workspace_bytes(N, Cc, H * W), x.device)
    mean = torch.empty(Cc, dtype=torch.float32, device=x.device)
    var = torch.empty(Cc, dtype=torch.float32, device=x.device)
    _timed("bn_stats", None, 4.0 * x.numel(), lambda: check(
        L.dcfp_bn_stats_f32(_p(x), ns, N, Cc, H * W, _p(mean), _p(var), _rp(run), _p(ws), ws.numel(), _stream()),
        "bn_stats"))
    return mean, var


def bn_apply(x, mean, var, gamma, beta, eps, residual=None, relu=False, out=None):
    N, Cc, H, W = x.shape
    x = x.contiguous()
    if residual is not None:
        residual = residual.contiguous()
    yns, ypitch = 0, 0
    if out is None:
        y = torch.empty_like(x)
    else:           # a channel slice of the ASPP concat tensor (aspp.py:77), or a row-pitched buffer
        y = out
        st = y.stride()
        ypitch = _pitch_of(y)
        if not ypitch and st[3] == 1 and st[2] > W and st[2] % 4 == 0 and st[1] == H * st[2]:
            ypitch = st[2]      # a channel slice of a row-pitched buffer (the DeepLabv3+ concat)
        if tuple(y.shape) != tuple(x.shape) or (not ypitch and (st[3] != 1 or st[2] != W or st[1] != H * W)):
            raise RuntimeError("bn_apply: out must have dense images or be a row-pitched buffer")
        yns = st[0]
    nbytes = (8.0 + (4.0 if residual is not None else 0.0)) * x.numel()
    _timed("bn_apply", None, nbytes, lambda: check(
        _lib.lib().dcfp_bn_apply_f32(_p(x), _p(mean), _p(var), _p(gamma), _p(beta), float(eps),
                                     _p(residual), int(relu), _p(y), yns, N, Cc, H * W, W, ypitch, _stream()),
        "bn_apply"))
    return y


def bn_apply_relu_mask(x, mean, var, gamma, beta, eps, residual):
    """y = relu(BN(x) + residual) plus the ReLU mask as one bit per element (int64 words), or None where
    the library has no mask path for the shape (HW % 256 != 0)."""
    N, Cc, H, W = x.shape
    if (H * W) % 256 != 0:
        return None
    x = x.contiguous(); residual = residual.contiguous()
    y = torch.empty_like(x)
    mask = torch.empty(x.numel() // 64, dtype=torch.int64, device=x.device)
    rc = [0]

    def run():
        rc[0] = _lib.lib().dcfp_bn_apply_relu_mask_f32(_p(x), _p(mean), _p(var), _p(gamma), _p(beta), float(eps),
                                                       _p(residual), _p(y), _p(mask), N, Cc, H * W, _stream())
    _timed("bn_apply", None, 12.125 * x.numel(), run)
    if rc[0] == _lib.E_UNSUPPORTED:
        return None
    check(rc[0], "bn_apply_relu_mask")
    return y, mask


def bn_bwd_reduce(dy, x, y, mean, var, gamma, beta, eps, relu, dgamma=None, dbeta=None):
    """relu: 0 none, 1 mask from y, 2 mask re-derived from x (forward had no residual), 3 `y` is the
    1-bit-per-element mask written by bn_apply_relu_mask.  Returns (sum_dy, sum_dy_xmu) adjacent in one
    buffer, and dgamma; dgamma / dbeta (optional C-float destinations: the parameters' gradient slots)
    receive sum_dy_xmu * istd and a copy of sum_dy."""
    N, Cc, H, W = x.shape
    dy, dns = _batch_strided(dy)
    L = _lib.lib()
    ws = _workspace("bn", L.dcfp_bn_workspace_bytes(N, Cc, H * W), x.device)
    s = torch.empty((2, Cc), dtype=torch.float32, device=x.device)
    s1, s2 = s[0], s[1]
    if dgamma is None:
        dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device)
    _timed("bn_bwd_reduce", None, (8.0 + (4.0 if relu == 1 else 0.125 if relu == 3 else 0.0)) * x.numel(), lambda: check(
        L.dcfp_bn_bwd_reduce_f32(_p(dy), dns, _p(x), _p(y) if relu in (1, 3) else None, 0, _p(mean), _p(var),
                                 _p(gamma), _p(beta), float(eps), int(relu), N, Cc, H * W, _p(s1), _p(s2),
                                 _p(dgamma), _p(dbeta), _p(ws), ws.numel(), _stream()),
        "bn_bwd_reduce"))
    return s1, s2, dgamma


def bn_bwd_apply(dy, x, y, mean, var, gamma, beta, eps, s1, s2, count, relu, want_residual, dx_out=None):
    """dx_out: optional row-pitched destination (pitched_buffer) for dx."""
    N, Cc, H, W = x.shape
    dy, dns = _batch_strided(dy)
    dxp = 0
    if dx_out is not None:
        dxp = _pitch_of(dx_out)
        if tuple(dx_out.shape) != tuple(x.shape) or not dxp:
            raise RuntimeError("bn_bwd_apply: dx_out must be a row-pitched buffer of x's shape")
        dx = dx_out
    else:
        dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_residual else None
    nbytes = (12.0 + (4.0 if relu == 1 else 0.125 if relu == 3 else 0.0) + (4.0 if want_residual else 0.0)) * x.numel()
    count_dev = count if isinstance(count, torch.Tensor) else None   # SyncBN: global count on device
    count_host = 0.0 if count_dev is not None else float(count)
    _timed("bn_bwd_apply", None, nbytes, lambda: check(
        _lib.lib().dcfp_bn_bwd_apply_f32(_p(dy), dns, _p(x), _p(y) if relu in (1, 3) else None, 0, _p(mean),
                                         _p(var), _p(gamma), _p(beta), float(eps), _p(s1), _p(s2), count_host,
                                         _p(count_dev), int(relu), _p(dx), _p(dres), N, Cc, H * W, W, dxp,
                                         _stream()),
        "bn_bwd_apply"))
    return dx, dres


# ---- the fused BatchNorm backward (dcfp_bn_bwd_fused_f32): both stages in one launch, dy and x read once.
# DCFP_BN_FUSED=0 keeps the two-kernel path (which the data-parallel path always takes: its sums cross the ranks).
BN_BWD_FUSED = os.environ.get("DCFP_BN_FUSED", "1") != "0"
FUSED_BN_USED = [0]            # launches since import (tests read it)
_FUSED_SYNC = {}               # (device index, stream) -> [hand-off buffer, last epoch, status word]


def _fused_sync(nbytes, device):
    """The hand-off buffer of the fused kernel's blocks, its next epoch and the give-up status word: zero-filled when
    created or grown, epochs strictly increasing per buffer (the contract of dcfp_bn_bwd_fused_f32)."""
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    st = _FUSED_SYNC.get(key)
    if st is None:
        st = [None, 0, torch.zeros(1, dtype=torch.int32, device=device)]
        _FUSED_SYNC[key] = st
    if st[0] is None or st[0].numel() < nbytes or st[1] >= 0xfffffff0:
        st[0] = torch.zeros(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        st[1] = 0
    st[1] += 1
    return st[0], st[1], st[2]


def check_fused_status():
    """Once per step, next to the step's own host synchronisation: raise if a block of a fused BatchNorm backward gave
    up waiting for the other blocks of its channel (its outputs were poisoned with NaN)."""
    for (dev, _), st in _FUSED_SYNC.items():
        v = int(st[2].item())
        if v != 0:
            raise RuntimeError("dcfp_amd: fused BatchNorm backward (call %d on device %s) gave up waiting for the blocks of "
                               "a channel; its outputs are NaN.  DCFP_BN_FUSED=0 selects the two-kernel path" % (v, dev))


def bn_bwd_fused(dy, x, y, mean, var, gamma, beta, eps, count, relu, want_residual, dx_out=None, dgamma=None, dbeta=None):
    """bn_bwd_reduce + bn_bwd_apply in one launch (same bits).  Returns (s1, s2, dgamma, dx, dres), or None when the
    shape is not supported by the fused kernel (the caller then takes the two-kernel path)."""
    N, Cc, H, W = x.shape
    L = _lib.lib()
    need = L.dcfp_bn_bwd_fused_sync_bytes(N, Cc, H * W)
    if need == 0:
        return None
    dy, dns = _batch_strided(dy)
    dxp = 0
    if dx_out is not None:
        dxp = _pitch_of(dx_out)
        if tuple(dx_out.shape) != tuple(x.shape) or not dxp:
            raise RuntimeError("bn_bwd_fused: dx_out must be a row-pitched buffer of x's shape")
        dx = dx_out
    else:
        dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_residual else None
    s = torch.empty((2, Cc), dtype=torch.float32, device=x.device)
    if dgamma is None:
        dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device)
    sync, epoch, status = _fused_sync(need, x.device)
    nbytes = (12.0 + (4.0 if relu == 1 else 0.125 if relu == 3 else 0.0) + (4.0 if want_residual else 0.0)) * x.numel()
    rc = [0]

    def run():
        rc[0] = L.dcfp_bn_bwd_fused_f32(_p(dy), dns, _p(x), _p(y) if relu in (1, 3) else None, 0, _p(mean), _p(var),
                                        _p(gamma), _p(beta), float(eps), float(count), int(relu), _p(dx), _p(dres),
                                        N, Cc, H * W, W, dxp, _p(s[0]), _p(s[1]), _p(dgamma), _p(dbeta), _p(sync),
                                        sync.numel(), epoch, 0, _p(status), _stream())
    _timed("bn_bwd_fused", None, nbytes, run)
    if rc[0] == _lib.E_UNSUPPORTED:
        return None
    check(rc[0], "bn_bwd_fused")
    FUSED_BN_USED[0] += 1
    return s[0], s[1], dgamma, dx, dres


def _sync_group(group):
    if group is False or not dist.is_available() or not dist.is_initialized():
        return None
    g = None if group is True else group
    if dist.get_world_size(g) <= 1 and not os.environ.get("DCFP_FORCE_SYNCBN"):
        return None   # (the env switch rehearses the exchange at world size 1)
    return g if g is not None else dist.group.WORLD


_COUNT_CACHE = {}


def _count_tensor(count, device):
    """Per-rank pixel count as a one-float device tensor, uploaded once per distinct value (a fresh
    torch.tensor(..., device=cuda) per BN layer is a blocking H2D copy: 115 pipeline drains per step)."""
    key = (float(count), str(device))
    t = _COUNT_CACHE.get(key)
    if t is None:
        t = torch.tensor([float(count)], device=device, dtype=torch.float32)
        _COUNT_CACHE[key] = t
    return t


def syncbn_combine_reference(allv, Cc):
    """The pooled statistics of `world` gathered rows (mean[C], var[C], count) - the ONE formula both the
    HIP kernel (syncbn_combine_kernel in csrc/bn.hip) and the host path below evaluate, in fp64 and in
    rank order:  tot = sum n_r;  m = (sum mean_r n_r)/tot;  v = (sum (var_r + (mean_r - m)^2) n_r)/tot."""
    a = allv.double()
    world = a.shape[0]
    n = a[:, 2 * Cc]
    tot = torch.zeros((), dtype=torch.float64, device=a.device)
    m = torch.zeros(Cc, dtype=torch.float64, device=a.device)
    for r in range(world):
        tot = tot + n[r]
        m = m + a[r, :Cc] * n[r]
    m = m / tot
    v = torch.zeros(Cc, dtype=torch.float64, device=a.device)
    for r in range(world):
        dlt = a[r, :Cc] - m
        v = v + (a[r, Cc:2 * Cc] + dlt * dlt) * n[r]
    return m.float(), (v / tot).float(), tot.float().reshape(1)


def sync_bn_stats(mean, var, count, group, run=None, running=None):
    """SyncBatchNorm forward exchange (engine.py:65): ONE all_gather of [mean, var, count]
    (2C+1 floats per rank), then the pooled mean / biased variance over all ranks' pixels
    (parallel-variance combination), identical on every rank; the total count stays on the device.
    run (device path) / running = (running_mean, running_var, momentum, nbt) (host path): the running
    statistics are updated from the POOLED statistics, as nn.SyncBatchNorm does."""
    Cc = mean.numel()
    world = dist.get_world_size(group)
    local = torch.cat([mean, var, _count_tensor(count, mean.device)])
    px = syncbn_p2p.for_group(group) if mean.is_cuda else None
    if px is not None:       # one launch: peer-to-peer gather + the same rank-order fp64 combination
        out = torch.empty(2 * Cc + 1, device=mean.device, dtype=torch.float32)
        _timed("syncbn_p2p_fwd", None, 4.0 * local.numel() * world, lambda: px.exchange(local, out, 2, _rp(run)))
        return out[:Cc], out[Cc:2 * Cc], out[2 * Cc:]
    allv = torch.empty(world, local.numel(), device=mean.device, dtype=mean.dtype)
    # (exposed on the compute stream: the normalisation that follows needs the pooled statistics; bench.py sums these)
    if mean.is_cuda:
        _timed("syncbn_allgather", None, 4.0 * local.numel() * world,
               lambda: dist.all_gather_into_tensor(allv, local.unsqueeze(0), group=group))
    else:
        dist.all_gather_into_tensor(allv, local.unsqueeze(0), group=group)
    if mean.is_cuda:
        out = torch.empty(2 * Cc + 1, device=mean.device, dtype=torch.float32)
        check(_lib.lib().dcfp_syncbn_combine_f32(_p(allv), world, Cc, _p(out), _p(out[Cc:]), _p(out[2 * Cc:]),
                                                 _rp(run), _stream()), "syncbn_combine")
        return out[:Cc], out[Cc:2 * Cc], out[2 * Cc:]
    # host tensors (the gloo tests): the same formula, evaluated by torch in fp64
    gmean, gvar, total = syncbn_combine_reference(allv, Cc)
    if running is not None:
        rm, rv, momentum, nbt = running
        if rm is not None and momentum is not None:
            n = float(total)
            rm.mul_(1.0 - momentum).add_(gmean, alpha=momentum)
            rv.mul_(1.0 - momentum).add_(gvar * (n / max(n - 1.0, 1.0)), alpha=momentum)
        if nbt is not None:
            nbt.add_(1)
    return gmean.contiguous(), gvar.contiguous(), total.contiguous()


def sync_bn_bwd_sums(s1, s2, group, async_op=False):
    """SyncBatchNorm backward exchange: ONE all_reduce(SUM) of [sum g, sum g*(x-mean)] (2C floats);
    bn_bwd_reduce returns the two rows adjacent in one buffer, which is then reduced in place.
    async_op: returns (s1, s2, work) with the exchange in flight on the collective's stream - the caller
    enqueues independent kernels (a weight gradient) and calls work.wait() before it reads the sums."""
    Cc = s1.numel()
    adjacent = (s1.is_contiguous() and s2.is_contiguous()
                and s1.untyped_storage().data_ptr() == s2.untyped_storage().data_ptr()
                and s2.storage_offset() == s1.storage_offset() + Cc)
    px = syncbn_p2p.for_group(group) if s1.is_cuda else None
    if px is not None:       # one launch: peer-to-peer gather + sum in rank order (identical on every rank)
        both = s1.as_strided((2 * Cc,), (1,), s1.storage_offset()) if adjacent else torch.cat([s1, s2])
        out = torch.empty_like(both)
        if async_op:
            work = px.exchange_async(both, out, 1)
            return out[:Cc], out[Cc:], work
        _timed("syncbn_p2p_bwd", None, 8.0 * Cc * px.world, lambda: px.exchange(both, out, 1))
        return out[:Cc], out[Cc:]
    if adjacent:
        both = s1.as_strided((2 * Cc,), (1,), s1.storage_offset())
        work = dist.all_reduce(both, group=group, async_op=async_op)
        return (s1, s2, work) if async_op else (s1, s2)
    both = torch.cat([s1, s2])
    work = dist.all_reduce(both, group=group, async_op=async_op)
    r1, r2 = both[:Cc], both[Cc:]
    return (r1, r2, work) if async_op else (r1.contiguous(), r2.contiguous())


def bn_forward_impl(x, gamma, beta, running_mean, running_var, residual, relu, training,
                    momentum, eps, sync, nbt=None, stats=None, want_mask=False, out=None):
    """Shared BN(+ReLU)(+residual) forward: returns (y, state) with state =
    (mean, var, count, group) for the backward.  `stats` = this rank's (mean, biased var, running-updated?)
    when the producing conv already emitted them (conv2d_fwd(..., want_stats=True)).  nbt: the module's
    num_batches_tracked buffer (incremented by the kernel that finalises the statistics)."""
    _require(x, "x")
    x = x.contiguous()
    N, Cc, H, W = x.shape
    count = float(N * H * W)
    group = _sync_group(sync) if training else None
    if training:
        run = _bn_run(running_mean, running_var, momentum, nbt)
        if stats is not None:
            mean, var, applied = stats
            if applied:
                run = None
        elif group is None:
            mean, var = bn_stats(x, run)
            run = None
        else:
            mean, var = bn_stats(x)
        if group is not None:
            mean, var, count = sync_bn_stats(mean, var, count, group, run)
        elif run is not None:     # statistics came from elsewhere without the bookkeeping
            if running_mean is not None and momentum is not None:
                check(_lib.lib().dcfp_bn_update_running_f32(
                    _p(mean), _p(var), Cc, float(momentum), float(count), None, _p(running_mean),
                    _p(running_var), _stream()), "bn_update_running")
            if nbt is not None:
                nbt.add_(1)
    else:
        mean, var = running_mean, running_var
    if want_mask and relu and residual is not None and BN_RELU_BITMASK and out is None:
        ym = bn_apply_relu_mask(x, mean, var, gamma, beta, eps, residual)
        if ym is not None:
            return ym[0], (mean, var, count, group, ym[1])
    y = bn_apply(x, mean, var, gamma, beta, eps, residual, relu, out=out)
    return y, (mean, var, count, group)


def _bn_bwd_preface(relu, y, state, gamma, beta, gparam, bparam):
    """What both forms of the BN backward start with: the kernels' relu mode and the tensor it reads (bn_bwd_reduce), and
    the parameters that receive dgamma / dbeta with their gradient targets: (relu, y, gp, tg, kg, bp, tb, kb)."""
    mask = state[4] if len(state) > 4 else None
    if relu and mask is not None:      # residual BN whose forward kept the ReLU mask as bits
        relu, y = 3, mask
    else:
        relu = (1 if y is not None else 2) if relu else 0
    gp = gparam if gparam is not None else gamma
    bp = bparam if bparam is not None else beta
    return (relu, y, gp) + tuple(arena.grad_target(gp)) + (bp,) + tuple(arena.grad_target(bp))


def bn_backward_reduce(dy, x, y, gamma, beta, state, relu, training, gparam=None, bparam=None, eps=1e-5, pre=None):
    """First half of the BN backward: the two per-channel sums, dgamma / dbeta written to the parameters'
    gradient slots, and (SyncBN) the exchange of the sums started asynchronously.  Returns a tuple for
    bn_backward_apply; independent kernels enqueued between the two overlap the exchange."""
    mean, var, count, group = state[:4]
    relu, y, gp, tg, kg, bp, tb, kb = _bn_bwd_preface(relu, y, state, gamma, beta, gparam, bparam)
    if pre is not None:     # the producer of dy already reduced it per 128 pixels (conv2d_dgrad_fanin_red): finish the sums
        s1, s2, _ = bn_bwd_sums_from_partials(pre, var, eps, dgamma=tg, dbeta=tb)
    else:
        s1, s2, _ = bn_bwd_reduce(dy, x, y, mean, var, gamma, beta, eps, relu, dgamma=tg, dbeta=tb)
    dgamma = arena.grad_commit(gp, tg, kg, add_into)
    dbeta = arena.grad_commit(bp, tb, kb, add_into)
    work = None
    if training and group is not None:
        s1, s2, work = sync_bn_bwd_sums(s1, s2, group, async_op=SYNCBN_ASYNC)[:3] if SYNCBN_ASYNC else \
            sync_bn_bwd_sums(s1, s2, group) + (None,)
    elif not training:   # running statistics are constants: dx = g * gamma * istd
        s1 = torch.zeros_like(s1); s2 = torch.zeros_like(s2)
    return (s1, s2, work, relu, y, dgamma, dbeta)


def bn_backward_apply(dy, x, gamma, beta, state, red, eps, want_res, dx_out=None):
    s1, s2, work, relu, y, dgamma, dbeta = red
    if work is not None:
        # (bench.py sums these: how long the compute stream stands still for a backward SyncBN exchange that the weight
        #  gradient enqueued in between did not hide - comm.syncbn_bwd_exposed_ms)
        _timed("syncbn_bwd_wait", None, 0.0, work.wait)
    mean, var, count = state[:3]
    dx, dres = bn_bwd_apply(dy, x, y, mean, var, gamma, beta, eps, s1, s2, count, relu, want_res, dx_out)
    return dx, dgamma, dbeta, dres


def bn_backward_impl(dy, x, y, gamma, beta, state, relu, training, eps, want_res, gparam=None, bparam=None,
                     between=None, dx_out=None, pre=None):
    """Shared backward: returns (dx, dgamma, dbeta, dres).  dgamma/dbeta are this rank's sums (None when
    they went straight into the gradient arena; the gradient all-reduce averages them); under SyncBN the
    sums entering dx are global.  `y` is only needed for the ReLU mask of a BN that had a residual input;
    otherwise the mask is re-derived from x inside the kernels (pass y=None).  between: optional callable
    run after the reduction (and the start of the SyncBN exchange) and before dx - independent work
    that hides the exchange."""
    if relu and len(state) > 4 and state[4] is not None and not dy.is_contiguous():
        # the kernels that take the ReLU mask as bits want dy dense over the batch too (DCFP_E_UNSUPPORTED otherwise): a
        # gradient that arrives as a channel-slice view - the backward of a cat or a narrow behind the block - is copied once
        dy = dy.contiguous()
    if BN_BWD_FUSED and training and pre is None and state[3] is None and not isinstance(state[2], torch.Tensor):
        # no exchange between the two stages: one launch, dy and x read once
        frelu, fy, gp, tg, kg, bp, tb, kb = _bn_bwd_preface(relu, y, state, gamma, beta, gparam, bparam)
        out = bn_bwd_fused(dy, x, fy, state[0], state[1], gamma, beta, eps, state[2], frelu, want_res, dx_out,
                           dgamma=tg, dbeta=tb)
        if out is not None:
            dgamma = arena.grad_commit(gp, tg, kg, add_into)
            dbeta = arena.grad_commit(bp, tb, kb, add_into)
            mid = between() if between is not None else None
            return (out[3], dgamma, dbeta, out[4]) + ((mid,) if between is not None else ())
    red = bn_backward_reduce(dy, x, y, gamma, beta, state, relu, training, gparam, bparam, eps, pre=pre)
    mid = between() if between is not None else None
    out = bn_backward_apply(dy, x, gamma, beta, state, red, eps, want_res, dx_out)
    return out + ((mid,) if between is not None else ())


def _conv_bn_fwd(inp, w, bnargs, g, b, stride=1, pad=0, dil=1, relu=True, res=None, want_mask=False, out=None, keep=None):
    """conv -> BatchNorm (+residual) (+ReLU) of the fused nodes: (conv output, y, BN state).  bnargs: the BatchNorm's
    (running_mean, running_var, training, momentum, eps, sync, nbt).  With FUSE_BN_STATS the conv hands the batch
    statistics of its output to the BatchNorm behind it."""
    rm, rv, training, momentum, eps, sync, nbt = bnargs
    stats = None
    if FUSE_BN_STATS and training:
        # the kernel finalising the statistics also does the running-stat bookkeeping, unless the
        # statistics still have to be pooled over the ranks first (SyncBN)
        run = _bn_run(rm, rv, momentum, nbt) if _sync_group(sync) is None else None
        c, stats = conv2d_fwd(inp, w, None, stride, pad, dil, want_stats=True, bn_run=run, keep=keep)
    else:
        c = conv2d_fwd(inp, w, None, stride, pad, dil, keep=keep)
    y, state = bn_forward_impl(c, g, b, rm, rv, res, relu, training, momentum, eps, sync, nbt=nbt,
                               stats=stats, want_mask=want_mask, out=out)
    return c, y, state


def _pack_bn_states(states):
    """Per-BN backward states (bn_forward_impl; None entries allowed) -> (flat, meta): the tensors (mean, var, a
    device-side SyncBN count, the ReLU bit mask) go through save_for_backward (version checks), the rest stays python."""
    flat, meta = [], []
    for st in states:
        if st is None:
            meta.append(None)
            continue
        mean, var, count, group = st[:4]
        mask = st[4] if len(st) > 4 else None
        is_t = isinstance(count, torch.Tensor)
        meta.append((len(flat), is_t, None if is_t else count, group, mask is not None))
        flat += [mean, var] + ([count] if is_t else []) + ([mask] if mask is not None else [])
    return flat, meta


def _bn_state(meta, flat, i):
    """State i as bn_forward_impl returned it, from _pack_bn_states' meta and the saved tensors."""
    if meta[i] is None:
        return None
    pos, is_t, count, group, has_mask = meta[i]
    st = (flat[pos], flat[pos + 1], flat[pos + 2] if is_t else count, group)
    return st + ((flat[pos + 2 + is_t],) if has_mask else ())


def _concat_buffer(ctx, cfg, shape, device):
    """The output of a concat node: the persistent row-pitched buffer of cfg["owner"] (its lease kept on ctx) where
    cfg["pitch"] asks for one - decided by the caller: grad mode is off inside forward - else a dense tensor."""
    ctx.pitch_slot = None
    if cfg["pitch"]:
        cat, ctx.pitch_slot = owner_pitched(cfg["owner"], shape, cfg["pitch"], device)
        return cat
    return torch.empty(shape, dtype=torch.float32, device=device)


def _release_pitch(ctx):
    """End of a node's backward: its pitched buffer may be reused by the next forward of its owner."""
    if ctx.pitch_slot is not None:
        ctx.pitch_slot.release()


class BatchNormActFn(torch.autograd.Function):
    """y = act(BN(x) [+ residual]) with batch statistics (training) or running statistics
    (eval).  Mirrors nn.BatchNorm2d + nn.ReLU(inplace) (+ the Bottleneck residual add,
    networks/backbone/resnet.py:41-56); `sync` reproduces nn.SyncBatchNorm (engine.py:65):
    statistics pooled over all ranks, gamma/beta gradients left local for the gradient
    all-reduce."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, residual, relu, training,
                momentum, eps, sync, nbt, pitch_cfg):
        x = x.contiguous()
        # pitch_cfg = (owner module, y_pitch, dx_pitch): write y row-pitched for the 3x3 conv that reads it next /
        # write dx row-pitched for the 3x3 conv that produced x (their shifted operands: conv_pitch)
        out, ctx.pitch_slot, ctx.dx_pitch, ctx.dx_key = None, None, 0, "bn_dx"
        if pitch_cfg is not None:
            owner, y_pitch, ctx.dx_pitch = pitch_cfg
            # (the gradient handed to autograd is a view of a persistent buffer: one per owning module, so that a later
            #  BatchNorm backward of the same shape cannot overwrite a gradient autograd still holds)
            ctx.dx_key = ("bn_dx", id(owner))
            if y_pitch and residual is None:
                out, ctx.pitch_slot = owner_pitched(owner, tuple(x.shape), y_pitch, x.device,
                                                    track=torch.is_grad_enabled())
        y, state = bn_forward_impl(x, gamma, beta, running_mean, running_var, residual, relu,
                                   training, momentum, eps, sync, nbt=nbt, out=out)
        flat, ctx.meta = _pack_bn_states([state])
        # y is saved only where the ReLU mask cannot be re-derived from x (residual input)
        ctx.save_for_backward(x, y if (relu and residual is not None) else None, *flat)
        ctx.params = (gamma, beta)
        ctx.cfg = (relu, training, eps, residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors[:2]
        gamma, beta = ctx.params
        relu, training, eps, has_res = ctx.cfg
        state = _bn_state(ctx.meta, ctx.saved_tensors[2:], 0)
        need_res = has_res and ctx.needs_input_grad[5]
        dx_out = pitched_buffer(tuple(x.shape), ctx.dx_pitch, ctx.dx_key, x.device) if ctx.dx_pitch else None
        dx, dgamma, dbeta, dres = bn_backward_impl(dy, x, y, gamma, beta, state, relu, training, eps, need_res,
                                                   dx_out=dx_out)
        _release_pitch(ctx)
        return dx, dgamma, dbeta, None, None, dres, None, None, None, None, None, None, None


class BottleneckFn(torch.autograd.Function):
    """One residual Bottleneck (networks/backbone/resnet.py:38-58) as a single autograd node:
    1x1 -> BN,ReLU -> 3x3(dil) -> BN,ReLU -> 1x1 -> BN (+residual) -> ReLU, with an optional
    1x1(stride)+BN downsample on the residual.  Same kernels as the op-level Functions; what the
    fusion buys is the backward: the block input receives two gradients (through conv1 and
    through the residual), and here conv1's dgrad ACCUMULATES into the residual gradient buffer
    instead of autograd adding two full tensors (33 full-size adds per step); every weight / gamma / beta
    gradient is written straight into the gradient arena; under SyncBN each weight gradient is enqueued
    between a BatchNorm's reduction and its dx so that it hides the exchange of the sums."""

    @staticmethod
    def forward(ctx, x, cfg, *tensors):
        # tensors: w1,g1,b1, w2,g2,b2, w3,g3,b3 [, wd,gd,bd]; cfg: dict of python values + BN buffers
        # (the block that produced x, if it left its bn3 record on the tensor: see the end of this function)
        ctx.prev_rec = getattr(x, "_dcfp_bn3_rec", None) if FANIN_BN_SUMS else None
        x = x.contiguous()
        has_ds = len(tensors) == 12
        w1, g1, b1, w2, g2, b2, w3, g3, b3 = tensors[:9]
        bnargs = cfg["bn"]   # per BN: (running_mean, running_var, training, momentum, eps, sync, nbt)
        stride, dil = cfg["stride"], cfg["dil"]

        # conv2 with dilation 1 / 2: its input y1 (and, in backward, the gradient of its output) are kept
        # row-pitched with a zero tail, so the 3x3 kernels copy every shifted quad without border handling.
        # y1 lives until this block's backward: one persistent buffer per block (cfg["owner"]), guarded by a
        # busy flag (a second forward before the backward gets a fresh buffer).
        N_, _, H_, W_ = x.shape
        y1_shape = (N_, w1.shape[0], H_, W_)
        pitch = conv_pitch(y1_shape, tuple(w2.shape), stride, dil, dil)
        y1_out, ctx.pitch_slot = None, None
        if pitch:
            y1_out, ctx.pitch_slot = owner_pitched(cfg.get("owner"), y1_shape, pitch, x.device)
        ctx.pitch = pitch
        c1, y1, st1 = _conv_bn_fwd(x, w1, bnargs[0], g1, b1, out=y1_out)
        # (conv2's Winograd input transform is kept for its weight gradient: 4x the size of y1, until this block's backward)
        ctx.keep2 = {} if ctx.needs_input_grad[5] else None      # inputs: x, cfg, w1, g1, b1, w2, ...
        c2, y2, st2 = _conv_bn_fwd(y1, w2, bnargs[1], g2, b2, stride, dil, dil, keep=ctx.keep2)
        if has_ds:
            wd, gd, bd = tensors[9:]
            cd, res, std = _conv_bn_fwd(x, wd, bnargs[3], gd, bd, stride, 0, 1, relu=False)
        else:
            cd, res, std = None, x, None
        c3, out, st3 = _conv_bn_fwd(y2, w3, bnargs[2], g3, b3, res=res, want_mask=True)
        ctx.has_ds = has_ds
        ctx.cfg = (stride, dil, [a[2] for a in bnargs], [a[4] for a in bnargs])
        ctx.params = tensors
        flat, ctx.meta = _pack_bn_states((st1, st2, st3, std))
        # with the 1-bit mask the block output is not needed by its own backward
        keep_out = out if len(st3) <= 4 else None
        ctx.save_for_backward(x, c1, y1, c2, y2, c3, keep_out, cd, *flat)
        # What the NEXT block needs to reduce this block's bn3 gradient in its fan-in epilogue (the gradient of `out` is
        # that fan-in's result): bn3's input, the ReLU bit mask and the batch mean.  The record travels on the output
        # tensor; the consumer leaves the partial sums in it and this block's backward picks them up.
        ctx.rec = None
        # (only when a backward pass can follow: a training-mode forward under no_grad builds no graph, and the record on
        #  its output would keep bn3's input alive for nothing)
        fused_bn3 = BN_BWD_FUSED and st3[3] is None and not FANIN_BN_SUMS_ALWAYS     # bn3's backward will be ONE launch
        if FANIN_BN_SUMS and not fused_bn3 and len(st3) > 4 and any(ctx.needs_input_grad):
            ctx.rec = {"c3": c3, "mask": st3[4], "mean": st3[0]}
            out._dcfp_bn3_rec = ctx.rec
        return out

    @staticmethod
    def backward(ctx, dout):
        x, c1, y1, c2, y2, c3, out, cd = ctx.saved_tensors[:8]
        flat = ctx.saved_tensors[8:]
        tensors = ctx.params
        w1, g1, b1, w2, g2, b2, w3, g3, b3 = tensors[:9]
        stride, dil, training, eps = ctx.cfg
        st1, st2, st3, std = (_bn_state(ctx.meta, flat, i) for i in range(4))

        def wg(dy, inp, w, st=1, pd=0, dl=1, keep=None):
            return lambda: wgrad_into_param(dy, inp, w, None, st, pd, dl, keep=keep)[0]

        # bn3 (+residual, ReLU): gradient of conv3's output and of the residual branch.  Identity-shortcut blocks whose
        # forward kept the ReLU mask as bits do not materialise the residual gradient dout * mask: conv1's dgrad adds
        # it from (dout, mask) in its epilogue (conv2d_dgrad_fanin) - 4 B/element less written per block
        mask3 = st3[4] if len(st3) > 4 else None
        fanin = (not ctx.has_ds and mask3 is not None and ctx.needs_input_grad[0] and dout.is_contiguous()
                 and tuple(dout.shape) == tuple(x.shape) and conv2d_dgrad_fanin_ok(None, w1, tuple(x.shape)))
        # bn3's sums may already sit in this block's record, reduced per 128 pixels by the fan-in that produced dout - but
        # only if dout IS that fan-in's result (autograd adds other consumers' gradients into a new tensor, or in place
        # with a version bump: either way the partial sums would be of something else)
        pre, rec = None, getattr(ctx, "rec", None)
        if rec is not None:
            part, ptr, ver = rec.pop("part", None), rec.pop("dx_ptr", None), rec.pop("dx_ver", None)
            if part is not None and dout.data_ptr() == ptr and dout._version == ver and dout.is_contiguous():
                pre = part
                FANIN_RED_USED[0] += 1
            # the record's references must not outlive this backward: the node object (ctx) stays until the whole graph
            # is dropped, and 33 blocks' bn3 inputs held that long are 14 GB of peak memory
            rec.clear()
            ctx.rec = None
        d_c3, dg3, db3, d_res = bn_backward_impl(dout, c3, out, g3, b3, st3, True, training[2], eps[2], not fanin, pre=pre)
        d_y2 = conv2d_dgrad(d_c3, w3, tuple(y2.shape), 1, 0, 1)
        # conv3's weight gradient does not feed bn2: it runs between bn2's reduction and its dx
        dc2_out = pitched_buffer(tuple(c2.shape), ctx.pitch, "d_c2", c2.device) if ctx.pitch else None
        d_c2, dg2, db2, _, dw3 = bn_backward_impl(d_y2, c2, None, g2, b2, st2, True, training[1], eps[1], False,
                                                  between=wg(d_c3, y2, w3), dx_out=dc2_out)
        d_y1 = conv2d_dgrad(d_c2, w2, tuple(y1.shape), stride, dil, dil)
        d_c1, dg1, db1, _, dw2 = bn_backward_impl(d_y1, c1, None, g1, b1, st1, True, training[0], eps[0], False,
                                                  between=wg(d_c2, y1, w2, stride, dil, dil, keep=ctx.keep2))
        grads = [None, dg1, db1, dw2, dg2, db2, dw3, dg3, db3]
        if ctx.has_ds:
            wd, gd, bd = tensors[9:]
            d_cd, dgd, dbd, _, dw1 = bn_backward_impl(d_res, cd, None, gd, bd, std, False, training[3], eps[3], False,
                                                      between=wg(d_c1, x, w1))
            dwd, _ = wgrad_into_param(d_cd, x, wd, None, stride, 0, 1)
            grads += [dwd, dgd, dbd]
            dx = conv2d_dgrad(d_cd, wd, tuple(x.shape), stride, 0, 1) if ctx.needs_input_grad[0] else None
        else:
            dw1, _ = wgrad_into_param(d_c1, x, w1, None, 1, 0, 1)
            dx = d_res
        grads[0] = dw1
        prev = ctx.prev_rec
        slots = 0
        if fanin and prev is not None and tuple(prev["c3"].shape) == tuple(x.shape):
            slots = conv2d_dgrad_fanin_red_slots(w1, tuple(x.shape))
        if fanin and slots > 0:
            # dx is the gradient arriving at the previous block's output: reduce it for that block's bn3 on the way out
            dx, part = conv2d_dgrad_fanin_red(d_c1, w1, tuple(x.shape), dout, mask3, prev["c3"], prev["mask"],
                                              prev["mean"], slots)
            prev["part"], prev["dx_ptr"], prev["dx_ver"] = part, dx.data_ptr(), dx._version
            del part
        elif fanin:
            dx = conv2d_dgrad_fanin(d_c1, w1, tuple(x.shape), dout, mask3)
        elif ctx.needs_input_grad[0]:
            dx = conv2d_dgrad(d_c1, w1, tuple(x.shape), 1, 0, 1, out=dx, accumulate=True)
        else:
            dx = None
        ctx.prev_rec = None
        _release_pitch(ctx)            # y1's buffer
        return (dx, None) + tuple(grads)


def bottleneck(x, cfg, tensors):
    return BottleneckFn.apply(x, cfg, *tensors)


def batch_norm_act(x, gamma, beta, running_mean, running_var, residual=None, relu=False,
                   training=True, momentum=0.1, eps=1e-5, sync=False, nbt=None, pitch_cfg=None):
    return BatchNormActFn.apply(x, gamma, beta, running_mean, running_var, residual, relu,
                                training, momentum, eps, sync, nbt, pitch_cfg)


class AsppFn(torch.autograd.Function):
    """The five ASPP branches and their concatenation (networks/tools/aspp.py:70-77) as ONE autograd node:
    1x1 / three dilated 3x3 conv -> BN -> ReLU, and global mean -> 1x1 conv -> BN -> ReLU -> broadcast,
    each writing its channel slice of the 1280-channel tensor directly (no torch.cat: the BN kernels take a
    batch stride).  Backward: the branches read their slice of the incoming gradient in place and their
    data gradients ACCUMULATE into one buffer through the dgrad epilogue (the reference's autograd adds
    five 2048-channel tensors: 4 read-read-write passes over 1 GB each); each branch's weight gradient
    runs between the next branch's BN reduction and its dx (hides the SyncBN exchange)."""

    @staticmethod
    def forward(ctx, x, cfg, *tensors):
        x = x.contiguous()
        N, Cin, H, W = x.shape
        widths = [t.shape[0] for t in tensors[0::3]]
        cat = torch.empty((N, sum(widths), H, W), dtype=torch.float32, device=x.device)
        offs = [sum(widths[:k]) for k in range(5)]
        states, cs, keeps = [], [], []
        for k in range(4):
            w, g, b = tensors[3 * k:3 * k + 3]
            pad, dil = cfg["convs"][k]
            kp = {} if ctx.needs_input_grad[2 + 3 * k] else None      # inputs: x, cfg, then (w, gamma, beta) per branch
            keeps.append(kp)
            c, _, st = _conv_bn_fwd(x, w, cfg["bn"][k], g, b, 1, pad, dil, out=cat[:, offs[k]:offs[k] + widths[k]],
                                    keep=kp)
            cs.append(c); states.append(st)
        w5, g5, b5 = tensors[12:15]
        rm, rv, training, momentum, eps, sync, nbt = cfg["bn"][4]
        pooled = rowsum(x, 1.0 / (H * W))                           # AdaptiveAvgPool2d(1) (aspp.py:56)
        c5 = conv2d_fwd(pooled, w5, None, 1, 0, 1)
        y5, st5 = bn_forward_impl(c5, g5, b5, rm, rv, None, True, training, momentum, eps, sync, nbt=nbt)
        broadcast_hw(y5, H, W, out=cat[:, offs[4]:offs[4] + widths[4]])   # bilinear 1x1 -> HxW (aspp.py:76)
        states.append(st5)
        ctx.keeps = keeps        # the branches' kept Winograd input transforms (released by their weight gradients)
        ctx.cfg = (cfg["convs"], [a[2] for a in cfg["bn"]], [a[4] for a in cfg["bn"]], offs, widths)
        ctx.params = tensors
        flat, ctx.meta = _pack_bn_states(states)
        ctx.save_for_backward(x, pooled, c5, *cs, *flat)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        x, pooled, c5 = ctx.saved_tensors[:3]
        cs = ctx.saved_tensors[3:7]
        flat = ctx.saved_tensors[7:]
        tensors = ctx.params
        convs, training, eps, offs, widths = ctx.cfg
        N, Cin, H, W = x.shape
        need_dx = ctx.needs_input_grad[0]
        grads = [None] * 15
        dx = None
        pending = None            # the previous branch's weight gradient, run inside the next BN backward
        for k in range(4):
            w, g, b = tensors[3 * k:3 * k + 3]
            pad, dil = convs[k]
            dslice = dcat[:, offs[k]:offs[k] + widths[k]]
            res = bn_backward_impl(dslice, cs[k], None, g, b, _bn_state(ctx.meta, flat, k), True, training[k], eps[k], False,
                                   between=pending)
            d_c, grads[3 * k + 1], grads[3 * k + 2] = res[0], res[1], res[2]
            if pending is not None:
                grads[3 * (k - 1)] = res[4]
            if need_dx:
                dx = conv2d_dgrad(d_c, w, tuple(x.shape), 1, pad, dil, out=dx, accumulate=dx is not None)
            pending = (lambda d_c=d_c, w=w, pad=pad, dil=dil, kp=ctx.keeps[k]:
                       wgrad_into_param(d_c, x, w, None, 1, pad, dil, keep=kp)[0])
        # image-pooling branch: broadcast^T = sum over pixels, then BN / 1x1 conv on N x C x 1 x 1
        w5, g5, b5 = tensors[12:15]
        g_y5 = rowsum(dcat[:, offs[4]:offs[4] + widths[4]], 1.0)
        res = bn_backward_impl(g_y5, c5, None, g5, b5, _bn_state(ctx.meta, flat, 4), True, training[4], eps[4], False, between=pending)
        d_c5, grads[13], grads[14], grads[9] = res[0], res[1], res[2], res[4]
        grads[12], _ = wgrad_into_param(d_c5, pooled, w5, None, 1, 0, 1)
        if need_dx:
            d_pooled = conv2d_dgrad(d_c5, w5, tuple(pooled.shape), 1, 0, 1)
            dx = broadcast_hw(d_pooled, H, W, 1.0 / (H * W), out=dx, accumulate=dx is not None)   # mean^T
        return (dx, None) + tuple(grads)


def aspp_branches(x, cfg, tensors):
    return AsppFn.apply(x, cfg, *tensors)


def _rows(t):
    """(batch stride, row pitch) of a [N,C,H,W] tensor with dense rows whose channels are H rows apart - a channel slice
    of a dense or row-pitched tensor (pitch 0: dense rows) - or None."""
    N, Cc, H, W = t.shape
    st = t.stride()
    if st[3] != 1 or st[2] < W or st[1] != H * st[2] or (st[2] != W and st[2] % 4) or (N > 1 and st[0] < Cc * H * st[2]):
        return None
    return (st[0] if N > 1 else Cc * H * st[2]), (st[2] if st[2] != W else 0)


def _rows_or_copy(t):
    """(t, batch stride, row pitch): t read in place where _rows describes it, else a contiguous copy of it."""
    r = _rows(t)
    if r is None:
        t = t.contiguous()
        r = _rows(t)
    return (t,) + r


def resize_bilinear_into(x, out, align_corners):
    """out[...] = F.interpolate(x, out.shape[2:], mode='bilinear', align_corners); `out` may be a channel slice of a
    batch-strided, row-pitched buffer (only its live floats are written)."""
    _require(x, "x"); _require(out, "out")
    x, xns = _batch_strided(x)
    N, Cc, h, w = x.shape
    H, W = out.shape[2], out.shape[3]
    r = _rows(out)
    if r is None or out.shape[0] != N or out.shape[1] != Cc:
        raise RuntimeError("resize_bilinear_into: out must be [N,C,H,W] with dense rows (a channel slice is fine)")
    _timed("resize_fwd", None, 4.0 * (x.numel() + out.numel()), lambda: check(
        _lib.lib().dcfp_resize_bilinear_into_f32(_p(x), xns, N, Cc, h, w, _p(out), r[0], r[1], H, W,
                                                 int(bool(align_corners)), _stream()), "resize_bilinear_into"))
    return out


def resize_bilinear_adjoint(dy, size, align_corners, out=None, accumulate=False):
    """dx (+)= interpolate^T(dy) for an input of spatial `size`; dy may be a channel slice of a batch-strided (row-pitched)
    tensor, read in place.  Deterministic (gather form, fixed summation order)."""
    _require(dy, "dy")
    dy, dns, dpitch = _rows_or_copy(dy)
    N, Cc, H, W = dy.shape
    h, w = int(size[0]), int(size[1])
    if out is None:
        dx = torch.empty((N, Cc, h, w), dtype=torch.float32, device=dy.device)
        accumulate = False
    else:
        dx = out
        if tuple(dx.shape) != (N, Cc, h, w) or not dx.is_contiguous():
            raise RuntimeError("resize_bilinear_adjoint: out must be a contiguous [N,C,h,w] tensor")
    _timed("resize_adjoint", None, 4.0 * (dy.numel() + dx.numel()), lambda: check(
        _lib.lib().dcfp_resize_bilinear_adjoint_f32(_p(dy), dns, dpitch, N, Cc, H, W, _p(dx), Cc * h * w, h, w,
                                                    int(bool(align_corners)), int(bool(accumulate)), _stream()),
        "resize_bilinear_adjoint"))
    return dx


class DecoderConcatFn(torch.autograd.Function):
    """The DeepLabv3+ decoder's concat (networks/deeplabv3p.py:31-38) as ONE autograd node:
    cat(interpolate(x, size of low), relu(bn1(conv1(low)))) written into one buffer - row-pitched for the 3x3 conv that
    reads it (ops.conv_pitch) - by its two producers: the resize kernel into channels [0, Cx), the BatchNorm apply of the
    1x1 conv's output into channels [Cx, Cx + C1).  No torch.cat, no copy.  Backward: both slices of the incoming
    gradient are read in place; the resize adjoint runs between the BatchNorm reduction and its dx (hides the SyncBN
    exchange), then conv1's dgrad (d low) and weight gradient."""

    @staticmethod
    def forward(ctx, x, low, cfg, w1, g1, b1):
        _require(x, "x"); _require(low, "low")
        low = low.contiguous()
        N, Cx, h, w = x.shape
        _, Cl, H, W = low.shape
        C1 = w1.shape[0]
        cat = _concat_buffer(ctx, cfg, (N, Cx + C1, H, W), x.device)
        align = cfg["align"]
        resize_bilinear_into(x, cat[:, :Cx], align)
        ctx.keep = {} if ctx.needs_input_grad[3] else None
        c, _, st = _conv_bn_fwd(low, w1, cfg["bn"], g1, b1, out=cat[:, Cx:], keep=ctx.keep)
        flat, ctx.meta = _pack_bn_states([st])
        ctx.save_for_backward(low, c, *flat)
        ctx.params = (w1, g1, b1)
        ctx.cfg = (cfg["bn"][2], cfg["bn"][4], Cx, (h, w), align)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        low, c = ctx.saved_tensors[:2]
        w1, g1, b1 = ctx.params
        training, eps, Cx, hw, align = ctx.cfg
        state = _bn_state(ctx.meta, ctx.saved_tensors[2:], 0)
        dx = [None]

        def adjoint():
            if ctx.needs_input_grad[0]:
                dx[0] = resize_bilinear_adjoint(dcat[:, :Cx], hw, align)
        res = bn_backward_impl(dcat[:, Cx:], c, None, g1, b1, state, True, training, eps, False, between=adjoint)
        d_c, dg, db = res[0], res[1], res[2]
        dlow = conv2d_dgrad(d_c, w1, tuple(low.shape), 1, 0, 1) if ctx.needs_input_grad[1] else None
        dw = wgrad_into_param(d_c, low, w1, None, 1, 0, 1, keep=ctx.keep)[0] if ctx.needs_input_grad[3] else None
        _release_pitch(ctx)
        return dx[0], dlow, None, dw, dg, db


def decoder_concat(x, low, cfg, w1, g1, b1):
    return DecoderConcatFn.apply(x, low, cfg, w1, g1, b1)


def _int_array(vals):
    vals = [int(v) for v in vals]
    return (C.c_int * len(vals))(*vals)


def _pool_levels(levels):
    levels = [(int(a), int(b)) for a, b in levels]
    if not 1 <= len(levels) <= 4 or any(not (1 <= a <= 8 and 1 <= b <= 8) for a, b in levels):
        raise RuntimeError(f"dcfp_amd: the pyramid pooling kernels take 1 to 4 levels of sizes 1..8, got {levels}")
    return levels


def _level_views(buf, N, widths, levels):
    out, off = [], 0
    for Cc, (a, b) in zip(widths, levels):
        n = N * Cc * a * b
        out.append(buf[off:off + n].view(N, Cc, a, b))
        off += n
    return out


def ppm_pool(x, levels, mean=True, dst=None):
    """F.adaptive_avg_pool2d(x, (sh, sw)) for every (sh, sw) of `levels` (1 to 4, sizes <= 8; sums when not `mean`) in
    one sweep over x: [N, C, sh, sw] views of one level-major buffer.  dst: optionally also copies x into it (a channel
    slice of a batch-strided, row-pitched tensor; only the live floats are written)."""
    _require(x, "x")
    levels = _pool_levels(levels)
    x = x.contiguous()
    N, Cc, H, W = x.shape
    buf = torch.empty(sum(N * Cc * a * b for a, b in levels), dtype=torch.float32, device=x.device)
    dns, dpitch = 0, 0
    if dst is not None:
        _require(dst, "dst")
        r = _rows(dst)
        if r is None or tuple(dst.shape) != (N, Cc, H, W):
            raise RuntimeError("ppm_pool: dst must be [N,C,H,W] with dense rows (a channel slice is fine)")
        dns, dpitch = r
    _timed("ppm_pool", None, 4.0 * x.numel() * (2 if dst is not None else 1), lambda: check(
        _lib.lib().dcfp_ppm_pool_f32(_p(x), N, Cc, H, W, len(levels), _int_array(v for hw in levels for v in hw),
                                     _p(buf), int(bool(mean)), _p(dst), dns, dpitch, _stream()), "ppm_pool"))
    return _level_views(buf, N, [Cc] * len(levels), levels)


def ppm_pool_adjoint(dp, levels, shape, g=None):
    """dx = g + the adjoint of ppm_pool(mean=True): dp is the flat level-major buffer of the levels' [N,C,sh,sw]
    gradients; g (optional) is read in place, dense or a row-pitched channel slice."""
    levels = _pool_levels(levels)
    N, Cc, H, W = [int(v) for v in shape]
    _require(dp, "dp")
    if dp.numel() != sum(N * Cc * a * b for a, b in levels) or not dp.is_contiguous():
        raise RuntimeError("ppm_pool_adjoint: dp must hold the level-major [N,C,sh,sw] blocks of every level")
    gns, gpitch = 0, 0
    if g is not None:
        _require(g, "g")
        g, gns, gpitch = _rows_or_copy(g)
        if tuple(g.shape) != (N, Cc, H, W):
            raise RuntimeError("ppm_pool_adjoint: g must be [N,C,H,W]")
    dx = torch.empty((N, Cc, H, W), dtype=torch.float32, device=dp.device)
    _timed("ppm_pool_adjoint", None, 4.0 * dx.numel() * (2 if g is not None else 1), lambda: check(
        _lib.lib().dcfp_ppm_pool_adjoint_f32(_p(dp), N, Cc, H, W, len(levels),
                                             _int_array(v for hw in levels for v in hw), _p(g), gns, gpitch, _p(dx),
                                             _stream()), "ppm_pool_adjoint"))
    return dx


def ppm_resize_adjoint(dy, widths, levels, align_corners):
    """The adjoint of F.interpolate(bilinear) from small grids, for every level at once: dy [N, sum(widths), H, W] holds
    the levels' channel slices in order (read in place, dense or a row-pitched slice); returns the [N, C_l, sh, sw]
    gradients, views of one level-major buffer.  Deterministic (fixed summation order)."""
    _require(dy, "dy")
    levels = _pool_levels(levels)
    dy, dns, dpitch = _rows_or_copy(dy)
    N, Ct, H, W = dy.shape
    if Ct != sum(widths) or len(widths) != len(levels):
        raise RuntimeError("ppm_resize_adjoint: dy must hold the levels' channels in order")
    buf = torch.empty(sum(N * c * a * b for c, (a, b) in zip(widths, levels)), dtype=torch.float32, device=dy.device)
    chw = [v for c, (a, b) in zip(widths, levels) for v in (c, a, b)]
    _timed("ppm_resize_adjoint", None, 4.0 * (dy.numel() + buf.numel()), lambda: check(
        _lib.lib().dcfp_ppm_resize_adjoint_f32(_p(dy), dns, dpitch, N, H, W, len(levels), _int_array(chw), _p(buf),
                                               int(bool(align_corners)), _stream()), "ppm_resize_adjoint"))
    return _level_views(buf, N, widths, levels)


class AdaptiveAvgPoolFn(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d((sh, sw)) for output sizes up to 8 (the PSPNet pyramid, networks/tools/ppm.py:27)."""

    @staticmethod
    def forward(ctx, x, sh, sw):
        _require(x, "x")
        ctx.shape = tuple(x.shape)
        ctx.hw = (sh, sw)
        return ppm_pool(x, [(sh, sw)])[0]

    @staticmethod
    def backward(ctx, dy):
        return ppm_pool_adjoint(dy.contiguous().reshape(-1), [ctx.hw], ctx.shape), None, None


def adaptive_avg_pool(x, size):
    sh, sw = (size, size) if isinstance(size, int) else size
    return AdaptiveAvgPoolFn.apply(x, int(sh), int(sw))


class PyramidPoolingFn(torch.autograd.Function):
    """The pyramid pooling module of PSPNet (networks/tools/ppm.py:33-37) up to its concat, as ONE autograd node:
    cat([interpolate(relu(bn_k(conv_k(adaptive_avg_pool(feats, s_k))))) for each stage k] + [feats]) written into one
    buffer - row-pitched for the 3x3 conv that reads it (ops.conv_pitch) - with no torch.cat.  One sweep over feats pools
    every level and copies feats into its slice; each stage's 1x1 conv -> BatchNorm -> ReLU runs on its s x s map and is
    resized into its slice.  Backward: both regions of the incoming gradient are read in place: the small-grid bilinear
    adjoint of all stages in one launch, per stage the BatchNorm backward, dgrad and weight gradient (the weight gradient
    of one stage runs between the next stage's BatchNorm reduction and its dx: hides the SyncBN exchange), then the pool
    adjoint adds the stages' pooled gradients to the feats slice."""

    @staticmethod
    def forward(ctx, feats, cfg, *tensors):
        _require(feats, "feats")
        feats = feats.contiguous()
        N, Cf, H, W = feats.shape
        nst = len(tensors) // 3
        widths = [int(t.shape[0]) for t in tensors[0::3]]
        levels = [(int(s), int(s)) for s in cfg["sizes"]]
        offs = [sum(widths[:k]) for k in range(nst + 1)]
        cat = _concat_buffer(ctx, cfg, (N, offs[nst] + Cf, H, W), feats.device)
        align = cfg["align"]
        pooled = ppm_pool(feats, levels, True, dst=cat[:, offs[nst]:])
        cs, states = [], []
        for k in range(nst):
            w, g, b = tensors[3 * k:3 * k + 3]
            rm, rv, training, momentum, eps, sync, nbt = cfg["bn"][k]
            c = conv2d_fwd(pooled[k], w, None, 1, 0, 1)
            y, st = bn_forward_impl(c, g, b, rm, rv, None, True, training, momentum, eps, sync, nbt=nbt)
            resize_bilinear_into(y, cat[:, offs[k]:offs[k + 1]], align)
            cs.append(c); states.append(st)
        flat, ctx.meta = _pack_bn_states(states)
        ctx.params = tensors
        ctx.cfg = (levels, widths, offs, (N, Cf, H, W), align, [a[2] for a in cfg["bn"]], [a[4] for a in cfg["bn"]])
        ctx.save_for_backward(*pooled, *cs, *flat)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        levels, widths, offs, fshape, align, training, eps = ctx.cfg
        nst = len(widths)
        saved = ctx.saved_tensors
        pooled, cs, flat = saved[:nst], saved[nst:2 * nst], saved[2 * nst:]
        tensors = ctx.params
        N, Cf, H, W = fshape
        need_dx = ctx.needs_input_grad[0]
        grads = [None] * (3 * nst)
        dys = ppm_resize_adjoint(dcat[:, :offs[nst]], widths, levels, align)
        dp = torch.empty(sum(N * Cf * a * b for a, b in levels), dtype=torch.float32, device=dcat.device) \
            if need_dx else None
        dps = _level_views(dp, N, [Cf] * nst, levels) if need_dx else None
        pending = None             # the previous stage's weight gradient, run inside the next BatchNorm backward
        for k in range(nst):
            w, g, b = tensors[3 * k:3 * k + 3]
            res = bn_backward_impl(dys[k], cs[k], None, g, b, _bn_state(ctx.meta, flat, k), True, training[k], eps[k], False,
                                   between=pending)
            d_c, grads[3 * k + 1], grads[3 * k + 2] = res[0], res[1], res[2]
            if pending is not None:
                grads[3 * (k - 1)] = res[4]
            if need_dx:
                conv2d_dgrad(d_c, w, tuple(pooled[k].shape), 1, 0, 1, out=dps[k])
            pending = (lambda d_c=d_c, w=w, x=pooled[k]: wgrad_into_param(d_c, x, w, None, 1, 0, 1)[0])
        grads[3 * (nst - 1)] = pending()
        dfeats = ppm_pool_adjoint(dp, levels, fshape, g=dcat[:, offs[nst]:]) if need_dx else None
        _release_pitch(ctx)
        return (dfeats, None) + tuple(grads)


def pyramid_pooling(feats, cfg, tensors):
    return PyramidPoolingFn.apply(feats, cfg, *tensors)


class ForkFn(torch.autograd.Function):
    """x -> (x, x) for a tensor with two consumers (layer3's output feeds layer4 and the deep-supervision
    head, networks/deeplabv3.py:44-50): the two incoming gradients are summed by dcfp_add_f32."""

    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)      # an unused tap (deepsup=False) sends None, not a zero tensor + a full add
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None or gb is None:
            return ga if gb is None else gb
        return add(ga, gb)


def fork(x):
    return ForkFn.apply(x) if (torch.is_grad_enabled() and x.requires_grad) else (x, x)


# ---------------------------------------------------------------- pooling
class MaxPool3x3s2Fn(torch.autograd.Function):
    """nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (networks/backbone/resnet.py:100)."""

    @staticmethod
    def forward(ctx, x):
        _require(x, "x")
        x = x.contiguous()
        N, Cc, H, W = x.shape
        Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        y = torch.empty((N, Cc, Ho, Wo), dtype=torch.float32, device=x.device)
        idx = torch.empty((N, Cc, Ho, Wo), dtype=torch.int32, device=x.device)
        check(_lib.lib().dcfp_maxpool3x3s2_fwd_f32(_p(x), _p(y), _p(idx), N, Cc, H, W, Ho, Wo, _stream()),
              "maxpool_fwd")
        ctx.save_for_backward(idx)
        ctx.shape = (N, Cc, H, W, Ho, Wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        N, Cc, H, W, Ho, Wo = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty((N, Cc, H, W), dtype=torch.float32, device=dy.device)
        check(_lib.lib().dcfp_maxpool3x3s2_bwd_f32(_p(dy), _p(idx), _p(dx), N, Cc, H, W, Ho, Wo, _stream()),
              "maxpool_bwd")
        return dx


def maxpool3x3s2(x):
    return MaxPool3x3s2Fn.apply(x)


def rowsum(x, scale):
    N, Cc, H, W = x.shape
    x, ns = _batch_strided(x)
    y = torch.empty((N, Cc, 1, 1), dtype=torch.float32, device=x.device)
    check(_lib.lib().dcfp_rowsum_f32(_p(x), ns, _p(y), float(scale), N, Cc, H * W, _stream()), "rowsum")
    return y


def broadcast_hw(v, H, W, scale=1.0, out=None, accumulate=False):
    """y[n,c,:,:] (+)= scale * v[n,c]; out: optional destination with dense images (a channel slice)."""
    N, Cc = v.shape[0], v.shape[1]
    v = v.contiguous()
    yns = 0
    if out is None:
        y = torch.empty((N, Cc, H, W), dtype=torch.float32, device=v.device)
        accumulate = False
    else:
        y = out
        st = y.stride()
        if tuple(y.shape) != (N, Cc, H, W) or st[3] != 1 or st[2] != W or st[1] != H * W:
            raise RuntimeError("broadcast_hw: out must be [N,C,H,W] with dense images")
        yns = st[0]
    check(_lib.lib().dcfp_broadcast_hw_f32(_p(v), float(scale), _p(y), yns, int(bool(accumulate)), N, Cc, H * W,
                                           _stream()), "broadcast_hw")
    return y


class GlobalAvgPoolFn(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d((1,1)) (networks/tools/aspp.py:56)."""

    @staticmethod
    def forward(ctx, x):
        _require(x, "x")
        ctx.hw = (x.shape[2], x.shape[3])
        return rowsum(x, 1.0 / (x.shape[2] * x.shape[3]))

    @staticmethod
    def backward(ctx, dy):
        H, W = ctx.hw
        return broadcast_hw(dy, H, W, 1.0 / (H * W))


class BroadcastHWFn(torch.autograd.Function):
    """F.interpolate of a 1x1 map to HxW (networks/tools/aspp.py:76): a constant broadcast
    for either align_corners setting."""

    @staticmethod
    def forward(ctx, v, H, W):
        _require(v, "v")
        return broadcast_hw(v, H, W)

    @staticmethod
    def backward(ctx, dy):
        return rowsum(dy, 1.0), None, None


def global_avg_pool(x):
    return GlobalAvgPoolFn.apply(x)


def broadcast_to_hw(v, H, W):
    return BroadcastHWFn.apply(v, H, W)


class ChannelScaleFn(torch.autograd.Function):
    """nn.Dropout2d with a host-drawn per-(n,c) keep/scale mask (networks/deeplabv3.py:40)."""

    @staticmethod
    def forward(ctx, x, mask):
        _require(x, "x")
        x = x.contiguous()
        N, Cc, H, W = x.shape
        mask = mask.contiguous()
        y = torch.empty_like(x)
        check(_lib.lib().dcfp_channel_scale_f32(_p(x), _p(mask), _p(y), N, Cc, H * W, _stream()),
              "channel_scale")
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dy = dy.contiguous()
        N, Cc, H, W = dy.shape
        dx = torch.empty_like(dy)
        check(_lib.lib().dcfp_channel_scale_f32(_p(dy), _p(mask), _p(dx), N, Cc, H * W, _stream()),
              "channel_scale")
        return dx, None


def dropout2d(x, p, training, fixed_mask=None):
    if not training or p == 0.0:
        return x
    if fixed_mask is not None:
        mask = fixed_mask.to(device=x.device, dtype=torch.float32)
    else:
        mask = torch.empty(x.shape[0], x.shape[1], device=x.device).bernoulli_(1.0 - p).div_(1.0 - p)
    return ChannelScaleFn.apply(x, mask)


def add(a, b):
    """out = a + b through the library (gradient fan-in)."""
    a = a.contiguous(); b = b.contiguous()
    out = torch.empty_like(a)
    check(_lib.lib().dcfp_add_f32(_p(a), _p(b), _p(out), a.numel(), _stream()), "add")
    return out


# --------------------------------------------- bilinear upsample (+) cross-entropy
class UpsampleBilinearFn(torch.autograd.Function):
    """F.interpolate(x, size, mode='bilinear', align_corners) (networks/deeplabv3.py:47,50)."""

    @staticmethod
    def forward(ctx, x, H, W, align_corners):
        _require(x, "x")
        x = x.contiguous()
        N, Cc, h, w = x.shape
        y = torch.empty((N, Cc, H, W), dtype=torch.float32, device=x.device)
        check(_lib.lib().dcfp_upsample_bilinear_fwd_f32(_p(x), _p(y), N, Cc, h, w, H, W,
                                                        int(bool(align_corners)), _stream()),
              "upsample_fwd")
        ctx.cfg = (N, Cc, h, w, H, W, int(bool(align_corners)))
        return y

    @staticmethod
    def backward(ctx, dy):
        N, Cc, h, w, H, W, ac = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty((N, Cc, h, w), dtype=torch.float32, device=dy.device)
        check(_lib.lib().dcfp_upsample_bilinear_bwd_f32(_p(dy), _p(dx), N, Cc, h, w, H, W, ac, _stream()),
              "upsample_bwd")
        return dx, None, None, None


def upsample_bilinear(x, size, align_corners):
    return UpsampleBilinearFn.apply(x, int(size[0]), int(size[1]), align_corners)


def upsample_ce_forward(logits, labels, size, align_corners, ignore_index, pixel_keep=None,
                        want_gt_prob=False):
    """Returns (out2=[loss_sum, valid_count], lse[N,H,W], gt_prob or None)."""
    _require(logits, "logits")
    logits = logits.contiguous()
    if labels.dtype != torch.int64 or not labels.is_cuda:
        raise RuntimeError("upsample_ce: labels must be a CUDA int64 tensor [N,H,W]")
    labels = labels.contiguous()
    N, Cc, h, w = logits.shape
    H, W = int(size[0]), int(size[1])
    if tuple(labels.shape) != (N, H, W):
        raise RuntimeError(f"upsample_ce: labels shape {tuple(labels.shape)} != {(N, H, W)}")
    L = _lib.lib()
    ws = _workspace("ce", L.dcfp_upsample_ce_workspace_bytes(N, H, W), logits.device)
    out2 = torch.empty(2, dtype=torch.float32, device=logits.device)
    lse = torch.empty((N, H, W), dtype=torch.float32, device=logits.device)
    gtp = torch.empty((N, H, W), dtype=torch.float32, device=logits.device) if want_gt_prob else None
    if pixel_keep is not None:
        pixel_keep = pixel_keep.to(torch.uint8).contiguous()
    check(L.dcfp_upsample_ce_fwd_f32(_p(logits), _p(labels), _p(pixel_keep), int(ignore_index), N, Cc,
                                     h, w, H, W, int(bool(align_corners)), _p(lse), _p(gtp), _p(out2),
                                     _p(ws), ws.numel(), _stream()), "upsample_ce_fwd")
    return out2, lse, gtp


class UpsampleCEFn(torch.autograd.Function):
    """loss = CrossEntropyLoss(ignore_index, 'mean')(F.interpolate(logits, size), labels),
    fused (networks/deeplabv3.py:47,50 + loss/criterion.py:60)."""

    @staticmethod
    def forward(ctx, logits, labels, H, W, align_corners, ignore_index, pixel_keep):
        out2, lse, _ = upsample_ce_forward(logits, labels, (H, W), align_corners, ignore_index, pixel_keep)
        ctx.save_for_backward(logits, labels, lse, out2, pixel_keep)
        ctx.cfg = (H, W, int(bool(align_corners)), int(ignore_index))
        return out2[0] / out2[1]

    @staticmethod
    def backward(ctx, gout):
        logits, labels, lse, out2, pixel_keep = ctx.saved_tensors
        H, W, ac, ignore = ctx.cfg
        logits = logits.contiguous()
        N, Cc, h, w = logits.shape
        scale = (gout / out2[1]).reshape(1).to(torch.float32).contiguous()
        dl = torch.empty_like(logits)
        check(_lib.lib().dcfp_upsample_ce_bwd_f32(_p(logits), _p(labels.contiguous()), _p(pixel_keep),
                                                  ignore, N, Cc, h, w, H, W, ac, _p(lse), _p(scale),
                                                  _p(dl), _stream()), "upsample_ce_bwd")
        return dl, None, None, None, None, None, None


def upsample_cross_entropy(logits, labels, size, align_corners, ignore_index=255, pixel_keep=None):
    if pixel_keep is not None:
        pixel_keep = pixel_keep.to(torch.uint8).contiguous()
    return UpsampleCEFn.apply(logits, labels, int(size[0]), int(size[1]), align_corners,
                              ignore_index, pixel_keep)


CE_BACKWARD_VARIANTS = ("cells19", "cells_chunked", "per_output")


def ce_backward_plan(N, C_, h, w, H, W):
    """-> (variant, chunk_width, chunks): the kernel the fused upsample + CE backward (plain and weighted) launches at
    this shape; variant is one of CE_BACKWARD_VARIANTS (dcfp_upsample_ce_bwd_plan)."""
    v, ct, n = C.c_int(-1), C.c_int(0), C.c_int(0)
    check(_lib.lib().dcfp_upsample_ce_bwd_plan(int(N), int(C_), int(h), int(w), int(H), int(W), C.byref(v),
                                               C.byref(ct), C.byref(n)), "upsample_ce_bwd_plan")
    return CE_BACKWARD_VARIANTS[v.value], ct.value, n.value


# ------------------------------------------------------------------ GSRL pieces
def upsample_margin(logits, size, align_corners):
    """p1 - p2 of softmax(F.interpolate(logits, size)) per pixel, [N,H,W]."""
    _require(logits, "logits")
    logits = logits.contiguous()
    N, Cc, h, w = logits.shape
    H, W = int(size[0]), int(size[1])
    out = torch.empty((N, H, W), dtype=torch.float32, device=logits.device)
    check(_lib.lib().dcfp_upsample_margin_f32(_p(logits), N, Cc, h, w, H, W, int(bool(align_corners)),
                                              _p(out), _stream()), "upsample_margin")
    return out


def maxfilter2d(x, k):
    """F.max_pool2d(x[:,None], k, stride=1, padding=k//2)[:,0] for a [N,H,W] map."""
    _require(x, "x")
    x = x.contiguous()
    N, H, W = x.shape
    y = torch.empty_like(x)
    check(_lib.lib().dcfp_maxfilter2d_s1_f32(_p(x), _p(y), N, H, W, int(k), _stream()), "maxfilter2d")
    return y


class UpsampleWCEFn(torch.autograd.Function):
    """Per-image (sum w*CE, sum w) of the bilinearly upsampled logits with per-pixel weights w
    (loss/criterion.py:94-99), fused like UpsampleCEFn."""

    @staticmethod
    def forward(ctx, logits, labels, pix_weight, H, W, align_corners, ignore_index):
        _require(logits, "logits"); _require(pix_weight, "pix_weight")
        logits = logits.contiguous(); labels = labels.contiguous(); pix_weight = pix_weight.contiguous()
        N, Cc, h, w = logits.shape
        L = _lib.lib()
        ws = _workspace("wce", L.dcfp_upsample_wce_workspace_bytes(N, H, W), logits.device)
        lse = torch.empty((N, H, W), dtype=torch.float32, device=logits.device)
        out = torch.empty((N, 2), dtype=torch.float32, device=logits.device)
        check(L.dcfp_upsample_wce_fwd_f32(_p(logits), _p(labels), _p(pix_weight), int(ignore_index), N, Cc,
                                          h, w, H, W, int(bool(align_corners)), _p(lse), _p(out), _p(ws),
                                          ws.numel(), _stream()), "upsample_wce_fwd")
        ctx.save_for_backward(logits, labels, pix_weight, lse)
        ctx.cfg = (H, W, int(bool(align_corners)), int(ignore_index))
        return out

    @staticmethod
    def backward(ctx, gout):
        logits, labels, pix_weight, lse = ctx.saved_tensors
        H, W, ac, ignore = ctx.cfg
        N, Cc, h, w = logits.shape
        gs = gout[:, 0].contiguous().to(torch.float32)
        dl = torch.empty_like(logits)
        check(_lib.lib().dcfp_upsample_wce_bwd_f32(_p(logits), _p(labels), _p(pix_weight), ignore, N, Cc, h, w,
                                                   H, W, ac, _p(lse), _p(gs), _p(dl), _stream()),
              "upsample_wce_bwd")
        return dl, None, None, None, None, None, None


def upsample_weighted_ce(logits, labels, pix_weight, size, align_corners, ignore_index=255):
    return UpsampleWCEFn.apply(logits, labels, pix_weight, int(size[0]), int(size[1]), align_corners,
                               ignore_index)


# ------------------------------------------------------------------ knowledge distillation
KD_MODES = {"pixel": 0, "channel": 1}      # DCFP_KD_PIXEL / DCFP_KD_CHANNEL of include/dcfp_hip.h


class KDLossFn(torch.autograd.Function):
    """T^2-scaled KL(teacher || student) of the temperature-softened logits (kd.hip): over the classes at
    every pixel ("pixel") or over the positions of every (n, c) plane ("channel").  The forward launch also writes
    dL/dstudent, so backward is grad_output x that tensor; the teacher gets no gradient."""

    @staticmethod
    def forward(ctx, student, teacher, T, mode):
        s, t = student.contiguous(), teacher.contiguous()
        N, Cc, h, w = s.shape
        L = _lib.lib()
        ws = _workspace("kd", L.dcfp_kd_workspace_bytes(mode, N, Cc, h, w), s.device)
        out = torch.empty(1, dtype=torch.float32, device=s.device)
        dl = torch.empty_like(s) if ctx.needs_input_grad[0] else None
        check(L.dcfp_kd_fwd_f32(_p(s), _p(t), mode, N, Cc, h, w, T, _p(ws), ws.numel(), _p(out), _p(dl), _stream()),
              "kd_fwd")
        ctx.save_for_backward(dl)
        return out.reshape(())

    @staticmethod
    def backward(ctx, gout):
        dl, = ctx.saved_tensors
        return dl * gout, None, None, None


def kd_loss(student, teacher, T=1.0, mode="pixel"):
    """Distillation loss between the fp32 [N,C,h,w] logits of a student and a frozen teacher, a 0-dim tensor:
         pixel:    T^2/(N h w) * sum_pixels KL(softmax_c(teacher/T) || softmax_c(student/T))
         channel:  T^2/(N C)   * sum_planes KL(softmax_yx(teacher/T) || softmax_yx(student/T))
    The gradient goes to `student` only; a teacher that requires grad is an error (detach it)."""
    _require(student, "student")
    _require(teacher, "teacher")
    if teacher.requires_grad:
        raise RuntimeError("kd_loss: the teacher's logits must not require grad (run the teacher under no_grad)")
    if student.dim() != 4 or tuple(student.shape) != tuple(teacher.shape):
        raise RuntimeError(f"kd_loss: student {tuple(student.shape)} and teacher {tuple(teacher.shape)} must be the "
                           "same [N,C,h,w]")
    if student.device != teacher.device:
        raise RuntimeError(f"kd_loss: student on {student.device}, teacher on {teacher.device}")
    if mode not in KD_MODES:
        raise ValueError(f"kd_loss: mode {mode!r} is not one of {sorted(KD_MODES)}")
    T = float(T)
    if not (T > 0.0 and T != float("inf")):
        raise ValueError(f"kd_loss: the temperature must be a finite positive number, got {T}")
    return KDLossFn.apply(student, teacher, T, KD_MODES[mode])


# ------------------------------------------------------------------ pair-wise similarity distillation
PA_F32_NCHW, PA_F16_NHWC = 0, 1            # DCFP_PA_F32_NCHW / DCFP_PA_F16_NHWC of include/dcfp_hip.h


class PairwiseKDFn(torch.autograd.Function):
    """Mean squared difference of the student's and the teacher's node-similarity matrices (pairwise.hip).
    When a gradient is wanted the forward call leaves the student's node matrix and the difference matrix in a workspace
    of its own, which the graph keeps; backward runs the gradient kernels on it with grad_output as their last factor
    and writes dL/dstudent once.  A loss-only call uses the shared scratch.  The teacher gets no gradient."""

    @staticmethod
    def forward(ctx, student, teacher, layout, pitch, Ct, pool):
        s = student.contiguous()
        N, Cs, h, w = s.shape
        L = _lib.lib()
        want = ctx.needs_input_grad[0]
        nbytes = L.dcfp_pairwise_workspace_bytes(N, Cs, Ct, h, w, pool, int(want))
        if nbytes == 0:
            raise RuntimeError(f"pairwise_kd_loss: student {tuple(s.shape)} with pool {pool} is beyond the kernels' "
                               "launch limits")
        if want:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
        else:
            ws = _workspace("pairwise", nbytes, s.device)
        out = torch.empty(1, dtype=torch.float32, device=s.device)
        check(L.dcfp_pairwise_fwd_f32(_p(s), _p(teacher), layout, pitch, N, Cs, Ct, h, w, pool, _p(ws), ws.numel(),
                                      _p(out), int(want), _stream()), "pairwise_fwd")
        ctx.save_for_backward(ws if want else None)
        ctx.cfg = (N, Cs, Ct, h, w, pool)
        return out.reshape(())

    @staticmethod
    def backward(ctx, gout):
        ws, = ctx.saved_tensors
        N, Cs, Ct, h, w, pool = ctx.cfg
        g = gout.to(torch.float32).contiguous()
        ds = torch.empty((N, Cs, h, w), dtype=torch.float32, device=ws.device)
        check(_lib.lib().dcfp_pairwise_bwd_f32(N, Cs, Ct, h, w, pool, _p(ws), ws.numel(), _p(g), _p(ds), _stream()),
              "pairwise_bwd")
        return ds, None, None, None, None, None


def pairwise_kd_loss(student, teacher, pool=2, teacher_channels=None):
    """Pair-wise similarity distillation (Liu et al. 2019) between a feature map of the student, fp32 [N,Cs,h,w], and
    of a frozen teacher over the same N, h, w, a 0-dim fp32 tensor:  nodes are the means of the pool x pool windows
    (avg_pool2d with ceil_mode, count_include_pad False), normalised over the channels (a node with squared norm
    <= 1e-12 is dead: zero, no gradient);  L = 1/(N P^2) * sum (f^S_p . f^S_q - f^T_p . f^T_q)^2 over images and node
    pairs.  The teacher is fp32 [N,Ct,h,w] or, as a deploy.Engine holds it, fp16 [N,h,w,pitch] with unit stride in the
    last dimension, of which the first `teacher_channels` (default: all) are read; Ct need not equal Cs.  The gradient
    goes to `student` only; a teacher that requires grad is an error (detach it)."""
    _require(student, "student")
    if not isinstance(teacher, torch.Tensor) or not teacher.is_cuda:
        raise RuntimeError("dcfp_amd: teacher must be a CUDA/HIP tensor (no CPU fallback exists)")
    if teacher.requires_grad:
        raise RuntimeError("pairwise_kd_loss: the teacher's feature must not require grad (run the teacher under no_grad)")
    if isinstance(pool, bool) or not isinstance(pool, int) or pool < 1:
        raise ValueError(f"pairwise_kd_loss: pool must be an int >= 1, got {pool!r}")
    if student.dim() != 4 or teacher.dim() != 4:
        raise RuntimeError(f"pairwise_kd_loss: student {tuple(student.shape)} and teacher {tuple(teacher.shape)} must be "
                           "4-dimensional")
    if student.device != teacher.device:
        raise RuntimeError(f"pairwise_kd_loss: student on {student.device}, teacher on {teacher.device}")
    N, _, h, w = student.shape
    if teacher.dtype == torch.float32:
        if teacher_channels is not None and int(teacher_channels) != teacher.shape[1]:
            raise ValueError(f"pairwise_kd_loss: teacher_channels {teacher_channels} on an fp32 teacher of "
                             f"{teacher.shape[1]} channels")
        nhw, Ct, layout, pitch = (teacher.shape[0], teacher.shape[2], teacher.shape[3]), teacher.shape[1], PA_F32_NCHW, 0
        teacher = teacher.contiguous()
    elif teacher.dtype == torch.float16:
        nhw, width = tuple(teacher.shape[:3]), teacher.shape[3]
        if nhw != (N, h, w):
            raise RuntimeError(f"pairwise_kd_loss: student {tuple(student.shape)} [N,C,h,w] and teacher "
                               f"{tuple(teacher.shape)} [N,h,w,pitch] must cover the same N, h, w")
        Ct = width if teacher_channels is None else int(teacher_channels)
        if not 1 <= Ct <= width:
            raise ValueError(f"pairwise_kd_loss: teacher_channels {teacher_channels} of a {width}-channel wide teacher")
        st = teacher.stride()                # (the stride of a dimension of size 1 says nothing)
        pitch = st[2] if w > 1 else st[1] if h > 1 else st[0] if N > 1 else width
        if not ((width == 1 or st[3] == 1) and pitch >= width and (h == 1 or st[1] == w * pitch)
                and (N == 1 or st[0] == h * w * pitch)):
            raise RuntimeError("pairwise_kd_loss: an fp16 teacher is [N,h,w,pitch] with unit stride in the last dimension "
                               f"and dense pixels, got strides {tuple(teacher.stride())}")
        layout = PA_F16_NHWC
    else:
        raise RuntimeError(f"dcfp_amd: teacher must be float32 [N,C,h,w] or float16 [N,h,w,pitch], got {teacher.dtype}")
    if nhw != (N, h, w):
        raise RuntimeError(f"pairwise_kd_loss: student {tuple(student.shape)} and teacher {tuple(teacher.shape)} must "
                           "cover the same N, h, w")
    return PairwiseKDFn.apply(student, teacher, layout, int(pitch), int(Ct), pool)


# ------------------------------------------------------------------ Lovasz-Softmax
LOVASZ_Q = 20                              # errors are quantised to q = round(e * 2^20) (csrc/lovasz.hip)
LOVASZ_BINS = (64, 128, 256, 512, 1024, 2048, 4096)


def _lovasz_args(name, logits, labels, size, bins):
    _require(logits, "logits")
    if logits.dim() != 4:
        raise RuntimeError(f"{name}: logits must be [N,C,h,w], got {tuple(logits.shape)}")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or not labels.is_cuda:
        raise RuntimeError(f"{name}: labels must be a CUDA int64 tensor [N,H,W]")
    if labels.device != logits.device:
        raise RuntimeError(f"{name}: logits on {logits.device}, labels on {labels.device}")
    N, Cc, h, w = logits.shape
    H, W = int(size[0]), int(size[1])
    if tuple(labels.shape) != (N, H, W):
        raise RuntimeError(f"{name}: labels shape {tuple(labels.shape)} != {(N, H, W)}")
    if bins not in LOVASZ_BINS:
        raise ValueError(f"{name}: bins must be a power of two in 64 .. 4096, got {bins!r}")
    if Cc > 255:
        raise ValueError(f"{name}: at most 255 classes, got {Cc}")
    return N, Cc, h, w, H, W


def _lovasz_hist(logits, labels, N, Cc, h, w, H, W, ac, ignore_index, bins):
    """-> (lse [N,H,W], workspace that holds the histogram): dcfp_lovasz_hist_f32 on contiguous inputs"""
    L = _lib.lib()
    ws = _workspace("lovasz", L.dcfp_lovasz_workspace_bytes(Cc, bins), logits.device)
    lse = torch.empty((N, H, W), dtype=torch.float32, device=logits.device)
    check(L.dcfp_lovasz_hist_f32(_p(logits), _p(labels), int(ignore_index), N, Cc, h, w, H, W, ac, bins, _p(lse),
                                 _p(ws), ws.numel(), _stream()), "lovasz_hist")
    return lse, ws


class LovaszSoftmaxFn(torch.autograd.Function):
    """Lovasz-Softmax loss of the bilinearly upsampled logits over the classes present in the labels (lovasz.hip,
    DESIGN §18).  Forward keeps the per-pixel log-sum-exp and the weight table [C, bins, 2]; the table is this node's
    own tensor, the histogram workspace is free for the next call as soon as forward returns."""

    @staticmethod
    def forward(ctx, logits, labels, H, W, align_corners, ignore_index, bins):
        logits, labels = logits.contiguous(), labels.contiguous()
        N, Cc, h, w = logits.shape
        ac = int(bool(align_corners))
        lse, ws = _lovasz_hist(logits, labels, N, Cc, h, w, H, W, ac, ignore_index, bins)
        out = torch.empty(1, dtype=torch.float32, device=logits.device)
        table = torch.empty((Cc, bins, 2), dtype=torch.float32, device=logits.device)
        check(_lib.lib().dcfp_lovasz_scan_f32(Cc, bins, _p(ws), ws.numel(), _p(out), _p(table), _stream()),
              "lovasz_scan")
        ctx.save_for_backward(logits, labels, lse, table)
        ctx.cfg = (H, W, ac, int(ignore_index), bins)
        return out.reshape(())

    @staticmethod
    def backward(ctx, gout):
        logits, labels, lse, table = ctx.saved_tensors
        H, W, ac, ignore, bins = ctx.cfg
        N, Cc, h, w = logits.shape
        scale = gout.reshape(1).to(torch.float32).contiguous()
        asum = torch.empty_like(lse)
        dl = torch.empty_like(logits)
        check(_lib.lib().dcfp_lovasz_bwd_f32(_p(logits), _p(labels), ignore, N, Cc, h, w, H, W, ac, bins, _p(lse),
                                             _p(table), _p(scale), _p(asum), _p(dl), _stream()), "lovasz_bwd")
        return dl, None, None, None, None, None, None


def lovasz_softmax(logits, labels, size, align_corners, ignore_index=255, bins=1024):
    """Lovasz-Softmax loss (Berman et al. 2018, classes='present') of softmax(F.interpolate(logits, size)) against
    `labels`, a 0-dim tensor.  logits fp32 [N,C,h,w], labels int64 [N,H,W]; a pixel counts when its label is a class
    and not ignore_index.  Errors are quantised to 2^-20 and binned into `bins` bins instead of sorted: the loss lies
    within [L - 1/bins - 2^-21, L + 2^-21] of the exact loss L, two calls give the same bits, and nothing of size
    N x C x H x W is allocated.  No class present: 0, with a zero gradient."""
    N, Cc, h, w, H, W = _lovasz_args("lovasz_softmax", logits, labels, size, bins)
    return LovaszSoftmaxFn.apply(logits, labels, H, W, align_corners, int(ignore_index), int(bins))


def lovasz_histogram(logits, labels, size, align_corners, ignore_index=255, bins=1024):
    """-> (nF, nB, SF, SB), each [C, bins]: per class and error bin the number of foreground / background pixels (int32)
    and the sums of their quantised errors q (int64) - what lovasz_softmax scans."""
    N, Cc, h, w, H, W = _lovasz_args("lovasz_histogram", logits, labels, size, bins)
    _, ws = _lovasz_hist(logits.detach().contiguous(), labels.contiguous(), N, Cc, h, w, H, W,
                         int(bool(align_corners)), ignore_index, int(bins))
    cb = Cc * bins
    sums = ws[:16 * cb].view(torch.int64).reshape(2, Cc, bins).clone()
    counts = ws[16 * cb:24 * cb].view(torch.int32).reshape(2, Cc, bins).clone()
    return counts[0], counts[1], sums[0], sums[1]


def lovasz_errors(logits, labels, size, align_corners, ignore_index=255):
    """-> q [N,C,H,W]: the quantised error min(2^20, floor(e * 2^20 + 0.5)) of every pixel and class, e = 1 - p for the
    label's class and p otherwise, as int64; 0xFFFFFFFF where the pixel does not count.  For tests and for a look at the
    error distribution: it writes N x C x H x W values and has no place in a training step."""
    N, Cc, h, w, H, W = _lovasz_args("lovasz_errors", logits, labels, size, LOVASZ_BINS[0])
    out = torch.empty((N, Cc, H, W), dtype=torch.int32, device=logits.device)
    logits, labels = logits.detach().contiguous(), labels.contiguous()
    check(_lib.lib().dcfp_lovasz_errors_u32(_p(logits), _p(labels), int(ignore_index), N, Cc, h, w, H, W,
                                            int(bool(align_corners)), _p(out), _stream()), "lovasz_errors")
    return out.to(torch.int64) & 0xFFFFFFFF


# ------------------------------------------------------------------ inference / evaluation
def conv2d_fused_infer(x, w, scale, shift, stride=1, pad=0, dil=1, residual=None, relu=False):
    """y = act(conv(x,w)*scale[co] + shift[co] (+ residual)): conv with an eval-mode BatchNorm
    folded into its epilogue (no autograd: inference only)."""
    _require(x, "x"); _require(w, "weight")
    x = x.contiguous(); w = w.contiguous()
    d = _desc(x.shape, w.shape, stride, pad, dil)
    y = torch.empty((d.N, d.Cout, d.Hout, d.Wout), dtype=torch.float32, device=x.device)
    fused = "fused" + _grid_variant(_on_grid(x, d.Cin * d.H * d.W), True, d.Cin * d.H * d.W)
    if residual is not None:
        residual = residual.contiguous()
        if tuple(residual.shape) != tuple(y.shape):
            raise RuntimeError("conv2d_fused_infer: residual shape mismatch")
    L = _lib.lib()
    if L.dcfp_conv2d_workspace_is_scratch(C.byref(d), _lib.CONV_FWD):
        ws, valid = _workspace("conv_scratch", L.dcfp_conv2d_workspace_bytes(C.byref(d), _lib.CONV_FWD), x.device), 0
    else:
        ws, valid = _wp_buffer(w, _lib.CONV_FWD, d, L.dcfp_conv2d_workspace_bytes(C.byref(d), _lib.CONV_FWD), fused)
    check(L.dcfp_conv2d_fwd_fused_f32_nchw(C.byref(d), _p(x), _p(w), _p(scale.contiguous()),
                                           _p(shift.contiguous()), _p(residual), int(bool(relu)), _p(y),
                                           _p(ws), ws.numel(), valid, _stream()), "conv2d_fwd_fused")
    return y


def upsample_argmax(logits, size, align_corners):
    """argmax over classes of F.interpolate(logits, size) per pixel -> int32 [N,H,W]."""
    _require(logits, "logits")
    logits = logits.contiguous()
    N, Cc, h, w = logits.shape
    H, W = int(size[0]), int(size[1])
    pred = torch.empty((N, H, W), dtype=torch.int32, device=logits.device)
    check(_lib.lib().dcfp_upsample_argmax_f32(_p(logits), N, Cc, h, w, H, W, int(bool(align_corners)),
                                              _p(pred), _stream()), "upsample_argmax")
    return pred


def confusion_matrix(pred, gt, num_classes, ignore_index=255, out=None):
    """conf[gt, pred] += 1 over pixels with gt != ignore (evaluate.py:229-247); int64 [C,C]."""
    if pred.dtype != torch.int32 or gt.dtype != torch.int64 or not pred.is_cuda or not gt.is_cuda:
        raise RuntimeError("confusion_matrix: pred int32 / gt int64 CUDA tensors expected")
    pred = pred.contiguous(); gt = gt.contiguous()
    if out is None:
        out = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=pred.device)
    check(_lib.lib().dcfp_confusion_matrix_i64(_p(pred), _p(gt), int(ignore_index), pred.numel(),
                                               int(num_classes), _p(out), _stream()), "confusion_matrix")
    return out


VOTE_MAX_MAPS = 16


def _fused_vote(name, entry, items, limit, what, layout, records, grid_hw, out_hw, align_corners, labels, conf,
                want_scores, want_pred, ignore_index):
    """What multiscale_vote and sliding_vote share: every check but those on a pass's own record, the outputs and the
    launch.  items: the maps / passes (at most `limit`), logits first, of shape `layout` (N, C in front of the last two
    dimensions); records(items, dev, N, C) checks them and returns a callable that gives, on the logits' device, the
    arguments of the C entry `entry` in front of N (it keeps the tensors they point to alive)."""
    items = list(items)
    if not 1 <= len(items) <= limit:
        raise RuntimeError("%s: 1 .. %d %s expected, got %d" % (name, limit, what, len(items)))
    H, W = int(grid_hw[0]), int(grid_hw[1])
    oh, ow = int(out_hw[0]), int(out_hw[1])
    first = items[0][0]
    _require(first, "logits")
    dims = layout.count(",") + 1
    if first.dim() != dims:
        raise RuntimeError("%s: logits %s expected" % (name, layout))
    dev, (N, Cc) = first.device, first.shape[dims - 4:dims - 2]
    if not (0 < oh <= H and 0 < ow <= W):
        raise RuntimeError("%s: the output %dx%d must be a crop of the grid %dx%d" % (name, oh, ow, H, W))
    lead = records(items, dev, N, Cc)
    if (conf is None) != (labels is None):
        raise RuntimeError("%s: labels and the confusion matrix come together" % name)
    if labels is not None:
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.device == dev and
                labels.dtype == torch.int64 and tuple(labels.shape) == (N, oh, ow) and labels.is_contiguous()):
            raise RuntimeError("%s: dense int64 [N,out_h,out_w] device labels expected" % name)
        if not (isinstance(conf, torch.Tensor) and conf.is_cuda and conf.device == dev and conf.dtype == torch.int64 and
                tuple(conf.shape) == (Cc, Cc) and conf.is_contiguous()):
            raise RuntimeError("%s: conf must be a contiguous int64 [C,C] device tensor" % name)
    if not (want_scores or want_pred or labels is not None):
        raise RuntimeError("%s: nothing asked for" % name)
    with torch.cuda.device(dev):
        head = lead()          # (lead stays bound: it keeps the records' tensors alive over the launch)
        scores = torch.empty((N, Cc, oh, ow), dtype=torch.float32, device=dev) if want_scores else None
        pred = torch.empty((N, oh, ow), dtype=torch.int32, device=dev) if want_pred else None
        check(getattr(_lib.lib(), entry)(*head, N, Cc, H, W, oh, ow, int(bool(align_corners)), _p(scores), _p(pred),
                                         _p(labels), int(ignore_index), _p(conf), _stream()), name)
    return pred, scores


def multiscale_vote(maps, grid_hw, out_hw, align_corners, labels=None, conf=None, want_scores=False, want_pred=True,
                    ignore_index=255):
    """The multi-scale + flip vote of evaluate.py:198-227 (whole=True) in one launch (csrc/vote.hip).
    maps: up to 16 tuples (logits fp32 [N,C,h,w], (hs, ws), flip, weight) - the low-resolution logits of the network
    on the image resized to hs x ws (mirrored along x when flip); grid_hw: the size (H, W) the reference resizes every
    pass back to; out_hw: the top-left crop of that grid that is produced.  labels int64 [N,out_h,out_w] and conf int64
    [C,C] (accumulated, given together) count the confusion matrix in the same launch.  -> (pred int32 [N,out_h,out_w] or None, scores
    fp32 [N,C,out_h,out_w] or None).  The N x C x hs x ws logits are never formed."""
    def records(maps, dev, N, Cc):
        recs, keep = (_lib.VoteMap * len(maps))(), []
        for i, (logits, (hs, ws), flip, weight) in enumerate(maps):
            _require(logits, "logits")
            if logits.dim() != 4 or tuple(logits.shape[:2]) != (N, Cc) or logits.device != dev:
                raise RuntimeError("multiscale_vote: every map holds [N,C,h,w] logits of one batch on one device")
            logits = logits.contiguous()
            keep.append(logits)
            recs[i] = _lib.VoteMap(logits.data_ptr(), logits.shape[2], logits.shape[3], int(hs), int(ws),
                                   int(bool(flip)), float(weight))
        return lambda: (recs, len(keep))
    return _fused_vote("multiscale_vote", "dcfp_vote_multiscale_f32", maps, VOTE_MAX_MAPS, "maps", "[N,C,h,w]",
                       records, grid_hw, out_hw, align_corners, labels, conf, want_scores, want_pred, ignore_index)


SLIDE_MAX_PASSES, SLIDE_MAX_TILES_PER_AXIS = _lib.SLIDE_MAX_PASSES, _lib.SLIDE_MAX_TILES_PER_AXIS
_SLIDE_TABLES, _SLIDE_TABLES_KEPT = {}, 1024


def _origins(name, v, what):
    v = [int(o) for o in v]
    if not 1 <= len(v) <= SLIDE_MAX_TILES_PER_AXIS:
        raise RuntimeError("%s: 1 .. %d tile %s expected, got %d" % (name, SLIDE_MAX_TILES_PER_AXIS, what, len(v)))
    return v


def gather_tiles(image, ys, xs, tile_size, flip=False):
    """All len(ys) * len(xs) zero-padded tiles of image fp32 [N,ch,h,w] in one launch (csrc/slide.hip): tile
    t = r * len(xs) + c is image[:, :, ys[r]:ys[r]+th, xs[c]:xs[c]+tw], cut at the image border and padded with zeros at
    the bottom / right (evaluate.pad).  flip: the tiles of torch.flip(image, [3]), which is never formed.
    -> fp32 [T,N,ch,th,tw]."""
    _require(image, "image")
    if image.dim() != 4:
        raise RuntimeError("gather_tiles: image [N,ch,h,w] expected")
    image = image.contiguous()
    ys, xs = _origins("gather_tiles", ys, "rows"), _origins("gather_tiles", xs, "columns")
    th, tw = int(tile_size[0]), int(tile_size[1])
    N, ch, h, w = image.shape
    tiles = torch.empty((len(ys) * len(xs), N, ch, th, tw), dtype=torch.float32, device=image.device)
    with torch.cuda.device(image.device):
        check(_lib.lib().dcfp_gather_tiles_f32(_p(image), N, ch, h, w, (C.c_int32 * len(ys))(*ys), len(ys),
                                               (C.c_int32 * len(xs))(*xs), len(xs), th, tw, int(bool(flip)), _p(tiles),
                                               _stream()), "gather_tiles")
    return tiles


def _slide_table(geometry, device):
    """The origin table of a vote's passes, (host ctypes array, device int32 tensor of a few KB), kept per geometry,
    device and stream: a call with a geometry seen before neither allocates nor copies, a new one (every new image size
    of a dataset without a common size) costs one small host-to-device copy.  Keyed by the stream like _workspace, so
    that the table is allocated on the stream that reads it and the allocator orders the reuse of an evicted one."""
    key = (device.index, torch.cuda.current_stream().cuda_stream, geometry)
    hit = _SLIDE_TABLES.get(key)
    if hit is None:
        stride = 2 * SLIDE_MAX_TILES_PER_AXIS
        flat = [0] * (stride * len(geometry))
        for k, (ys, xs) in enumerate(geometry):
            flat[k * stride:k * stride + len(ys)] = ys
            flat[k * stride + SLIDE_MAX_TILES_PER_AXIS:k * stride + SLIDE_MAX_TILES_PER_AXIS + len(xs)] = xs
        if len(_SLIDE_TABLES) >= _SLIDE_TABLES_KEPT:       # (a dataset of many image sizes: the oldest one goes)
            del _SLIDE_TABLES[next(iter(_SLIDE_TABLES))]
        hit = _SLIDE_TABLES[key] = ((C.c_int32 * len(flat))(*flat), torch.tensor(flat, dtype=torch.int32, device=device))
    return hit


def sliding_vote(passes, grid_hw, out_hw, align_corners, labels=None, conf=None, want_scores=False, want_pred=True,
                 ignore_index=255):
    """The multi-scale + flip vote of evaluate.py:198-227 with whole=False (sliding-window tiles) in one launch (DESIGN
    §12, csrc/slide.hip).  passes: up to 16 tuples (logits fp32 [T,N,C,lh,lw], (hs, ws), (th, tw), ys, xs, flip, weight):
    the low-resolution logits of the network on each of the T = len(ys) * len(xs) padded th x tw tiles (row-major;
    evaluate.sliding_tiles) of the image resized to hs x ws, mirrored along x when flip.  Everything else as
    multiscale_vote.  -> (pred int32 [N,out_h,out_w] or None, scores fp32 [N,C,out_h,out_w] or None).  Neither the
    upsampled tiles nor the N x C x hs x ws accumulator are ever formed."""
    def records(passes, dev, N, Cc):
        recs, keep, geometry = (_lib.SlidePass * len(passes))(), [], []
        for i, (logits, (hs, ws), (th, tw), ys, xs, flip, weight) in enumerate(passes):
            _require(logits, "logits")
            ys, xs = _origins("sliding_vote", ys, "rows"), _origins("sliding_vote", xs, "columns")
            if logits.dim() != 5 or tuple(logits.shape[:3]) != (len(ys) * len(xs), N, Cc) or logits.device != dev:
                raise RuntimeError("sliding_vote: every pass holds [rows*cols,N,C,lh,lw] logits of one batch on one "
                                   "device")
            logits = logits.contiguous()
            keep.append(logits)
            geometry.append((tuple(ys), tuple(xs)))
            recs[i] = _lib.SlidePass(logits.data_ptr(), logits.shape[3], logits.shape[4], int(hs), int(ws), int(th),
                                     int(tw), len(ys), len(xs), int(bool(flip)), float(weight))

        def lead():
            host, table = _slide_table(tuple(geometry), dev)
            return recs, len(keep), host, _p(table)
        return lead
    return _fused_vote("sliding_vote", "dcfp_vote_sliding_f32", passes, SLIDE_MAX_PASSES, "passes",
                       "[T,N,C,lh,lw]", records, grid_hw, out_hw, align_corners, labels, conf, want_scores, want_pred,
                       ignore_index)


def label_boundary(labels, num_classes, d, background=255):
    """The label map with everything but the class boundaries set to `background`: a pixel with
    0 <= label < num_classes keeps its label unless the whole (2d+1)x(2d+1) window centred on it lies inside the
    image and carries that label.  int32 / int64 [H,W] or [N,H,W] -> a new tensor of the same shape and dtype."""
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise RuntimeError("dcfp_amd: labels must be a CUDA/HIP tensor (no CPU fallback exists)")
    if labels.dtype not in (torch.int32, torch.int64) or labels.dim() not in (2, 3):
        raise RuntimeError("label_boundary: int32 / int64 [H,W] or [N,H,W] labels expected")
    src = labels.contiguous()
    N = src.shape[0] if src.dim() == 3 else 1
    H, W = src.shape[-2:]
    out = torch.empty_like(src)
    L = _lib.lib()
    ws = _workspace("label_boundary", L.dcfp_label_boundary_workspace_bytes(N, H, W), src.device)
    fn = L.dcfp_label_boundary_i32 if src.dtype == torch.int32 else L.dcfp_label_boundary_i64
    check(fn(_p(src), _p(out), N, H, W, int(num_classes), int(d), int(background), _p(ws), ws.numel(), _stream()),
          "label_boundary")
    return out


def png_deflate_bound(H, W):
    """The largest size in bytes of one stream of png_deflate_labels for an H x W map (host only)."""
    return int(_lib.lib().dcfp_png_deflate_bound(int(H), int(W)))


def png_deflate_labels(pred, luts=None):
    """Finished zlib streams of the 8-bit PNGs of a prediction: pred int32 [N,H,W], luts uint8 [P,256]
    (1 <= P <= 4; None: the identity table) -> (streams, offsets, lengths): stream n*P + p, the image
    luts[p][pred[n] & 255], is streams[offsets[s] : offsets[s] + lengths[s]]; streams is a uint8 device buffer (a
    workspace: the next call on the stream overwrites it), offsets and lengths are int64 [N*P] device tensors.  The
    streams lie one after the other from 0 on, so sum(lengths) bytes hold them all."""
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        raise RuntimeError("dcfp_amd: pred must be a CUDA/HIP tensor (no CPU fallback exists)")
    if pred.dtype != torch.int32 or pred.dim() != 3 or not pred.is_contiguous():
        raise RuntimeError("png_deflate_labels: a contiguous int32 [N,H,W] prediction expected")
    if luts is None:
        luts = torch.arange(256, dtype=torch.uint8, device=pred.device).reshape(1, 256)
    if not (isinstance(luts, torch.Tensor) and luts.is_cuda and luts.device == pred.device and luts.dtype == torch.uint8
            and luts.dim() == 2 and luts.shape[1] == 256 and 1 <= luts.shape[0] <= 4 and luts.is_contiguous()):
        raise RuntimeError("png_deflate_labels: luts must be a contiguous uint8 [P,256] tensor on pred's device, "
                           "1 <= P <= 4")
    N, H, W = (int(v) for v in pred.shape)
    P = int(luts.shape[0])
    L = _lib.lib()
    bound = L.dcfp_png_deflate_bound(H, W)
    ws_bytes = L.dcfp_png_deflate_workspace_bytes(N, H, W, P)
    if N < 1 or bound == 0 or ws_bytes == 0:
        raise RuntimeError("png_deflate_labels: N >= 1, 1 <= H <= 4096, 1 <= W <= 8192 expected, got %s"
                           % (tuple(pred.shape),))
    out = _workspace("png_streams", N * P * bound, pred.device)
    ws = _workspace("png_rows", ws_bytes, pred.device)
    meta = torch.empty((2, N * P), dtype=torch.int64, device=pred.device)
    check(L.dcfp_png_deflate_labels_i32(_p(pred), N, H, W, _p(luts), P, _p(out), out.numel(), _p(meta[0]), _p(meta[1]),
                                        _p(ws), ws.numel(), _stream()), "png_deflate_labels")
    return out, meta[0], meta[1]


def augment_batch(images, labels, records, taps, lut_a, lut_b, id_table, crop_size, ignore_label=255):
    """The device half of the training augmentation (datasets.base builds its arguments).
    images: N uint8 [H,W,3] BGR tensors, labels: N uint8 [H,W] raw-id tensors or None, all on one device and dense;
    records: N tuples (col_off, row_off, lut_a_off, lut_b_off, hsv_flags, hue_delta, sat_alpha); taps int32 [T,4],
    lut_a uint8 [A] or None, lut_b float32 [B], id_table uint8 [256] or None: device tensors.
    -> (fp32 [N,3,ch,cw], int64 [N,ch,cw], int32 [N,256] histogram); the last two are None without labels."""
    N = len(images)
    ch, cw = int(crop_size[0]), int(crop_size[1])
    if N == 0 or len(records) != N or (labels is not None and len(labels) != N):
        raise RuntimeError("augment_batch: one record (and one label map) per image expected")
    dev = taps.device
    for t, dt in ((taps, torch.int32), (lut_b, torch.float32), (lut_a, torch.uint8), (id_table, torch.uint8)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise RuntimeError("dcfp_amd: the augmentation tables must be dense CUDA/HIP tensors (no CPU fallback exists)")
    if taps.dim() != 2 or taps.shape[1] != 4 or (id_table is not None and id_table.numel() != 256):
        raise RuntimeError("augment_batch: taps [T,4] and a 256-entry id table expected")
    recs = (_lib.AugSample * N)()
    for i, (img, r) in enumerate(zip(images, records)):
        lab = None if labels is None else labels[i]
        if not (img.is_cuda and img.device == dev and img.dtype == torch.uint8 and img.dim() == 3 and
                img.shape[2] == 3 and img.is_contiguous()):
            raise RuntimeError("augment_batch: dense uint8 [H,W,3] device images expected")
        if lab is not None and not (lab.device == dev and lab.dtype == torch.uint8 and lab.is_contiguous() and
                                    tuple(lab.shape) == tuple(img.shape[:2])):
            raise RuntimeError("augment_batch: dense uint8 [H,W] device label maps of the images' sizes expected")
        recs[i] = _lib.AugSample(img.data_ptr(), None if lab is None else lab.data_ptr(), img.shape[0], img.shape[1],
                                 int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5]), float(r[6]), 0)
    out = torch.empty((N, 3, ch, cw), dtype=torch.float32, device=dev)
    lab_out = hist = None
    if labels is not None:
        lab_out = torch.empty((N, ch, cw), dtype=torch.int64, device=dev)
        hist = torch.empty((N, 256), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().dcfp_augment_u8_to_f32_nchw(
            recs, N, ch, cw, _p(taps), taps.shape[0], _p(lut_a), 0 if lut_a is None else lut_a.numel(), _p(lut_b),
            lut_b.numel(), _p(id_table), int(ignore_label), _p(out), _p(lab_out), _p(hist), _stream()), "augment_batch")
    return out, lab_out, hist


def balance_weight(labels, hist, num_classes, balance, ignore_label=255, target_class=None, beta=0.9999):
    """get_label (Base.py:73-89) on the device: int64 [N,H,W] trainId labels + the int32 [N,256] histogram of
    augment_batch -> fp32 [N,H,W] class-balance weights (0 at ignore_label).  balance 1: 1/(n_c+1); balance 2:
    (1+1e-8-beta^n_t)/(1+1e-8-beta^n_c) with the per-sample int32 [N] target_class; both clipped to [0,1], in fp64."""
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda:
        raise RuntimeError("dcfp_amd: labels must be a CUDA/HIP tensor (no CPU fallback exists)")
    if balance not in (1, 2) or labels.dtype != torch.int64 or labels.dim() != 3 or not labels.is_contiguous() or \
            hist.dtype != torch.int32 or tuple(hist.shape) != (labels.shape[0], 256) or not hist.is_contiguous():
        raise RuntimeError("balance_weight: balance 1 or 2, dense int64 [N,H,W] labels and an int32 [N,256] histogram expected")
    if balance == 2:
        if target_class is None:
            raise RuntimeError("balance_weight: balance 2 needs the per-sample target class")
        target_class = torch.as_tensor(target_class, dtype=torch.int32).to(labels.device).contiguous()
        if target_class.numel() != labels.shape[0]:
            raise RuntimeError("balance_weight: one target class per sample expected")
    N = labels.shape[0]
    weight = torch.empty(labels.shape, dtype=torch.float32, device=labels.device)
    with torch.cuda.device(labels.device):
        check(_lib.lib().dcfp_balance_weight_f32(_p(labels), _p(hist), _p(target_class) if balance == 2 else None, N,
                                                 labels.shape[1] * labels.shape[2], int(num_classes), int(ignore_label),
                                                 int(balance), float(beta), _p(weight), _stream()), "balance_weight")
    return weight


class Components:
    """A labelled batch of `label_components`, left on the device.  Per sample s: `label_map(s)` int32
    [Hp,Wp] (the smallest linear index of the pixel's component, -1 background), `labels(s)` the ascending list of
    component labels and `component_sizes(s)` their pixel counts (both need `counts()`)."""

    def __init__(self, records, layout, work, counts):
        self.records, self.layout, self.work, self._counts_dev = records, layout, work, counts
        self.N = len(layout)
        self._i32 = work.view(torch.int32)
        self._counts = None

    def counts(self):
        """The N component counts on the host: the one synchronisation of a labelled batch."""
        if self._counts is None:
            self._counts = self._counts_dev.tolist()
        return self._counts

    def sizes(self, n):
        """Pixel count of component n[s] (1-based) of every sample, 0 where n[s] == 0: one gather, one copy."""
        n = [int(v) for v in n]
        if len(n) != self.N:
            raise RuntimeError("Components.sizes: one component number per sample expected")
        for v, c in zip(n, self.counts()):
            if not 0 <= v <= c:
                raise RuntimeError("Components.sizes: component %d of %d" % (v, c))
        at = torch.tensor([lay["sizes"] + max(v, 1) - 1 for v, lay in zip(n, self.layout)], dtype=torch.int64)
        got = self._i32[at.to(self.work.device)].tolist()
        return [g if v > 0 else 0 for g, v in zip(got, n)]

    def label_map(self, s):
        lay = self.layout[s]
        return self._i32[lay["base"]:lay["base"] + lay["Hp"] * lay["Wp"]].view(lay["Hp"], lay["Wp"])

    def labels(self, s):
        lay = self.layout[s]
        return self._i32[lay["roots"]:lay["roots"] + self.counts()[s]]

    def component_sizes(self, s):
        lay = self.layout[s]
        return self._i32[lay["sizes"]:lay["sizes"] + self.counts()[s]]


def label_components(labels, records, maps, id_table, ignore_label=255):
    """8-connected components of one class per sample on the scaled, padded label grid.
    labels: N dense uint8 [H,W] raw-id device tensors; records: N tuples (dst_h, dst_w, Hp, Wp, row_off, col_off, cls);
    maps: device int32 table holding every sample's nearest-neighbour row map [dst_h] at row_off and column map [dst_w]
    at col_off; id_table: uint8 [256] or None.  Pixel (y, x) of the Hp x Wp grid is foreground iff y < dst_h, x < dst_w
    and id_table[raw[row_map[y], col_map[x]]] == cls: the padding is background whatever `ignore_label` is (it is
    taken for the call shape of the reference's padding and only range-checked).  -> Components; nothing is
    synchronised here."""
    N = len(labels)
    if N == 0 or len(records) != N or not 0 <= int(ignore_label) <= 255:
        raise RuntimeError("label_components: one record per label map and an ignore label in 0..255 expected")
    if not (isinstance(maps, torch.Tensor) and maps.is_cuda and maps.dtype == torch.int32 and maps.is_contiguous()) or \
            (id_table is not None and not (id_table.is_cuda and id_table.dtype == torch.uint8 and
                                           id_table.numel() == 256 and id_table.is_contiguous())):
        raise RuntimeError("dcfp_amd: the component maps and id table must be dense CUDA/HIP tensors "
                           "(no CPU fallback exists)")
    dev = maps.device
    L = _lib.lib()
    recs = (_lib.CcSample * N)()
    layout, total = [], 0
    for i, (lab, r) in enumerate(zip(labels, records)):
        if not (isinstance(lab, torch.Tensor) and lab.is_cuda and lab.device == dev and lab.dtype == torch.uint8 and
                lab.dim() == 2 and lab.is_contiguous()):
            raise RuntimeError("label_components: dense uint8 [H,W] device label maps expected")
        dst_h, dst_w, Hp, Wp, row_off, col_off, cls = (int(v) for v in r)
        nbytes = L.dcfp_components_workspace_bytes(Hp, Wp)
        if nbytes == 0:
            raise RuntimeError("label_components: grid %dx%d is not supported" % (Hp, Wp))
        recs[i] = _lib.CcSample(lab.data_ptr(), lab.shape[0], lab.shape[1], dst_h, dst_w, Hp, Wp, row_off, col_off,
                                cls, 0, total)
        base, p8, cap4 = total // 4, (Hp * Wp + 7) & ~7, (((Hp + 1) // 2) * ((Wp + 1) // 2) + 3) & ~3
        layout.append({"Hp": Hp, "Wp": Wp, "base": base, "roots": base + 2 * p8, "sizes": base + 2 * p8 + cap4})
        total += (nbytes + 15) & ~15
    work = torch.empty(total, dtype=torch.uint8, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(L.dcfp_label_components_u8(recs, N, _p(maps), maps.numel(), _p(id_table), _p(work), work.numel(),
                                         _p(counts), _stream()), "label_components")
    return Components(recs, layout, work, counts)


def component_pixel(components, n, k):
    """(y, x) of the k[s]-th pixel (0-based, linear-index order) of component n[s] (1-based) of every sample of a
    labelled batch -> device int32 [N,2]; (-1, -1) where n[s] == 0.  A rank-select: the label map is read once."""
    c = components
    dev = c.work.device
    nk = torch.tensor([[int(v) for v in n], [int(v) for v in k]], dtype=torch.int32)
    if tuple(nk.shape) != (2, c.N):
        raise RuntimeError("component_pixel: one (n, k) per sample expected")
    nk = nk.to(dev)
    yx = torch.empty((c.N, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().dcfp_component_pixel_i32(c.records, c.N, _p(c.work), c.work.numel(), _p(c._counts_dev),
                                                  _p(nk[0]), _p(nk[1]), _p(yx), _stream()), "component_pixel")
    return yx


def state_digest_device(t, base=0):
    """The digest of `state_digest`, left on the device: int64 [2] holding (d0, d1) as bits.  No host synchronisation."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("dcfp_amd: state_digest takes a CUDA/HIP tensor (no CPU fallback exists)")
    if t.element_size() != 4 or not t.is_contiguous():
        raise RuntimeError("state_digest: a contiguous tensor of a 4-byte dtype expected, got %s%s"
                           % (t.dtype, "" if t.is_contiguous() else " (not contiguous)"))
    base = int(base)
    if not 0 <= base < 1 << 64:
        raise ValueError("state_digest: base is an unsigned 64-bit index")
    n = t.numel()
    L = _lib.lib()
    out = torch.empty(2, dtype=torch.int64, device=t.device)
    with torch.cuda.device(t.device):
        ws = _workspace("state_digest", L.dcfp_state_digest_workspace_bytes(n), t.device)
        check(L.dcfp_state_digest_u64(_p(t) if n else None, n, base, _p(ws), ws.numel(), _p(out), _stream()),
              "state_digest")
    return out


def state_digest(t, base=0):
    """(d0, d1) of a contiguous CUDA tensor of a 4-byte dtype read as 32-bit words w_i, mod 2^64:
    d0 = sum w_i, d1 = sum (base + i + 1) * w_i.  Two Python ints in [0, 2^64); reading them is one host synchronisation."""
    d0, d1 = state_digest_device(t, base).tolist()
    return d0 & 0xFFFFFFFFFFFFFFFF, d1 & 0xFFFFFFFFFFFFFFFF
