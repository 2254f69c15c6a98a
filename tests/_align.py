"""Operands off the 16-byte grid for the fp32 training kernels, and the table of conv routes that
tests/test_alignment_gpu.py runs with them.  The kernels of conv_igemm2*.hip, conv_winograd2/3.hip, conv_wgrad.hip,
conv_stem.hip, bn.hip, pool.hip and ppm.hip choose between 16-byte and 4-byte accesses on the host, from the addresses
they are handed; a tensor whose data_ptr() % 16 is 4, 8 or 12 reaches the 4-byte side on shapes that would otherwise
never see it.  A plain helper module like tests/_wp_cases.py: no fixtures, no tests.

displaced(t, k) copies `t` to an address with data_ptr() % 16 == 4 * k inside a buffer whose other floats - `guard` of
them in front and behind at least - hold GUARD_BITS, a NaN no arithmetic produces (quiet NaNs of the hardware are
0x7fc00000 / 0xffc00000): guards_intact() compares bits, so a store outside the tensor is seen, and an output pre-filled
with the pattern (displaced_empty) shows every element that was never written."""
import torch

GUARD_BITS = 0x7FA5C3E1          # a signalling-NaN pattern with a payload of its own


def _fill(buf):
    buf.view(torch.int32).fill_(GUARD_BITS)
    return buf


class Guarded:
    """A tensor view inside a guard-filled buffer.  .view is the tensor to hand to the library."""

    def __init__(self, buf, view, spans):
        self.buf, self.view, self._spans = buf, view, spans      # spans: [(start, stop)] floats of buf the view covers

    def guards_intact(self):
        """True where every float of the buffer outside the view still holds GUARD_BITS."""
        bits = self.buf.view(torch.int32)
        mask = torch.ones(bits.numel(), dtype=torch.bool, device=bits.device)
        for a, b in self._spans:
            mask[a:b] = False
        return bool((bits[mask] == GUARD_BITS).all())

    def unwritten(self):
        """Elements of the view that still hold GUARD_BITS (an output the kernel was to fill completely: 0)."""
        v = self.view.contiguous().view(torch.int32)
        return int((v == GUARD_BITS).sum())


def _place(shape, k, guard, device, lead=0):
    """(buf, first float of the tensor's storage in buf, floats) such that the float `lead` behind `first` sits at an
    address % 16 == 4 * k."""
    assert k in (0, 1, 2, 3) and guard >= 4
    n = 1
    for s in shape:
        n *= int(s)
    buf = _fill(torch.empty(n + 2 * guard + 8, dtype=torch.float32, device=device))
    base = (buf.data_ptr() // 4) % 4
    first = guard + (k - base - guard - lead) % 4
    return buf, first, n


def displaced_empty(shape, k, guard=64, device="cpu"):
    """A guard-filled output of `shape` at data_ptr() % 16 == 4 * k (k = 0: on the grid, with guards all the same)."""
    buf, first, n = _place(shape, k, guard, device)
    view = buf[first:first + n].view(*shape)
    assert view.data_ptr() % 16 == 4 * k and view.is_contiguous()
    return Guarded(buf, view, [(first, first + n)])


def displaced(t, k, guard=64):
    """A copy of the contiguous-shaped tensor `t` (float32, any device) at data_ptr() % 16 == 4 * k."""
    g = displaced_empty(tuple(t.shape), k, guard, t.device)
    g.view.copy_(t)
    return g


def displaced_slice(shape, k, lo, wide, guard=64, device="cpu", src=None):
    """The channel slice [:, lo:lo + C] of a displaced [N, wide, H, W] tensor: dense images, image stride wide * H * W -
    the out= form of ops.conv2d_fwd and the dy form of ops._batch_strided (the ASPP / decoder / PPM concat buffers).
    Everything outside the slice is guard, the other channels included.  src: values to copy into the slice."""
    N, Cc, H, W = shape
    assert lo >= 0 and lo + Cc <= wide
    buf, first, n = _place((N, wide, H, W), k, guard, device)
    whole = buf[first:first + n].view(N, wide, H, W)
    view = whole[:, lo:lo + Cc]
    assert whole.data_ptr() % 16 == 4 * k
    spans = [(first + (i * wide + lo) * H * W, first + (i * wide + lo + Cc) * H * W) for i in range(N)]
    if src is not None:
        view.copy_(src)
    return Guarded(buf, view, spans)


def displaced_pitched(t, k, pitch, guard=64):
    """A row-pitched copy of [N, C, H, W] `t` (rows `pitch` floats apart, zero tails, `pitch - W` zeros in front: the
    contract of DcfpConvDesc.x_pitch) whose first element sits at data_ptr() % 16 == 4 * k."""
    N, Cc, H, W = t.shape
    lead = pitch - W
    buf, first, n = _place((lead + N * Cc * H * pitch,), k, guard, t.device, lead)
    body = buf[first:first + n]
    body.zero_()
    view = body[lead:].view(N, Cc, H, pitch)[..., :W]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * k
    return Guarded(buf, view, [(first, first + n)])


def vector_eligible(case):
    """The shape conditions under which the library's 16-byte branches are taken for aligned operands: whole quads of
    pixels per channel on both sides of the conv (a 1 x 1 map - the gemv - has whole quads of channels instead)."""
    N, Cin, H, W, Cout, k, s, p, d = case
    Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
    if H * W == 1:
        return Cin % 4 == 0 and Cout % 4 == 0
    return (H * W) % 4 == 0 and (Ho * Wo) % 4 == 0 and (Cin * H * W) % 4 == 0 and (Cout * Ho * Wo) % 4 == 0


# ------------------------------------------------------------------ the route table
def _ig(taps, cfg):
    return f"igemm2_kernel<{taps},{cfg}>"


_T0, _T1, _T2, _T3, _T4, _T5 = "1,4,1,4,0", "2,4,1,4,0", "2,4,2,2,0", "2,2,2,2,0", "4,4,2,2,0", "2,4,2,2,1"
D8_1, D8_9, DMA1P, GEMV = "igemm2_dma8_kernel<1>", "igemm2_dma8_kernel<9>", "igemm2_dma1p_kernel", "gemv_1x1_map_kernel"
DMA9, DMA9M = "igemm2_dma_kernel<9,false>", "igemm2_dma_kernel<9,true>"
WINO_FUSED = "winograd_f2x2_3x3 fused (wino_fused_kernel)"
WINO_3PASS = "winograd_f2x2_3x3 (igemm2_dma1p_kernel<false,true>)"
STEM = "stem_fwd_kernel"

# Kernels that copy from their source into LDS 16 bytes at a time (buffer_load ... lds): a displaced source must never
# reach them.  Everything else - the register-staged tile family, the stem, the gemv - reads any 4-byte aligned address.
LDS_DMA = (D8_1, D8_9, DMA1P, DMA9, DMA9M, WINO_FUSED, WINO_3PASS)

# ((N, Cin, H, W, Cout, k, stride, pad, dil), forward kernel, dgrad kernel); None: the pass is not run for the row.
# Every row is vector-eligible (vector_eligible): with aligned operands it takes the 16-byte loads / stores / epilogue
# of its kernel.  The tile rows are those of tests/_wp_cases.CASES on maps of whole quads: 12 x 16 for the 32- and 64-row
# tiles, 132 x 191 (P % 4 == 0, width off the LDS-DMA shapes, 197 tiles of 256 pixels) for the 128- and 256-row ones.
CONV = [
    ((2, 16, 12, 16, 19, 1, 1, 0, 1), _ig(1, _T0), _ig(1, _T0)),
    ((2, 47, 12, 16, 64, 1, 1, 0, 1), _ig(1, _T1), _ig(1, _T1)),
    ((2, 47, 12, 16, 95, 1, 1, 0, 1), _ig(1, _T3), None),
    ((2, 47, 12, 16, 257, 3, 1, 1, 1), _ig(9, _T3), _ig(9, _T1)),
    ((2, 64, 32, 48, 96, 1, 2, 0, 1), None, _ig(1, _T5)),                    # strided dgrad, one live phase
    ((2, 16, 16, 20, 24, 3, 2, 1, 1), _ig(9, _T0), _ig(9, _T5)),             # strided dgrad, four phases
    ((2, 16, 132, 191, 128, 1, 1, 0, 1), _ig(1, _T2), None),                 # the 128-row tile
    ((2, 16, 132, 191, 100, 3, 1, 1, 1), _ig(9, _T2), None),
    ((2, 16, 132, 191, 160, 1, 1, 0, 1), _ig(1, _T4), None),
    ((2, 16, 132, 191, 160, 3, 1, 1, 1), _ig(9, _T4), None),
    ((2, 24, 128, 192, 40, 1, 1, 0, 1), D8_1, D8_1),
    ((2, 24, 128, 192, 200, 3, 1, 4, 4), D8_9, D8_9),                        # the largest shape of the file
    ((2, 40, 128, 192, 256, 1, 1, 0, 1), DMA1P, D8_1),
    ((2, 24, 128, 192, 256, 3, 1, 4, 4), DMA9, None),
    ((2, 16, 128, 192, 256, 3, 1, 2, 2), DMA9M, _ig(9, _T0)),
    ((2, 96, 96, 160, 200, 3, 1, 4, 4), WINO_FUSED, WINO_FUSED),
    ((2, 128, 64, 96, 192, 3, 1, 4, 4), WINO_3PASS, None),
    ((2, 3, 64, 128, 64, 3, 2, 1, 1), STEM, None),
    ((2, 2048, 1, 1, 256, 1, 1, 0, 1), GEMV, GEMV),
]
# ... and the row-pitched rows of tests/_narrow_cases.NARROW_PITCH (x / dy with the pitch the network gives them)
from _narrow_cases import NARROW_PITCH  # noqa: E402
CONV += [(case, D8_9, D8_9) for case in sorted(NARROW_PITCH)]

# rows that also run the options of the issue: want_stats, keep=, conv2d_fused_infer with a displaced residual
OPTION_ROWS = [(2, 40, 128, 192, 256, 1, 1, 0, 1), (2, 16, 132, 191, 128, 1, 1, 0, 1), (2, 96, 96, 160, 200, 3, 1, 4, 4)]
# the masked fan-in data gradient (Cin % 256 == 0, H * W % 256 == 0, the persistent 1x1 kernel)
FANIN_ROW = (2, 256, 128, 192, 32, 1, 1, 0, 1)

WG1, WG9 = "wgrad2_kernel<1,2,2,1,1>", "wgrad2_kernel<9,2,2,1,1>"
WIDE1, WIDE9 = "wgrad_dma_kernel<1,false,true>", "wgrad_dma_kernel<9,false,true>"
WINO_WG_FUSED = "winograd_f2x2_3x3 wgrad fused (wino_wgrad_fused_kernel)"
WINO_WG = "winograd_f2x2_3x3 wgrad (wgrad_dma_kernel<1,false,false,true>)"
STEM_WG = "stem_wgrad_kernel"
WGRAD_LDS_DMA = (WIDE1, WIDE9, WINO_WG_FUSED, WINO_WG, "wgrad_dma_kernel<1,false>", "wgrad_dma_kernel<9,false>",
                 "wgrad_dma_kernel<9,true>")

# (case, weight-gradient kernel, x row pitch (0: dense), what else the row is there for)
WGRAD = [
    ((2, 16, 12, 16, 19, 1, 1, 0, 1), WG1, 0, "bias"),                       # the one-wave tile (+ need_bias)
    ((2, 23, 12, 16, 5, 3, 1, 2, 2), WG9, 0, ""),
    ((2, 5, 12, 16, 150, 3, 1, 1, 1), "wgrad2_kernel<9,4,1,2,2>", 0, ""),    # the lop-sided tiles
    ((2, 8, 12, 16, 130, 3, 1, 2, 2), "wgrad2_kernel<9,4,2,2,2>", 0, ""),
    ((2, 130, 16, 32, 1, 1, 1, 0, 1), WIDE1, 0, ""),
    ((2, 130, 128, 192, 5, 3, 1, 2, 2), WIDE9, 196, ""),                     # pitched x
    ((2, 256, 32, 32, 256, 1, 1, 0, 1), "wgrad_dma_kernel<1,false>", 0, "splits bias"),   # several splits, 65536 % 4 == 0
    ((2, 96, 96, 160, 200, 3, 1, 4, 4), WINO_WG_FUSED, 0, ""),
    ((2, 256, 64, 128, 256, 3, 1, 2, 2), WINO_WG, 0, "kept"),                 # the forward leaves its transform behind
    ((2, 3, 64, 128, 64, 3, 2, 1, 1), STEM_WG, 0, ""),
    ((2, 2048, 1, 1, 256, 1, 1, 0, 1), GEMV, 0, ""),
]


def conv_names():
    """Every forward / dgrad kernel name tests/_wp_cases.CASES and tests/_narrow_cases.NARROW can produce."""
    import _narrow_cases as nc
    import _wp_cases as wp
    names = set()
    for _, fwd, dgrad in wp.CASES:
        names |= {fwd, dgrad}
    for _, fwd, dgrad, _ in nc.NARROW:
        names |= {fwd, dgrad}
    return names - {None}


def wgrad_names():
    import _narrow_cases as nc
    return {wg for *_, wg in nc.NARROW} - {None}
