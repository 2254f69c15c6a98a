"""Conv shapes for the kept-weight-copy tests: one small case per forward / dgrad kernel family that keeps a permuted or
transformed copy of its weights in a per-conv buffer (ops._wp_buffer) which ops.refresh_wp() rebuilds after an optimizer
step.  tests/test_wp_layout_host_cpu.py holds every routing written here to dcfp_conv2d_kernel_name and proves the table
complete against a seeded descriptor sweep; tests/test_step_kernels_gpu.py runs the cases.

A case is ((N, Cin, H, W, Cout, k, stride, pad, dil), forward kernel, dgrad kernel); None = that pass is not run for the
case (its family is covered by another row)."""
import ctypes as C
import math
import random

FWD, DGRAD = 0, 1
WINO_FUSED = "winograd_f2x2_3x3 fused (wino_fused_kernel)"
WINO_3PASS = "winograd_f2x2_3x3 (igemm2_dma1p_kernel<false,true>)"

CASES = [
    ((1, 16, 9, 13, 19, 1, 1, 0, 1), "igemm2_kernel<1,1,4,1,4,0>", "igemm2_kernel<1,1,4,1,4,0>"),
    ((2, 47, 9, 13, 64, 1, 1, 0, 1), "igemm2_kernel<1,2,4,1,4,0>", "igemm2_kernel<1,2,4,1,4,0>"),
    ((2, 47, 9, 13, 95, 1, 1, 0, 1), "igemm2_kernel<1,2,2,2,2,0>", None),
    ((2, 47, 11, 15, 257, 3, 1, 1, 1), "igemm2_kernel<9,2,2,2,2,0>", "igemm2_kernel<9,2,4,1,4,0>"),   # Mpad 384, CkP 272
    ((2, 64, 32, 48, 96, 1, 2, 0, 1), None, "igemm2_kernel<1,2,4,2,2,1>"),
    ((2, 16, 17, 19, 24, 3, 2, 1, 1), None, "igemm2_kernel<9,2,4,2,2,1>"),
    ((2, 24, 128, 192, 40, 1, 1, 0, 1), "igemm2_dma8_kernel<1>", "igemm2_dma8_kernel<1>"),            # perm8 1, Mpad 256
    ((2, 24, 128, 192, 200, 3, 1, 4, 4), "igemm2_dma8_kernel<9>", "igemm2_dma8_kernel<9>"),
    ((2, 40, 128, 192, 256, 1, 1, 0, 1), "igemm2_dma1p_kernel", "igemm2_dma8_kernel<1>"),
    ((2, 24, 128, 192, 256, 3, 1, 4, 4), "igemm2_dma_kernel<9,false>", None),
    ((2, 16, 128, 192, 256, 3, 1, 2, 2), "igemm2_dma_kernel<9,true>", "igemm2_kernel<9,1,4,1,4,0>"),
    ((2, 96, 96, 160, 200, 3, 1, 4, 4), WINO_FUSED, WINO_FUSED),                                      # perm8 2 / 3
    # (named after the three-pass path the cost model priced; dcfp_wino_run takes the fused kernel wherever it applies, so
    #  the transformed filters are kept all the same)
    ((2, 128, 64, 96, 192, 3, 1, 4, 4), WINO_3PASS, None),
    ((2, 3, 64, 128, 64, 3, 2, 1, 1), "stem_fwd_kernel", None),              # kept layout exists, the kernel does not read it
    ((2, 2048, 1, 1, 256, 1, 1, 0, 1), "gemv_1x1_map_kernel", "gemv_1x1_map_kernel"),                 # likewise
    # the 128 x 256 tile (M <= 128 filling the chip, or M > 128 short of 192 tiles of 256 x 256) and the 256 x 256 tile off
    # the LDS-DMA shapes (output width no multiple of 4)
    ((2, 16, 129, 191, 128, 1, 1, 0, 1), "igemm2_kernel<1,2,4,2,2,0>", None),
    ((2, 16, 129, 191, 100, 3, 1, 1, 1), "igemm2_kernel<9,2,4,2,2,0>", None),
    ((2, 16, 129, 191, 160, 1, 1, 0, 1), "igemm2_kernel<1,4,4,2,2,0>", None),
    ((2, 16, 129, 191, 160, 3, 1, 1, 1), "igemm2_kernel<9,4,4,2,2,0>", None),
]
# ... and the 1-, 2- and 5-channel layers a pruned model is left with (tests/_narrow_cases.py: one row per kernel they
# reach): M = 1 in a 32- or 256-row copy, Ck = 1 in a 16-channel one.  Their row-pitched rows stay behind - the
# descriptors here are dense - and are refreshed and replayed in tests/test_narrow_widths_gpu.py.
from _narrow_cases import NARROW, NARROW_PITCH  # noqa: E402
CASES += [(case, fwd, dgrad) for case, fwd, dgrad, _ in NARROW if case not in NARROW_PITCH]

# kernels that leave the kept buffer alone (its layout is still registered and refreshed: nothing may depend on it)
UNUSED_COPY = ("stem_fwd_kernel", "gemv_1x1_map_kernel")


def desc_of(case):
    from dcfp_amd import ops
    N, Cin, H, W, Cout, k, s, p, d = case
    return ops._desc((N, Cin, H, W), (Cout, Cin, k, k), s, p, d)


def kernel_name(d, which):
    from dcfp_amd import ops
    return ops.conv_kernel_name(d, which)


def layout(d, which):
    """(status, WpEntry) of dcfp_conv2d_wp_layout."""
    from dcfp_amd import _lib
    e = _lib.WpEntry()
    return _lib.lib().dcfp_conv2d_wp_layout(C.byref(d), which, C.byref(e)), e


def extent_bytes(e):
    """Bytes of the kept buffer the copy described by `e` occupies."""
    return (16 if e.perm8 >= 2 else e.T) * e.CkP * e.Mpad * 4


def block_count(e, block_elems=2048):
    """Blocks of the multi-tensor refresh (DCFP_WP_BLOCK_ELEMS = 2048 elements each; a fused-Winograd entry has one
    (channel, filter) pair per element)."""
    elems = e.CkP * e.Mpad * (1 if e.perm8 >= 2 else e.T)
    return (elems + block_elems - 1) // block_elems


def keeps_copy(d, which):
    """True where a forward / dgrad call of this descriptor gets a per-conv kept buffer with a registered layout."""
    from dcfp_amd import _lib
    if _lib.lib().dcfp_conv2d_workspace_is_scratch(C.byref(d), which):
        return False
    return layout(d, which)[0] == 0


def sweep(n, seed):
    """Seeded descriptors: 1x1 and 3x3, stride 1 / 2, dilation 1 ... 36, pad in {0, d, d + 1}, channel counts on and off
    the 16 / 32 / 64 / 128 / 256 grids, maps from 1 x 1 to 129 x 257."""
    rng = random.Random(seed)
    grid = [16, 32, 64, 128, 256, 512, 1024, 2048]
    sizes = [1, 2, 3, 4, 7, 8, 9, 13, 16, 17, 31, 32, 33, 48, 64, 65, 96, 97, 128, 129, 160, 191, 192, 256, 257]

    def channels():
        r = rng.random()
        if r < 0.4:
            return rng.choice(grid)
        if r < 0.7:
            return max(1, rng.choice(grid) + rng.choice([-3, -1, 1, 5, 24]))
        return rng.randint(1, 600)

    out = []
    while len(out) < n:
        k = rng.choice([1, 3])
        s = rng.choice([1, 1, 1, 2])
        d = rng.choice([1, 1, 2, 3, 4, 6, 12, 16, 18, 24, 36, rng.randint(1, 36)]) if k == 3 else 1
        p = rng.choice([0, d, d + 1]) if k == 3 else 0
        N = rng.choice([1, 2, 3, 8])
        H = min(129, rng.choice(sizes)) if rng.random() < 0.7 else rng.randint(1, 129)
        W = rng.choice(sizes) if rng.random() < 0.7 else rng.randint(1, 257)
        if (H + 2 * p - d * (k - 1) - 1) // s + 1 < 1 or (W + 2 * p - d * (k - 1) - 1) // s + 1 < 1:
            continue
        cin, cout = channels(), channels()
        if rng.random() < 0.02:         # the network's first conv: image channels in, 64 out, 3x3 stride 2
            cin, cout, k, s, p, d = rng.choice([1, 2, 3]), 64, 3, 2, 1, 1
        out.append((N, cin, H, W, cout, k, s, p, d))
    return out


def conv_tolerance(case):
    """The forward bound of tests/test_conv_random_gpu.py (relative L2 against fp64); dgrad uses max(tol, 1e-5)."""
    K = case[1] * case[5] * case[5]
    return 3e-6 * max(1.0, math.sqrt(K) / 8)
