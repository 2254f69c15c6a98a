"""The tile plan the Winograd paths share (csrc/wino_plan.h, exported as dcfp_wino_tile_plan), on the CPU for every
H, W in 1..80 and d in {1, 2, 4, 6, 12, 36}: the enumerated tiles cover every output pixel exactly once, a tile in a
reduced component class really has the skipped outputs outside the image, regions are whole 64-tile blocks, and a
map whose H and W are multiples of 2d keeps the full grid of super-blocks (TH, TW, T of the plan without the
ragged-map savings, which is also what ragged = 0 gives everywhere)."""
import ctypes as C

import numpy as np
import pytest

DILS = (1, 2, 4, 6, 12, 36)
N = 2


def _plan(L, H, W, d, ragged, classes):
    out = (C.c_int64 * 39)()
    assert L.dcfp_wino_tile_plan(N, H, W, d, ragged, classes, out) == 0
    TH, TW, T, T16, nreg, tblocks = out[0:6]
    regs = [tuple(out[6 + 8 * i: 14 + 8 * i]) for i in range(nreg)]
    assert out[38] == sum(N * r[1] * r[3] * (4 if r[4] else 3) * (4 if r[5] else 3) for r in regs)     # components issued
    return TH, TW, T, T16, regs, tblocks


def _full_grid(H, W, d):
    TH = d * ((H + 2 * d - 1) // (2 * d))
    TW = (d * ((W + 2 * d - 1) // (2 * d)) + 3) // 4 * 4
    return TH, TW


def _axis_cover(t0, n, d, size):
    """Per pixel of the axis: how many of the tiles t0 .. t0 + n - 1 own it; and the tiles' first / second output."""
    t = np.arange(t0, t0 + n)
    o0 = t + d * (t // d)
    o1 = o0 + d
    own = np.concatenate([o0[o0 < size], o1[o1 < size]])
    return np.bincount(own, minlength=size)[:size], o0, o1


@pytest.fixture(scope="module")
def L():
    from dcfp_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("d", DILS)
def test_plan_covers_every_pixel_once_and_classes_are_true(L, d):
    for H in range(1, 81):
        for W in range(1, 81):
            for classes in (1, 0):
                TH, TW, T, T16, regs, tblocks = _plan(L, H, W, d, 1, classes)
                assert T == N * TH * TW and T16 == (T + 15) // 16 * 16 and TW % 4 == 0
                assert TH <= _full_grid(H, W, d)[0] and TW <= _full_grid(H, W, d)[1]
                if not classes:
                    assert regs == [(0, TH, 0, TW, 1, 1, 0, (T + 63) // 64)]
                grid = np.zeros((H, W), dtype=np.int64)
                nb = 0
                for i, (r0, nr, c0, nc, rows3, cols3, tb0, nblocks) in enumerate(regs):
                    assert nr > 0 and nc > 0 and c0 % 4 == 0 and nc % 4 == 0
                    assert r0 + nr <= TH and c0 + nc <= TW
                    assert tb0 == nb and nblocks == (N * nr * nc + 63) // 64      # whole blocks, back to back
                    nb += nblocks
                    cr, ho0, ho1 = _axis_cover(r0, nr, d, H)
                    cc, wo0, wo1 = _axis_cover(c0, nc, d, W)
                    grid += np.outer(cr, cc)
                    if not rows3:
                        assert (ho1 >= H).all(), (H, W, d, "a 12-component tile has its second output row inside")
                    if not cols3:
                        assert (wo1 >= W).all(), (H, W, d, "a 12-component tile has its second output column inside")
                    if i > 0:
                        assert not (rows3 and cols3)                             # the 16-component region comes first
                assert nb == tblocks
                assert (grid == 1).all(), (H, W, d, classes)
                area = sum(r[1] * r[3] for r in regs)
                assert area == TH * TW                                            # the regions tile the enumerated grid


@pytest.mark.parametrize("d", DILS)
def test_plan_of_a_whole_map_is_the_full_grid(L, d):
    for H in range(2 * d, 81, 2 * d):
        for W in range(2 * d, 81, 2 * d):
            TH, TW, T, T16, regs, tblocks = _plan(L, H, W, d, 1, 1)
            assert (TH, TW) == _full_grid(H, W, d) == (H // 2, (W // 2 + 3) // 4 * 4)
            assert T == N * TH * TW and regs == [(0, TH, 0, TW, 1, 1, 0, (T + 63) // 64)]
            assert _plan(L, H, W, d, 0, 1) == (TH, TW, T, T16, regs, tblocks)
    # ragged = 0: the full grid in one 16-component region on every map
    for H, W in ((1, 1), (7, 12), (10, 20), (14, 32), (64, 80), (79, 77)):
        TH, TW, T, T16, regs, tblocks = _plan(L, H, W, d, 0, 1)
        assert (TH, TW) == _full_grid(H, W, d) and regs == [(0, TH, 0, TW, 1, 1, 0, (T + 63) // 64)]


def test_plan_of_the_aspp_maps(L):
    """The counts the change was sized with: 128 x 256 at d = 12 / 24 / 36 (full / half tile rows and columns)."""
    want = {12: (68, 132, 60, 124), 24: (72, 136, 56, 120), 36: (72, 144, 56, 112)}
    for d, (TH, TW, fr, fc) in want.items():
        th, tw, T, T16, regs, _ = _plan(L, 128, 256, d, 1, 1)
        assert (th, tw) == (TH, TW)
        assert regs[0][:6] == (0, fr, 0, fc, 1, 1)
        assert [r[4:6] for r in regs] == [(1, 1), (0, 1), (1, 0), (0, 0)]
