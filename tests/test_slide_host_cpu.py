"""CPU: the host side of the fused sliding-window evaluation - evaluate.sliding_tiles against the reference's loop and
the oracle's tile count, the two geometries it refuses, the descriptor checks of dcfp_vote_sliding_f32 and
dcfp_gather_tiles_f32 (no launch without a GPU) and the --fused-sliding flag of tools/evaluate.py."""
import ctypes
import importlib.util
import os

import pytest
import torch

import _slide_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w), tile: the geometries of tests/test_slide_gpu.py at every scale they use, and the Cityscapes recipe
GEOMETRIES = [((33, 41), (17, 17)), ((20, 60), (9, 25)), ((20, 30), (33, 33)), ((17, 17), (17, 17)),
              ((24, 30), (17, 17)), ((41, 51), (17, 17)), ((32, 48), (17, 17)), ((16, 24), (17, 17)),
              ((56, 84), (17, 17)), ((49, 61), (17, 17)), ((20, 61), (9, 25)), ((1024, 2048), (769, 769))]
GEOMETRIES += [((int(33 * s), int(41 * s)), (17, 25)) for s in sr.SIX_SCALES]


@pytest.mark.parametrize("hw,tile", GEOMETRIES)
def test_sliding_tiles_is_the_reference_loop(hw, tile):
    from dcfp_amd import evaluate as ev
    boxes, rows, cols = sr.reference_tiles(hw[0], hw[1], tile)
    ys, xs = ev.sliding_tiles(hw[0], hw[1], tile)
    assert (len(ys), len(xs)) == (rows, cols)
    mine = [(y, min(y + tile[0], hw[0]), x, min(x + tile[1], hw[1])) for y in ys for x in xs]
    assert mine == boxes
    if hw == (1024, 2048):
        assert (rows, cols) == (2, 4)


class _OneHot:
    """On its k-th call: ones in channel k.  The oracle's result is then cover_k / count per channel."""

    def __init__(self, T, tile):
        self.T, self.tile, self.calls = T, tile, 0

    def __call__(self, image):
        out = torch.zeros((image.shape[0], self.T) + self.tile, dtype=image.dtype)
        out[:, self.calls] = 1
        self.calls += 1
        return [out]


@pytest.mark.parametrize("hw,tile", GEOMETRIES)
def test_coverage_count_is_the_oracles(hw, tile):
    from oracle import evalmetrics
    from dcfp_amd import evaluate as ev
    ys, xs = ev.sliding_tiles(hw[0], hw[1], tile)
    T = len(ys) * len(xs)
    net = _OneHot(T, tile)
    got = evalmetrics.predict_sliding(net, torch.zeros((1, 3) + hw), tile, T)[0]      # [T, h, w] = cover_t / count
    assert net.calls == T
    cover = torch.zeros((T,) + hw)
    for r, y in enumerate(ys):
        for c, x in enumerate(xs):
            cover[r * len(xs) + c, y:y + tile[0], x:x + tile[1]] = 1
    count = cover.sum(0)
    rc = torch.tensor([sum(y <= v < y + tile[0] for y in ys) for v in range(hw[0])])
    cc = torch.tensor([sum(x <= v < x + tile[1] for x in xs) for v in range(hw[1])])
    assert torch.equal(count, (rc[:, None] * cc[None, :]).float())                    # separable
    assert int(count.min()) >= 1
    assert torch.equal(got, cover / count)


def test_refused_geometries():
    from dcfp_amd import evaluate as ev
    with pytest.raises(ValueError) as e:
        ev.sliding_tiles(60, 10, (49, 49))               # stride 33: no tile column at all
    assert "60" in str(e.value) and "10" in str(e.value) and "49" in str(e.value)
    with pytest.raises(ValueError) as e:
        ev.sliding_tiles(60, 20, (25, 9))                # stride 17 > tile_w 9: columns 9 and 10 under no tile
    assert "60" in str(e.value) and "20" in str(e.value) and "25" in str(e.value) and "9" in str(e.value)


def _table(L, per_pass):
    from dcfp_amd import _lib
    flat = []
    for ys, xs in per_pass:
        flat += list(ys) + [0] * (_lib.SLIDE_MAX_TILES_PER_AXIS - len(ys))
        flat += list(xs) + [0] * (_lib.SLIDE_MAX_TILES_PER_AXIS - len(xs))
    return (ctypes.c_int32 * len(flat))(*flat)


def _vote(L, passes, n, host, dev=1, N=1, C=19, H=33, W=41, oh=33, ow=41, scores=1, pred=1, gt=0, conf=0):
    p = lambda v: ctypes.c_void_p(0x1000 if v else None)          # never dereferenced: the checks come before the launch
    return L.dcfp_vote_sliding_f32(passes, n, host, p(dev), N, C, H, W, oh, ow, 1, p(scores), p(pred), p(gt), 255,
                                   p(conf), None)


def test_sliding_vote_descriptor_errors_do_not_need_a_gpu():
    from dcfp_amd import _lib
    L = _lib.lib()
    E = _lib.E_BADDESC
    ok = ([0, 12, 16], [0, 12, 24])                                   # 33 x 41 with 17 x 17 tiles

    def rec(logits=0x1000, lh=3, lw=3, hs=33, ws=41, th=17, tw=17, rows=3, cols=3, flip=0, weight=1.0):
        return _lib.SlidePass(logits, lh, lw, hs, ws, th, tw, rows, cols, flip, weight)
    good = (_lib.SlidePass * 17)(*[rec() for _ in range(17)])
    host = _table(L, [ok] * 17)
    assert _vote(L, good, 0, host) == E
    assert _vote(L, good, 17, host) == E
    assert _vote(L, None, 1, host) == E
    assert _vote(L, good, 1, None) == E                               # no host table
    assert _vote(L, good, 1, host, dev=0) == E                        # no device table
    assert _vote(L, (_lib.SlidePass * 2)(rec(), rec(logits=None)), 2, host) == E
    assert _vote(L, good, 1, host, oh=34) == E
    assert _vote(L, good, 1, host, ow=42) == E
    assert _vote(L, good, 1, host, C=0) == E
    assert _vote(L, good, 1, host, N=0) == E
    assert _vote(L, good, 1, host, gt=0, conf=1) == E                 # conf without gt
    assert _vote(L, good, 1, host, gt=1, conf=1, C=1025) == E         # as dcfp_confusion_matrix_i64
    assert _vote(L, good, 1, host, scores=0, pred=0) == E             # nothing asked for
    for bad in (rec(rows=0), rec(rows=33), rec(cols=0), rec(cols=33), rec(lh=0), rec(tw=0), rec(flip=2),
                rec(weight=float("nan"))):
        assert _vote(L, (_lib.SlidePass * 1)(bad), 1, host) == E
    for ys, xs in (([0, 16, 12], ok[1]),                              # unsorted
                   (ok[0], [0, 24, 12]),
                   ([0, 12, 33], ok[1]),                              # outside the image
                   ([-1, 12, 16], ok[1]),
                   ([1, 12, 16], ok[1]),                              # row 0 under no tile
                   (ok[0], [0, 12, 23]),                              # column 40
                   (ok[0], [0, 18, 24]),                              # column 17
                   ([0, 12, 15], ok[1])):                             # row 32
        assert _vote(L, good, 1, _table(L, [(ys, xs)])) == E
    assert ctypes.sizeof(_lib.SlidePass) == 48
    # the second pass is checked like the first
    assert _vote(L, good, 2, _table(L, [ok, ([0, 12, 15], ok[1])])) == E


def test_gather_tiles_descriptor_errors_do_not_need_a_gpu():
    from dcfp_amd import _lib
    L = _lib.lib()
    E = _lib.E_BADDESC
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)
    p = lambda v: ctypes.c_void_p(0x1000 if v else None)

    def gather(image=1, N=1, ch=3, h=33, w=41, ys=(0, 12, 16), xs=(0, 12, 24), rows=None, cols=None, th=17, tw=17,
               flip=0, tiles=1):
        return L.dcfp_gather_tiles_f32(p(image), N, ch, h, w, arr(ys) if ys else None, len(ys) if rows is None else rows,
                                       arr(xs) if xs else None, len(xs) if cols is None else cols, th, tw, flip,
                                       p(tiles), None)
    assert gather(image=0) == E
    assert gather(tiles=0) == E
    assert gather(ys=None, rows=3) == E
    assert gather(xs=None, cols=3) == E
    assert gather(rows=0) == E
    assert gather(ys=tuple(range(33))) == E
    assert gather(xs=tuple(range(33))) == E
    assert gather(N=0) == E
    assert gather(th=0) == E
    assert gather(flip=2) == E
    assert gather(ys=(0, 12, 33)) == E                                # an origin outside the image
    assert gather(xs=(-1, 12, 24)) == E
    assert L.dcfp_gather_tiles_f32(p(1), 1, 3, 33, 41, arr((0, 12, 16)), 3, arr((0, 12, 24)), 3, 17, 17, 0,
                                   ctypes.c_void_p(0x1004), None) == E    # tiles not 16-byte aligned


def _tool(name):
    spec = importlib.util.spec_from_file_location("_slide_tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_evaluation_tool_knows_the_flag():
    parser = _tool("evaluate").get_parser()
    assert parser.parse_args([]).fused_sliding is False
    assert parser.parse_args(["--fused-sliding", "True"]).fused_sliding is True
    assert parser.parse_args(["--fused-sliding", "False"]).fused_sliding is False
