"""The kernels that run once per optimizer step through a device-resident pointer table, and the Python caches that decide
when those tables are rebuilt: the multi-tensor weight-copy refresh (ops.refresh_wp) against the copy every conv builds
for itself and against fp64 convolutions, the SGD and EIC kernels through the C ABI against fp64 / the bit-exact oracle,
and FusedSGD's state transitions against torch.optim.SGD."""
import ctypes as C
import math
import weakref

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _wp_cases import CASES, FWD, DGRAD, UNUSED_COPY, block_count, conv_tolerance, desc_of, extent_bytes, kernel_name, layout
from oracle import scoring

pytestmark = pytest.mark.gpu

PASSES = [(i, which) for i, (_, fwd, dgrad) in enumerate(CASES) for which, want in ((FWD, fwd), (DGRAD, dgrad))
          if want is not None]


# ---------------------------------------------------------------------------------------------- kept weight copies
@pytest.fixture
def wp(monkeypatch):
    """The registry of kept copies, empty for this test (weights other tests left alive would join the refresh table and
    make its order and size depend on the test order), and a spy on what every conv call is told about its buffer."""
    from dcfp_amd import ops, _lib
    monkeypatch.setattr(ops, "_WP_OWNERS", weakref.WeakSet())
    monkeypatch.setattr(ops, "_WP_TABLE", {"version": 0, "built": -1, "dev": None, "n": 0, "blocks": 0, "entries": []})
    seen = []
    real = ops._conv_workspace

    def spy(w, which, d, variant=""):
        ws, valid = real(w, which, d, variant)
        seen.append((which, variant, valid, ws.data_ptr()))
        return ws, valid
    monkeypatch.setattr(ops, "_conv_workspace", spy)
    launches = []
    L = _lib.lib()
    real_refresh = L.dcfp_conv2d_permute_weights_multi_f32

    def counted(table, n, blocks, stream):
        launches.append((n, blocks))
        return real_refresh(table, n, blocks, stream)
    monkeypatch.setattr(L, "dcfp_conv2d_permute_weights_multi_f32", counted)
    return {"seen": seen, "launches": launches}


def _key(case, which, variant=""):
    N, Cin, H, W, Cout, k, s, p, d = case
    return (which, N, H, W, s, p, d, 0, 0, variant)


def _operand(case, which, gen, device):
    N, Cin, H, W, Cout, k, s, p, d = case
    dsc = desc_of(case)
    shape = (N, Cin, H, W) if which == FWD else (N, Cout, dsc.Hout, dsc.Wout)
    return torch.randn(shape, generator=gen).to(device)


def _weights(case, gen, device):
    N, Cin, H, W, Cout, k, s, p, d = case
    return (torch.randn(Cout, Cin, k, k, generator=gen) / math.sqrt(Cin * k * k)).to(device)


def _run(case, which, t, w):
    from dcfp_amd import ops
    N, Cin, H, W, Cout, k, s, p, d = case
    if which == FWD:
        return ops.conv2d_fwd(t, w, None, s, p, d)
    return ops.conv2d_dgrad(t, w, (N, Cin, H, W), s, p, d)


def _ref64(case, which, t, w):
    N, Cin, H, W, Cout, k, s, p, d = case
    t64, w64 = t.detach().cpu().double(), w.detach().cpu().double()
    if which == FWD:
        return F.conv2d(t64, w64, None, s, p, d)
    return torch.nn.grad.conv2d_input((N, Cin, H, W), w64, t64, s, p, d)


def _rel(a, b):
    a = a.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _bound(case, which):
    tol = conv_tolerance(case)
    return tol if which == FWD else max(tol, 1e-5)


def _expected_copy(w, e):
    """The permuted copy written out from its definition: Wp[t][c][slot] = w[row(slot)*sAm + c*sAc + t], zero for the
    padding rows / channels; row() is the identity, or for perm8 = 1 the 8-way interleave of each 256-row group."""
    W3 = torch.as_strided(w.detach().reshape(-1), (e.M, e.Ck, e.T), (e.sAm, e.sAc, 1))
    slot = torch.arange(e.Mpad, device=w.device)
    if e.perm8 == 1:
        j = slot % 256
        row = (slot - j) + 32 * (j % 8) + j // 8
    else:
        assert e.perm8 == 0
        row = slot
    live = row < e.M
    out = torch.zeros(e.T, e.CkP, e.Mpad, dtype=torch.float32, device=w.device)
    out[:, :e.Ck, live] = W3[row[live]].permute(2, 1, 0)
    return out.reshape(-1)


def _same_bytes(buf, nbytes, floats):
    return torch.equal(buf[:nbytes].view(torch.int32), floats.contiguous().view(torch.int32).reshape(-1))


def _refresh():
    from dcfp_amd import ops
    ops.WEIGHT_EPOCH[0] += 1
    ops.refresh_wp()


@pytest.mark.parametrize("ci,which", PASSES, ids=[f"{i}-{'fwd' if wh == FWD else 'dgrad'}" for i, wh in PASSES])
def test_refreshed_copy_equals_on_demand_copy(cuda, wp, ci, which):
    case, name = CASES[ci][0], CASES[ci][1 + which]
    dsc = desc_of(case)
    assert kernel_name(dsc, which) == name
    rc, e = layout(dsc, which)
    assert rc == 0
    ext = extent_bytes(e)
    gen = torch.Generator().manual_seed(1000 + 2 * ci + which)
    t, w = _operand(case, which, gen, cuda), _weights(case, gen, cuda)
    seen, key = wp["seen"], _key(case, which)

    cold = _run(case, which, t, w)                                   # 1: wp_valid = 0, the conv builds its own copy
    assert seen[-1][2] == 0
    buf = w._dcfp_wp[key][1]
    assert seen[-1][3] == buf.data_ptr() and buf.numel() >= ext
    snap = buf[:ext].clone()
    used = name not in UNUSED_COPY
    if used and e.perm8 < 2:
        assert _same_bytes(snap, ext, _expected_copy(w, e)), "the on-demand copy is not the documented layout"
    buf.fill_(0xFF)                                                  # 2
    _refresh()                                                       # 3
    assert wp["launches"] == [(1, e.n_blocks)] and e.n_blocks == block_count(e)
    if used:                                                         # 4
        assert torch.equal(buf[:ext], snap), "refresh_wp() and the conv disagree about the kept copy"
    elif e.perm8 < 2:
        assert _same_bytes(buf, ext, _expected_copy(w, e))
    assert bool((buf[ext:] == 0xFF).all()), "the refresh wrote past the layout's extent"
    again = _run(case, which, t, w)                                  # 5
    assert seen[-1][2] == 1 and seen[-1][3] == buf.data_ptr(), "the refreshed copy was not taken (wp_valid)"
    assert torch.equal(again, cold)                                  # 6
    version = w._version                                             # 7: what FusedSGD does - torch does not see the write
    w.data.view(-1)[::7] += 0.01
    w.data.mul_(1.25)
    assert w._version == version
    _refresh()
    out = _run(case, which, t, w)
    assert seen[-1][2] == 1
    fresh = _run(case, which, t, w.clone())                          # 8
    assert seen[-1][2] == 0
    assert torch.equal(out, fresh) and not torch.equal(out, cold)
    if not used:                                                     # (nothing reads the buffer: any content must do)
        buf.fill_(0xFF)
        assert torch.equal(_run(case, which, t, w), fresh)
    r = _rel(out, _ref64(case, which, t, w))                         # 9
    assert r < _bound(case, which), (case, which, r)
    torch.cuda.synchronize()


def test_one_refresh_serves_all_registered_weights(cuda, wp):
    """Every case registered at once (the same weight under its forward and its dgrad key): ONE launch rebuilds them all.
    Entries of 1 ... 256 blocks in whatever order the registry yields them - the first, the last and the one-block
    entries of the kernel's binary search over first_block are all among those checked."""
    from dcfp_amd import ops
    gen = torch.Generator(device=cuda).manual_seed(7)
    held = []
    for ci, (case, fwd, dgrad) in enumerate(CASES):
        N, Cin, H, W, Cout, k, s, p, d = case
        w = torch.randn(Cout, Cin, k, k, generator=gen, device=cuda) / math.sqrt(Cin * k * k)
        dsc = desc_of(case)
        for which, want in ((FWD, fwd), (DGRAD, dgrad)):
            if want is None:
                continue
            shape = (N, Cin, H, W) if which == FWD else (N, Cout, dsc.Hout, dsc.Wout)
            _run(case, which, torch.randn(shape, generator=gen, device=cuda), w)
            e = layout(dsc, which)[1]
            buf = w._dcfp_wp[_key(case, which)][1]
            held.append((case, which, want, w, e, buf, buf[:extent_bytes(e)].clone()))
    assert len(held) == len(PASSES) >= 25
    for *_, buf, _ in held:
        buf.fill_(0xFF)
    _refresh()
    blocks = [h[4].n_blocks for h in held]
    assert wp["launches"] == [(len(held), sum(blocks))] and min(blocks) == 1 and max(blocks) >= 256
    T = ops._WP_TABLE
    table = np.frombuffer(T["dev"].cpu().numpy().tobytes(), dtype=np.int64).reshape(len(held), -1)
    assert table[0, 2] == 0 and (np.diff(table[:, 2]) == table[:-1, 3]).all()        # first_block is the running sum
    assert sorted(table[:, 1].tolist()) == sorted(h[5].data_ptr() for h in held)
    for case, which, name, w, e, buf, snap in held:
        ext = extent_bytes(e)
        if name not in UNUSED_COPY:
            assert torch.equal(buf[:ext], snap), (case, which, name)
        if e.perm8 < 2:
            assert _same_bytes(buf, ext, _expected_copy(w, e)), (case, which, name)
        assert bool((buf[ext:] == 0xFF).all()), (case, which, name)
        assert w._dcfp_wp[_key(case, which)][0][2] == ops.WEIGHT_EPOCH[0]           # marked valid for this epoch
    torch.cuda.synchronize()


def _edit(w):
    w.data.view(-1)[::5] -= 0.02
    w.data.mul_(0.8)


@pytest.mark.parametrize("case", [(2, 64, 16, 32, 64, 1, 1, 0, 1), (2, 16, 128, 192, 256, 1, 1, 0, 1)],
                         ids=["tile64x512", "dma1p"])
def test_statistics_and_plain_forward_share_the_kept_copy(cuda, wp, case):
    """conv2d_fwd(want_stats=True) (BatchNorm statistics in the epilogue) and the plain forward of one weight use one
    buffer; each takes over the copy the refresh built after the other flavour ran."""
    from dcfp_amd import ops
    N, Cin, H, W, Cout, k, s, p, d = case
    gen = torch.Generator().manual_seed(41)
    x, w = _operand(case, FWD, gen, cuda), _weights(case, gen, cuda)
    seen = wp["seen"]

    def stats(wt):
        y, st = ops.conv2d_fwd(x, wt, None, s, p, d, want_stats=True)
        assert st is not None, "this shape has fused statistics"
        return y, st[0], st[1]
    y0 = stats(w)
    assert seen[-1][2] == 0
    buf = seen[-1][3]
    _edit(w); _refresh()
    y1 = ops.conv2d_fwd(x, w, None, s, p, d)
    assert seen[-1][2:] == (1, buf)
    assert torch.equal(y1, ops.conv2d_fwd(x, w.clone(), None, s, p, d)) and not torch.equal(y1, y0[0])
    _edit(w); _refresh()
    y2 = stats(w)
    assert seen[-1][2:] == (1, buf)
    c2 = stats(w.clone())
    assert seen[-1][2] == 0
    assert all(torch.equal(a, b) for a, b in zip(y2, c2))
    assert _rel(y2[0], _ref64(case, FWD, x, w)) < _bound(case, FWD)
    y64 = _ref64(case, FWD, x, w)
    assert _rel(y2[1], y64.mean((0, 2, 3))) < 2e-5 and _rel(y2[2], y64.var((0, 2, 3), unbiased=False)) < 2e-5
    assert len(w._dcfp_wp) == 1
    torch.cuda.synchronize()


def test_fanin_and_plain_dgrad_share_the_kept_copy(cuda, wp):
    """conv2d_dgrad_fanin on its smallest shape (256 input channels, H*W a multiple of 256, the 256 x 256 tile) and the
    plain data gradient of the same weight, interleaved across refreshes."""
    from dcfp_amd import ops
    N, Cin, H, W, Cout = 2, 256, 128, 192, 32
    xs = (N, Cin, H, W)
    gen = torch.Generator(device=cuda).manual_seed(43)
    rnd = lambda *sh: torch.randn(*sh, generator=gen, device=cuda)
    w = rnd(Cout, Cin, 1, 1) / math.sqrt(Cin)
    assert ops.conv2d_dgrad_fanin_ok((N, Cout, H, W), w, xs)
    dy, fan_src, c3, res = rnd(N, Cout, H, W), rnd(*xs), rnd(*xs), rnd(*xs)
    mean, var = ops.bn_stats(c3)
    y, mask = ops.bn_apply_relu_mask(c3, mean, var, torch.ones(Cin, device=cuda), torch.zeros(Cin, device=cuda), 1e-5, res)
    seen = wp["seen"]
    f0 = ops.conv2d_dgrad_fanin(dy, w, xs, fan_src, mask)
    assert seen[-1][2] == 0
    buf = seen[-1][3]
    _edit(w); _refresh()
    p1 = ops.conv2d_dgrad(dy, w, xs, 1, 0, 1)
    assert seen[-1][2:] == (1, buf)
    assert torch.equal(p1, ops.conv2d_dgrad(dy, w.clone(), xs, 1, 0, 1))
    _edit(w); _refresh()
    f2 = ops.conv2d_dgrad_fanin(dy, w, xs, fan_src, mask)
    assert seen[-1][2:] == (1, buf)
    assert torch.equal(f2, ops.conv2d_dgrad_fanin(dy, w.clone(), xs, fan_src, mask)) and not torch.equal(f2, f0)
    p2 = ops.conv2d_dgrad(dy, w, xs, 1, 0, 1)
    assert seen[-1][2:] == (1, buf)
    # the fan-in is the plain gradient plus the masked residual gradient (one more rounding)
    want = p2.double() + fan_src.double() * (y > 0).double()
    assert float((f2.double() - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())
    assert len(w._dcfp_wp) == 1
    torch.cuda.synchronize()


def test_biased_classifier_shares_the_kept_copy(cuda, wp):
    from dcfp_amd import ops
    case = (2, 256, 33, 33, 19, 1, 1, 0, 1)
    gen = torch.Generator().manual_seed(47)
    x, w = _operand(case, FWD, gen, cuda), _weights(case, gen, cuda)
    b = torch.randn(19, generator=gen).to(cuda)
    seen = wp["seen"]
    ops.conv2d_fwd(x, w, None)
    buf = seen[-1][3]
    _edit(w); _refresh()
    yb = ops.conv2d_fwd(x, w, b)
    assert seen[-1] == (FWD, "", 1, buf)
    assert torch.equal(yb, ops.conv2d_fwd(x, w.clone(), b))
    ref = _ref64(case, FWD, x, w) + b.cpu().double().view(1, -1, 1, 1)
    assert _rel(yb, ref) < _bound(case, FWD)
    _edit(w); _refresh()
    y = ops.conv2d_fwd(x, w, None)
    assert seen[-1] == (FWD, "", 1, buf)
    assert torch.equal(y, ops.conv2d_fwd(x, w.clone(), None))
    torch.cuda.synchronize()


def test_bias_and_fused_variants_are_left_to_their_calls(cuda, wp):
    """A 3x3 conv whose plain forward is Winograd: the biased forward (direct kernel) and the inference call with a folded
    BatchNorm keep copies of their own ("bias" / "fused"), which refresh_wp() neither lists nor touches; they rebuild
    on demand when the weights change."""
    from dcfp_amd import ops
    case = (2, 96, 96, 160, 200, 3, 1, 4, 4)
    N, Cin, H, W, Cout, k, s, p, d = case
    assert kernel_name(desc_of(case), FWD).startswith("winograd")
    gen = torch.Generator().manual_seed(53)
    x, w = _operand(case, FWD, gen, cuda), _weights(case, gen, cuda)
    b = torch.randn(Cout, generator=gen).to(cuda)
    sc, sh = (torch.rand(Cout, generator=gen) + 0.5).to(cuda), torch.randn(Cout, generator=gen).to(cuda)
    seen = wp["seen"]

    def three(wt):
        return (ops.conv2d_fwd(x, wt, None, s, p, d), ops.conv2d_fwd(x, wt, b, s, p, d),
                ops.conv2d_fused_infer(x, wt, sc, sh, s, p, d, None, True))
    a0 = three(w)
    assert [v[1] for v in seen[-2:]] == ["", "bias"]
    kb, kf = _key(case, FWD, "bias"), _key(case, FWD, "fused")
    assert set(w._dcfp_wp) == {_key(case, FWD), kb, kf}
    snaps = {kk: w._dcfp_wp[kk][1].clone() for kk in (kb, kf)}
    tags = {kk: w._dcfp_wp[kk][0] for kk in (kb, kf)}
    _refresh()
    assert wp["launches"][-1][0] == 1                                # one entry: the plain forward's
    for kk in (kb, kf):
        assert torch.equal(w._dcfp_wp[kk][1], snaps[kk]) and w._dcfp_wp[kk][0] == tags[kk]
    _edit(w); _refresh()
    a1 = three(w)
    assert [v[2] for v in seen[-2:]] == [1, 0]
    c1 = three(w.clone())
    assert all(torch.equal(u, v) for u, v in zip(a1, c1)) and not any(torch.equal(u, v) for u, v in zip(a1, a0))
    y64 = _ref64(case, FWD, x, w)
    assert _rel(a1[0], y64) < _bound(case, FWD)
    assert _rel(a1[1], y64 + b.cpu().double().view(1, -1, 1, 1)) < _bound(case, FWD)
    ref = torch.relu(y64 * sc.cpu().double().view(1, -1, 1, 1) + sh.cpu().double().view(1, -1, 1, 1))
    assert _rel(a1[2], ref) < _bound(case, FWD)
    torch.cuda.synchronize()


def test_cache_transitions_keep_results_right(cuda, wp):
    """Replaced storage, more shapes on one weight than the cache holds, a shape first seen after the table was built:
    every result equals the cold call's bit for bit and the fp64 convolution within the conv bound."""
    Cin, Cout = 47, 95
    gen = torch.Generator().manual_seed(59)
    w = _weights((1, Cin, 1, 1, Cout, 3, 1, 1, 1), gen, cuda)
    xs = {}

    def check(hw, which=FWD):
        case = (2, Cin, hw[0], hw[1], Cout, 3, 1, 1, 1)
        if (hw, which) not in xs:
            xs[(hw, which)] = _operand(case, which, gen, cuda)
        t = xs[(hw, which)]
        out = _run(case, which, t, w)
        valid = wp["seen"][-1][2]
        assert torch.equal(out, _run(case, which, t, w.clone())), (hw, which)
        assert _rel(out, _ref64(case, which, t, w)) < _bound(case, which), (hw, which)
        return valid

    assert check((9, 13)) == 0
    _edit(w); _refresh()
    assert check((9, 13)) == 1
    # a shape first seen after the table was built: cold now, part of the next refresh
    assert check((12, 16)) == 0 and check((12, 16), DGRAD) == 0
    _edit(w); _refresh()
    assert wp["launches"][-1][0] == 3
    assert check((9, 13)) == 1 and check((12, 16)) == 1 and check((12, 16), DGRAD) == 1
    # the storage is replaced (a load by assignment): the copies are stale whatever the epoch says
    _refresh()                         # (the table is up to date, on the old storage)
    w.data = w.data.clone()
    launched = len(wp["launches"])
    _edit(w); _refresh()               # notices the move: launches nothing (its table points at the old storage)
    assert len(wp["launches"]) == launched
    assert check((9, 13)) == 0 and check((12, 16)) == 0
    _edit(w); _refresh()               # table rebuilt on the new storage
    assert len(wp["launches"]) == launched + 1 and wp["launches"][-1][0] == 3
    assert check((9, 13)) == 1 and check((12, 16), DGRAD) == 1
    # more than 8 shapes on one weight (multi-scale evaluation): the cache is cleared, later refreshes follow
    for i in range(9):
        assert check((5 + i, 7)) == 0
    assert len(w._dcfp_wp) <= 9
    _edit(w); _refresh()
    _edit(w); _refresh()
    live = [kk for kk in w._dcfp_wp]
    assert wp["launches"][-1][0] == len(live)
    assert check((13, 7)) == 1 and check((9, 13)) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- SGD kernel (C ABI)
U = 2.0 ** -24
SGD_SIZES = [1, 255, 256, 257, 16383, 16384, 16385, 2 * 16384, 70001]


def _sgd_layout():
    rng = np.random.RandomState(61)
    sizes = rng.randint(1, 301, 300).tolist() + SGD_SIZES + rng.randint(1, 301, 300).tolist()
    offs, off = [], 0
    for n in sizes:
        off += int(rng.randint(1, 70))           # a gap of sentinels in front of every tensor (and one behind the last)
        offs.append(off)
        off += n
    return sizes, offs, off + 64


@pytest.mark.parametrize("momentum,first,lr", [(0.9, 0, 0.0123), (0.9, 1, 0.0123), (0.0, 0, 0.0123), (0.0, 1, 0.0123),
                                               (0.9, 0, 0.0), (0.9, 1, 0.0)])
def test_sgd_kernel_against_fp64_per_element(cuda, capsys, momentum, first, lr):
    """sgd_momentum_kernel over a hand-built table on ONE flat buffer per operand (sentinels between the tensors):
    g' = g + wd*p; buf = first ? g' : m*buf + g'; p' = p - lr*buf against the same lines in fp64 from the fp32 inputs.
    Per-element bounds from unit roundoff u = 2^-24, twice the worst case of the four roundings (two FMAs, a multiply,
    an add): |dp'| <= 2u(|p'| + lr(m|buf| + |b| + |g'|)), |db| <= 2u(m|buf| + |b| + |g'|)."""
    from dcfp_amd import _lib
    from dcfp_amd._lib import SgdEntry, SGD_CHUNK
    sizes, offs, total = _sgd_layout()
    SENT = np.float32(-12345.678)
    rng = np.random.RandomState(67)
    host = {k: np.full(total, SENT, np.float32) for k in "pgb"}
    live = np.zeros(total, bool)
    wd_el = np.zeros(total, np.float32)
    entries = (SgdEntry * len(sizes))()
    dev = {}
    chunk = 0
    wds = []
    for i, (n, o) in enumerate(zip(sizes, offs)):
        wd = np.float32(5e-4 if (i % 3) else 0.0)
        wds.append(wd)
        host["p"][o:o + n] = rng.randn(n).astype(np.float32)
        host["g"][o:o + n] = (rng.randn(n) * 0.3).astype(np.float32)
        host["b"][o:o + n] = np.nan if first else (rng.randn(n) * 0.5).astype(np.float32)
        live[o:o + n] = True
        wd_el[o:o + n] = wd
    for k in "pgb":
        dev[k] = torch.from_numpy(host[k].copy()).to(cuda)
    for i, (n, o) in enumerate(zip(sizes, offs)):
        e = entries[i]
        e.param, e.grad, e.momentum_buf = (dev[k].data_ptr() + 4 * o for k in "pgb")
        e.n, e.first_chunk, e.weight_decay = n, chunk, float(wds[i])
        chunk += (n + SGD_CHUNK - 1) // SGD_CHUNK
    assert chunk == 600 + 6 + 2 + 2 + 5 and len(sizes) == 609          # one chunk each, 16385 and 2*16384 two, 70001 five
    table = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8).to(cuda)
    _lib.check(_lib.lib().dcfp_sgd_momentum_f32(C.c_void_p(table.data_ptr()), len(sizes), chunk, lr, momentum, first,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "sgd")
    torch.cuda.synchronize()
    out = {k: dev[k].cpu().numpy() for k in "pgb"}
    for k in "pgb":                                                  # nothing written past n, gradients untouched
        assert np.array_equal(out[k][~live].view(np.int32), host[k][~live].view(np.int32)), k
    assert np.array_equal(out["g"].view(np.int32), host["g"].view(np.int32))
    p, g = host["p"][live].astype(np.float64), host["g"][live].astype(np.float64)
    m, lr64, wd = float(np.float32(momentum)), float(np.float32(lr)), wd_el[live].astype(np.float64)
    g1 = g + wd * p
    old = np.zeros_like(p) if first else host["b"][live].astype(np.float64)
    b = g1 if first else m * old + g1
    p1 = p - lr64 * b
    mb = 0.0 if first else m * np.abs(old)
    bound_b = 2 * U * (mb + np.abs(b) + np.abs(g1))
    bound_p = 2 * U * (np.abs(p1) + lr64 * (mb + np.abs(b) + np.abs(g1)))
    err_b, err_p = np.abs(out["b"][live] - b), np.abs(out["p"][live] - p1)
    assert np.isfinite(out["b"][live]).all() and np.isfinite(out["p"][live]).all()      # first_step ignores the NaN buffer
    with capsys.disabled():
        print("\n[sgd kernel m=%g first=%d lr=%g] worst |err|/bound: param %.3f, momentum %.3f"
              % (momentum, first, lr, float((err_p / bound_p).max()), float((err_b / np.maximum(bound_b, 1e-300)).max())))
    assert (err_b <= bound_b).all(), float((err_b / bound_b).max())
    assert (err_p <= bound_p).all(), float((err_p / bound_p).max())
    if lr == 0.0:
        assert np.array_equal(out["p"].view(np.int32), host["p"].view(np.int32))


# ---------------------------------------------------------------------------------------------- EIC kernel
def test_eic_kernel_bit_exact_on_long_layers_and_special_values(cuda):
    """eic_update_kernel, 130 layers in one launch, widths around and far beyond its 256-thread stride, three steps,
    against oracle.scoring.eic_step bit for bit: exact zeros, -0.0, sign flips, products g*gamma that are subnormal
    (flag = product > 0 as IEEE fp32 with denormals has it) or underflow to zero, subnormal scores, +-inf and NaN."""
    from dcfp_amd import _lib
    from dcfp_amd._lib import EicEntry
    widths = [[1, 255, 256, 257, 2048, 4099][i % 6] for i in range(130)]
    rng = np.random.RandomState(71)
    offs, off = [], 0
    for n in widths:
        off += int(rng.randint(1, 40))
        offs.append(off)
        off += n
    total = off + 32
    SENT = np.float32(-777.25)
    live = np.zeros(total, bool)
    for n, o in zip(widths, offs):
        live[o:o + n] = True

    def specials(n, kind):
        v = (rng.randn(n) * (0.05 if kind == "g" else 1.0)).astype(np.float32)
        pick = rng.randint(0, 16, n)
        v[pick == 0] = 0.0
        v[pick == 1] = -0.0
        v[pick == 2] = np.float32(1e-20) * np.sign(v[pick == 2])          # product of two of these: subnormal 1e-40
        v[pick == 3] = np.float32(1e-30) * np.sign(v[pick == 3])          # product of two: underflows to zero
        v[pick == 4] = np.float32(3e-39) * np.sign(v[pick == 4])          # subnormal itself
        if kind == "g":
            v[pick == 5] = np.inf
            v[pick == 6] = -np.inf
            v[pick == 7] = np.nan
        return v

    gamma = np.full(total, SENT, np.float32)
    for n, o in zip(widths, offs):
        gamma[o:o + n] = specials(n, "w")
    d_gamma = torch.from_numpy(gamma.copy()).to(cuda)
    d_grad = torch.full((total,), float(SENT), device=cuda)
    eic0 = np.full(total, SENT, np.float32)
    eic0[live] = 0.0
    d_eic = torch.from_numpy(eic0.copy()).to(cuda)
    entries = (EicEntry * len(widths))()
    for i, (n, o) in enumerate(zip(widths, offs)):
        e = entries[i]
        e.gamma, e.grad, e.eic, e.n = d_gamma.data_ptr() + 4 * o, d_grad.data_ptr() + 4 * o, d_eic.data_ptr() + 4 * o, n
    table = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8).to(cuda)
    r = 0.999
    ref = eic0.copy()
    seen_sub = 0
    for step in range(3):
        grad = np.full(total, SENT, np.float32)
        for n, o in zip(widths, offs):
            grad[o:o + n] = specials(n, "g")
        if step == 1:                                     # the same magnitudes with every sign flipped once
            grad[live] = -prev_grad[live]
        prev_grad = grad
        d_grad.copy_(torch.from_numpy(grad))
        _lib.check(_lib.lib().dcfp_eic_update_f32(C.c_void_p(table.data_ptr()), len(widths), float(r), float(1 - r),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "eic")
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            prod = grad[live] * gamma[live]
            seen_sub += int(((np.abs(prod) > 0) & (np.abs(prod) < np.float32(1.1754944e-38))).sum())
            ref[live] = scoring.eic_step(gamma[live], grad[live], ref[live], r)
        mine = d_eic.cpu().numpy()
        assert np.array_equal(mine[~live].view(np.int32), eic0[~live].view(np.int32)), step
        bad = np.nonzero(~((mine[live] == ref[live]) | (np.isnan(mine[live]) & np.isnan(ref[live]))))[0]
        assert bad.size == 0, (step, bad[:5], mine[live][bad[:5]], ref[live][bad[:5]], grad[live][bad[:5]],
                               gamma[live][bad[:5]])
        assert np.array_equal(mine[live], ref[live], equal_nan=True)
    assert seen_sub > 1000                                # the subnormal-product branch really was exercised
    assert np.isnan(ref[live]).any() and np.isinf(ref[live]).any() and (ref[live] == 0).any()
    sub = np.abs(ref[live])
    assert ((sub > 0) & (sub < np.float32(1.1754944e-38))).any()          # subnormal scores


# ---------------------------------------------------------------------------------------------- FusedSGD transitions
SHAPES = [(7,), (16383,), (16385,), (3, 5, 3, 3), (1,), (40000,), (16384,), (255,)]
GROUP_OF = [0, 0, 0, 0, 0, 1, 1, 1]
BASE_LR, MOM, WD, STEPS = 0.05, 0.9, 5e-4, 6


def _grad(step, i):
    g = torch.Generator().manual_seed(100 * step + i + 1)
    return torch.randn(SHAPES[i], generator=g) * 0.5


def _init(i):
    g = torch.Generator().manual_seed(9000 + i)
    return torch.randn(SHAPES[i], generator=g)


class _Run:
    """One optimizer driven through a script of steps; the same driver serves FusedSGD on the GPU and torch.optim.SGD on
    the CPU (gradients are handed over the way the backward kernels do: into the arena's view where there is one)."""

    def __init__(self, factory, device, dtype):
        self.factory, self.device, self.dtype = factory, device, dtype
        self.params = [torch.nn.Parameter(_init(i).to(device=device, dtype=dtype)) for i in range(len(SHAPES))]
        self.opt = self._make(self.params)
        self.fresh_state = self.opt.state_dict()          # of an optimizer that never stepped
        self.history = []
        self.floor = [torch.zeros(s, dtype=torch.float64) for s in SHAPES]

    def _make(self, params):
        groups = [{"params": [p for p, gi in zip(params, GROUP_OF) if gi == 0]},
                  {"params": [p for p, gi in zip(params, GROUP_OF) if gi == 1], "weight_decay": 0.0}]
        return self.factory(groups, lr=BASE_LR, momentum=MOM, weight_decay=WD)

    def give(self, p, g):
        from dcfp_amd import arena
        g = g.to(device=self.device, dtype=self.dtype)
        t, token = arena.grad_target(p)
        t.copy_(g)
        out = arena.grad_commit(p, t, token)
        if out is not None:                               # what autograd's AccumulateGrad does with a returned gradient
            p.grad = out if p.grad is None else p.grad + out

    def resume(self):
        sd = self.opt.state_dict()
        self.params = [torch.nn.Parameter(p.detach().clone()) for p in self.params]
        self.opt = self._make(self.params)
        self.opt.load_state_dict(sd)

    def step(self, it, spec):
        from dcfp_amd import optimizer as om
        for ev in spec.get("before", ()):
            if ev == "resume":
                self.resume()
            elif ev == "load_fresh":
                self.opt.load_state_dict(self.fresh_state)
            elif ev == "load_partial":                        # the state of parameters 1 and 5 is missing from the checkpoint
                sd = self.opt.state_dict()
                self.opt.load_state_dict({"state": {k: v for k, v in sd["state"].items() if k not in (1, 5)},
                                          "param_groups": sd["param_groups"]})
            elif ev == "move_out":
                for i in (1, 5):
                    self.params[i].data = self.params[i].data.clone()
            elif ev[0] == "wd":
                self.opt.param_groups[ev[1]]["weight_decay"] = ev[2]
        self.opt.zero_grad(set_to_none=spec.get("to_none", True))
        om.adjust_learning_rate(self.opt, BASE_LR, it, 20, 0.9, -1)
        for i, p in enumerate(self.params):
            if i not in spec.get("no_grad", ()):
                self.give(p, _grad(it, i))
        if self.dtype == torch.float64:
            self._floor_terms()
        self.opt.step()
        self.history.append([p.detach().cpu().clone() for p in self.params])

    def _floor_terms(self):
        """The per-element roundoff bound of one update (test_sgd_kernel_against_fp64_per_element), from the fp64 run's
        values, summed over the steps: the floor below which a difference says nothing."""
        for gi, group in enumerate(self.opt.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                i = next(k for k, q in enumerate(self.params) if q is p)
                buf = self.opt.state.get(p, {}).get("momentum_buffer")
                g1 = p.grad + group["weight_decay"] * p.detach()
                mb = torch.zeros_like(g1) if buf is None else MOM * buf.abs()
                b = g1 if buf is None else MOM * buf + g1
                p1 = p.detach() - group["lr"] * b
                self.floor[i] += 2 * U * (p1.abs() + group["lr"] * (mb + b.abs() + g1.abs()))


def _fused(cuda):
    from dcfp_amd.optimizer import FusedSGD
    return _Run(FusedSGD, cuda, torch.float32)


def _drive(run, script):
    for it, spec in enumerate(script):
        run.step(it, spec)
    if run.device != torch.device("cpu"):
        torch.cuda.synchronize()
    return run


def _against_torch(cuda, capsys, label, script):
    """|FusedSGD - fp64| <= 3 x |torch.optim.SGD fp32 - fp64| per tensor and step (floor: the summed roundoff bound)."""
    mine = _drive(_fused(cuda), script)
    t64 = _drive(_Run(torch.optim.SGD, torch.device("cpu"), torch.float64), script)
    t32 = _drive(_Run(torch.optim.SGD, torch.device("cpu"), torch.float32), script)
    worst = 0.0
    for it in range(len(script)):
        for i in range(len(SHAPES)):
            ref = t64.history[it][i]
            err = float((mine.history[it][i].double() - ref).abs().max())
            spread = float((t32.history[it][i].double() - ref).abs().max())
            floor = float(t64.floor[i].max())
            worst = max(worst, err / max(spread, floor / 3, 1e-300))
            assert err <= max(3 * spread, floor), (label, it, i, err, spread, floor)
    with capsys.disabled():
        print("\n[FusedSGD %s] worst |mine - fp64| / |torch fp32 - fp64| over %d steps x %d tensors: %.2f (bound 3)"
              % (label, len(script), len(SHAPES), worst))
    return mine


def test_fused_sgd_poly_lr_steady_state(cuda, capsys):
    run = _against_torch(cuda, capsys, "poly lr, set_to_none", [{} for _ in range(STEPS)])
    assert run.opt.table_rebuilds == 2                    # one upload per group, however often the lr changes
    run = _against_torch(cuda, capsys, "poly lr, in-place zero_grad", [{"to_none": False} for _ in range(STEPS)])
    assert run.opt.table_rebuilds == 2


def test_fused_sgd_late_and_missing_gradients(cuda, capsys):
    """Parameter 2 has no gradient on steps 0-2 (its momentum starts with its first gradient, at step 3); parameter 6
    loses its gradient at step 4: skipped after zero_grad(set_to_none=True), a step on zeros after the in-place flavour.
    (The late gradient runs with set_to_none only: the arena's in-place zero_grad attaches a zeroed view to EVERY
    parameter, so there a parameter that never had a gradient takes steps on zeros where torch leaves it alone.)"""
    script = [{"no_grad": (2,)}, {"no_grad": (2,)}, {"no_grad": (2,)}, {}, {"no_grad": (6,)}, {}]
    run = _against_torch(cuda, capsys, "late / missing gradients", script)
    assert torch.equal(run.history[2][2], _init(2))       # untouched until its first gradient
    script = [{}, {}, {}, {}, {"no_grad": (6,)}, {}]
    _against_torch(cuda, capsys, "missing gradient, in-place zero_grad", [dict(s, to_none=False) for s in script])
    mixed = [dict(s, to_none=bool(it % 2)) for it, s in enumerate(script)]
    _against_torch(cuda, capsys, "missing gradient, both zero_grad flavours", mixed)


def test_fused_sgd_weight_decay_change_rebuilds_the_table(cuda, capsys):
    script = [{}, {}, {}, {"before": [("wd", 0, 1e-3), ("wd", 1, 2e-4)]}, {}, {}]
    run = _against_torch(cuda, capsys, "weight decay change", script)
    assert run.opt.table_rebuilds == 4


def test_fused_sgd_resume_is_bit_identical(cuda, capsys):
    script = [{}, {}, {}, {"before": ["resume"]}, {}, {}]
    resumed = _against_torch(cuda, capsys, "save / resume", script)
    straight = _drive(_fused(cuda), [{} for _ in range(STEPS)])
    for it in range(STEPS):
        for i in range(len(SHAPES)):
            assert torch.equal(resumed.history[it][i], straight.history[it][i]), (it, i)


def test_fused_sgd_loading_a_never_stepped_state_restarts_momentum(cuda, capsys):
    """load_state_dict of a state without momentum buffers (a checkpoint taken before the first step) after two steps:
    momentum restarts from zero, as in torch.optim.SGD - not from what the arena's momentum buffer still holds."""
    script = [{}, {}, {"before": ["load_fresh"]}, {}, {}, {}]
    _against_torch(cuda, capsys, "never-stepped state loaded after 2 steps", script)
    script = [{}, {}, {"before": ["load_partial"]}, {}, {}, {}]
    _against_torch(cuda, capsys, "partial state loaded after 2 steps", script)


def test_fused_sgd_parameters_moved_out_of_the_arena_keep_their_momentum(cuda, capsys):
    script = [{}, {}, {}, {"before": ["move_out"]}, {}, {}]
    moved = _against_torch(cuda, capsys, "parameters moved out of the arena", script)
    straight = _drive(_fused(cuda), [{} for _ in range(STEPS)])
    for i in range(len(SHAPES)):
        assert torch.equal(moved.history[-1][i], straight.history[-1][i]), i
