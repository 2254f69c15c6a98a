"""CPU: which kernels the 1-, 2- and 5-channel layers of a pruned model reach, from the host functions of the built
library.  (a) every row of tests/_narrow_cases.NARROW routes where it says, with the row pitch it says; (b) the table is
complete: every (pass, kernel, narrow side) class that a conv of any golden prune fixture meets at the training and the
full-size geometry has a row; (c) the enumeration behind (b) is not vacuous; (d) the rows with dense operands are part of
tests/_wp_cases.CASES, so the kept-weight-copy tests refresh and replay them."""
import ctypes as C

import _narrow_cases as nc
import _wp_cases as wp


def _met():
    """{class: (fixture, geometry, layer, case)} - one real layer per class."""
    met = {}
    for path in nc.fixtures():
        for geo in nc.GEOMETRIES:
            for layer, case in nc.slim_convs(path, geo, named=True):
                for cls in nc.classes_of(case):
                    met.setdefault(cls, (path.rsplit("/", 1)[-1], geo, layer, case))
    return met


def test_every_row_routes_as_written():
    seen = set()
    for case, fwd, dgrad, wgrad in nc.NARROW:
        assert case not in seen, case
        seen.add(case)
        N, Cin, H, W, Cout, k, s, p, d = case
        assert min(Cin, Cout) <= 9, case                      # (9: the far side of the 8-channel granule)
        assert nc.pitch_of(case) == nc.NARROW_PITCH.get(case, 0), (case, nc.pitch_of(case))
        got = nc.routes(case)
        for which, want in enumerate((fwd, dgrad, wgrad)):
            assert want is None or got[which] == want, (case, nc.PASS_NAMES[which], got[which], want)
    assert set(nc.NARROW_PITCH) <= seen and nc.STATS <= seen


def test_table_covers_every_class_the_slim_models_meet():
    met = _met()
    table = set()
    for case, fwd, dgrad, wgrad in nc.NARROW:
        table |= nc.classes_of(case, (fwd, dgrad, wgrad))
    missing = {cls: met[cls] for cls in met if cls not in table}
    assert not missing, "classes without a NARROW row:\n" + "\n".join(f"  {c}: {m}" for c, m in sorted(missing.items()))


def test_enumeration_is_not_vacuous():
    met = _met()
    widths = set()
    n = 0
    for path in nc.fixtures():
        assert path.rsplit("_gp", 1)[0].rsplit("prune_", 1)[1] in nc.MODELS, path
        for geo in nc.GEOMETRIES:
            for case in nc.slim_convs(path, geo):
                widths.add(min(case[1], case[4]))
                n += 1
    assert len(nc.fixtures()) >= 6 and n >= 100, (len(nc.fixtures()), n)
    assert {1, 2, 5} <= widths, widths
    for p in nc.PASS_NAMES:
        for side in "MK":
            assert any(c[0] == p and c[2] == side for c in met), (p, side, sorted(met))
    # both geometries matter: the LDS-DMA kernels are reached at the full-size maps only, the large register-staged
    # tiles at the training maps (odd widths) only
    kernels = {c[1] for c in met}
    assert {nc.D8_1, nc.D8_9, nc.DMA1P, nc.WIDE1, nc.WIDE9, nc.GEMV, nc._ig(1, nc._T4), nc._ig(9, nc._T5)} <= kernels, kernels


def test_a_renamed_layer_cannot_drop_out_of_the_enumeration(tmp_path):
    """Every name of a fixture (and every name with an in_n: / out_n: entry) resolves to a Conv2d or a BatchNorm2d of the
    model definition, or slim_convs raises."""
    import numpy as np
    import pytest
    src = [p for p in nc.fixtures() if p.endswith("prune_v3r50_gp50.npz")][0]
    g = dict(np.load(src))
    for victim in ("backbone.layer2.0.conv1", "backbone.layer3.1.conv2"):
        renamed = {}
        for k, v in g.items():
            renamed[k.replace(victim, victim + "_renamed")] = v
        renamed["names"] = np.array([n.replace(victim, victim + "_renamed") if n == victim else n for n in g["names"].tolist()])
        path = str(tmp_path / "prune_v3r50_gp50.npz")
        np.savez(path, **renamed)
        with pytest.raises(KeyError, match="_renamed"):
            list(nc.slim_convs(path, "train"))
    # an entry whose name is missing from `names` is looked at all the same
    extra = dict(g)
    extra["out_n:backbone.layer9.0.conv1"] = g["out_n:backbone.layer2.0.conv1"]
    np.savez(path, **extra)
    with pytest.raises(KeyError, match="layer9"):
        list(nc.slim_convs(path, "train"))


def test_flip_allowance_is_the_existing_share():
    assert abs(nc.FLIP_RATE - 2.47e-7) < 1e-9
    assert [nc.flip_allowance(n) for n in (234, 3999, 35904, 4227072, 4718592, 26148864)] == [0, 0, 1, 5, 6, 16]


def test_required_routes_are_in_the_table():
    """The routes that matter at narrow widths whether or not a fixture layer happens to take them."""
    have = set()
    for case, fwd, dgrad, wgrad in nc.NARROW:
        have |= nc.classes_of(case, (fwd, dgrad, wgrad))
        N, Cin, H, W, Cout, k, s, p, d = case
        have |= {("dil", d, side) for side in nc.sides(case, nc.FWD) if k == 3}
        have |= {("nn", wgrad, Cin * k * k)}
        have |= {("cout", wgrad, Cout), ("cout", fwd, Cout)}
    for want in [("dgrad", nc._ig(9, nc._T5), "M"), ("dgrad", nc._ig(9, nc._T5), "K"),
                 ("dil", 2, "M"), ("dil", 2, "K"), ("dil", 4, "M"), ("dil", 4, "K"),
                 ("cout", nc.WIDE1, 1), ("nn", nc.WG1, 1), ("nn", nc.WG9, 9),
                 ("nn", "wgrad2_kernel<9,4,1,2,2>", 45), ("nn", "wgrad2_kernel<9,4,2,2,2>", 72), ("cout", nc.GEMV, 5)]:
        assert want in have, want
    # 3, 7, 8 and 9 on the reduction side of every pass
    for c in (3, 7, 8, 9):
        assert any(case[1] == c and case[5] == 3 for case, *_ in nc.NARROW), c          # forward K = 9c, wgrad Nn = 9c
        assert any(case[4] == c and case[5] == 1 for case, *_ in nc.NARROW), c          # dgrad K = c
    # both orientations of each layer pair
    for c in (1, 2, 5):
        for k in (1, 3):
            ins = [case for case, *_ in nc.NARROW if case[1] == c and case[5] == k]
            outs = [case for case, *_ in nc.NARROW if case[4] == c and case[5] == k]
            assert ins and outs, (c, k)


def test_statistics_rows_are_the_ones_the_library_offers():
    from dcfp_amd import _lib
    L = _lib.lib()
    for case, *_ in nc.NARROW:
        d = nc.desc_of(case)
        slots = L.dcfp_conv2d_fwd_stat_slots(C.byref(d), None, 0)
        assert (slots > 0) == (case in nc.STATS), (case, slots)
        if case[4] <= nc.NARROW_MAX:
            assert slots == 0, case                            # a narrow Cout never has all-live tiles


def test_per_channel_figure_sees_what_a_whole_tensor_norm_hides():
    """The GPU file's judge (_narrow_cases.per_channel) on mutated CPU results - ATen's fp32 conv stands in for
    a kernel that is right: (a) one output channel of 129 off by 2e-5 relative moves the whole-tensor norm by 2e-5 / sqrt(129)
    = 1.8e-6, inside the forward bound 3e-6, and the per-channel figure by 6.7 bounds; (b) a width-1 slice written one
    float late (its base rounded to the next 4-float boundary and then some) is an O(1) error in that channel alone;
    (c) a K tail read unzeroed - one stray product added to every output of one channel of five."""
    import torch
    import torch.nn.functional as F
    _per_channel = nc.per_channel
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(2, 5, 20, 31, generator=g), torch.randn(129, 5, 1, 1, generator=g) / 5 ** 0.5
    y64, y32 = F.conv2d(x.double(), w.double()), F.conv2d(x, w)
    tol = nc.tolerance((2, 5, 20, 31, 129, 1, 1, 0, 1))
    assert tol == 3e-6
    assert _per_channel(y32, y64, y32, 1, tol)[1] <= 1.0                       # the stand-in passes
    bad = y32.clone()
    bad[:, 77] *= 1.0 + 2e-5
    whole = float((bad.double() - y64).norm() / y64.norm())
    assert whole < tol                                                         # (a) invisible to the whole-tensor norm
    assert _per_channel(bad, y64, y32, 1, tol)[1] > 5.0
    w5 = torch.randn(5, 9, 3, 3, generator=g) / 9.0
    x9 = torch.randn(2, 9, 12, 15, generator=g)
    z64, z32 = F.conv2d(x9.double(), w5.double(), None, 1, 1), F.conv2d(x9, w5, None, 1, 1)
    tol = nc.tolerance((2, 9, 12, 15, 5, 3, 1, 1, 1))
    late = z32.clone()
    late[0, 1] = torch.roll(z32[0, 1].reshape(-1), 1).reshape(12, 15)          # (b)
    assert _per_channel(late, z64, z32, 1, tol)[1] > 1e4
    stray = z32.clone()
    stray[:, 3] += 1e-4 * x9[:, 0]                                             # (c)
    assert float((stray.double() - z64).norm() / z64.norm()) < 1e-4 and _per_channel(stray, z64, z32, 1, tol)[1] > 10.0
    # dw: one wrong filter row of 5 and one wrong input-channel column of 9
    dy = torch.randn(z32.shape, generator=g) + 0.5
    dw64 = torch.nn.grad.conv2d_weight(x9.abs().double(), w5.shape, dy.double(), 1, 1)
    dw32 = torch.nn.grad.conv2d_weight(x9.abs(), w5.shape, dy, 1, 1)
    assert _per_channel(dw32, dw64, dw32, 0, 2e-5)[1] <= 1.0 and _per_channel(dw32, dw64, dw32, 1, 2e-5)[1] <= 1.0
    m = dw32.clone(); m[2] *= 1.0 + 3.5e-5
    assert float((m.double() - dw64).norm() / dw64.norm()) < 2e-5 and _per_channel(m, dw64, dw32, 0, 2e-5)[1] > 1.5
    m = dw32.clone(); m[:, 6] *= 1.0 + 5e-5
    assert float((m.double() - dw64).norm() / dw64.norm()) < 2e-5 and _per_channel(m, dw64, dw32, 1, 2e-5)[1] > 2.0


def test_dense_rows_are_in_the_kept_copy_table():
    in_table = {case: (fwd, dgrad) for case, fwd, dgrad in wp.CASES}
    n = 0
    for case, fwd, dgrad, _ in nc.NARROW:
        if case in nc.NARROW_PITCH:
            assert case not in in_table, case                  # (that table's descriptors are dense)
            continue
        assert in_table.get(case) == (fwd, dgrad), (case, in_table.get(case))
        d = wp.desc_of(case)
        for which, want in ((wp.FWD, fwd), (wp.DGRAD, dgrad)):
            assert wp.kernel_name(d, which) == want and wp.keeps_copy(d, which), (case, which)
        n += 1
    assert n >= 40
    # the padded copy is many times the live extent at these widths
    rc, e = wp.layout(wp.desc_of((2, 1, 9, 13, 19, 1, 1, 0, 1)), wp.DGRAD)
    assert rc == 0 and (e.M, e.Ck, e.Mpad, e.CkP) == (1, 19, 32, 32)
    rc, e = wp.layout(wp.desc_of((2, 133, 128, 192, 2, 1, 1, 0, 1)), wp.FWD)
    assert rc == 0 and (e.M, e.Mpad, e.perm8) == (2, 256, 1)
