"""CPU: the table of tests/_align.py against the host functions of the built library, and the helper itself.
(a) every row of CONV / WGRAD routes where it says and is vector-eligible, so that tests/test_alignment_gpu.py moves
operands off the 16-byte grid on shapes that take the 16-byte paths when aligned; (b) the table is complete: every
forward, data-gradient and weight-gradient kernel name that tests/_wp_cases.CASES and tests/_narrow_cases.NARROW can
produce has a row, so a new route cannot go untested; (c) every kernel name of the table is classed - LDS-DMA (a
displaced source must not reach it) or register-staged; (d) the host queries that take a pointer answer by its
alignment; (e) displaced() places its copies where it says and guards_intact() sees a single changed word."""
import ctypes as C

import torch

import _align as al
import _narrow_cases as nc
import _wp_cases as wp

FWD, DGRAD, WGRAD = 0, 1, 2


def _desc(case, xp=0, dp=0):
    from dcfp_amd import ops
    N, Cin, H, W, Cout, k, s, p, d = case
    return ops._desc((N, Cin, H, W), (Cout, Cin, k, k), s, p, d, xp, dp)


def test_every_row_routes_as_written():
    from dcfp_amd import ops
    seen = set()
    for case, fwd, dgrad in al.CONV:
        assert case not in seen, case
        seen.add(case)
        assert al.vector_eligible(case), case
        pitch = nc.NARROW_PITCH.get(case, 0)
        assert pitch == nc.pitch_of(case) or not pitch, case
        d = _desc(case, pitch, pitch)
        for which, want in ((FWD, fwd), (DGRAD, dgrad)):
            assert want is None or ops.conv_kernel_name(d, which) == want, (case, which, ops.conv_kernel_name(d, which), want)
    assert set(nc.NARROW_PITCH) <= seen and set(al.OPTION_ROWS) <= seen
    seen = set()
    for case, name, xp, flags in al.WGRAD:
        assert case not in seen, case
        seen.add(case)
        assert al.vector_eligible(case), case
        assert ops.conv_kernel_name(_desc(case, xp, 0), WGRAD) == name, (case, ops.conv_kernel_name(_desc(case, xp, 0), WGRAD))
        assert set(flags.split()) <= {"bias", "splits", "kept"}
    assert ops.conv_kernel_name(_desc(al.FANIN_ROW), DGRAD) == al.DMA1P
    assert ops.conv2d_dgrad_fanin_ok(None, torch.empty(al.FANIN_ROW[4], al.FANIN_ROW[1], 1, 1), al.FANIN_ROW[:4])


def test_the_rows_the_issue_names_are_there():
    from dcfp_amd import _lib, ops
    L = _lib.lib()
    flags = {f for *_, fl in al.WGRAD for f in fl.split()}
    assert flags == {"bias", "splits", "kept"}
    for case, name, xp, fl in al.WGRAD:
        d = _desc(case, xp, 0)
        N, Cin, H, W, Cout, k = case[:6]
        if "splits" in fl:      # several split-K slabs and a weight tensor of whole quads: the vector reduce when aligned
            assert (Cout * Cin * k * k) % 4 == 0
            assert L.dcfp_conv2d_workspace_bytes(C.byref(d), WGRAD) >= 2 * Cout * Cin * k * k * 4
        if "kept" in fl:        # the forward can leave its transformed input behind
            assert L.dcfp_conv2d_xform_bytes(C.byref(d)) > 0 and name == al.WINO_WG
    names = {n for _, n, _, _ in al.WGRAD}
    assert {al.WINO_WG_FUSED, al.WINO_WG, al.STEM_WG, al.GEMV, al.WG1, al.WIDE1, al.WIDE9} <= names
    assert ((2, 3, 64, 128, 64, 3, 2, 1, 1), al.STEM_WG, 0, "") in al.WGRAD
    opt = {ops.conv_kernel_name(_desc(c), FWD) for c in al.OPTION_ROWS}
    assert opt == {al.DMA1P, al._ig(1, al._T2), al.WINO_FUSED}, opt


def test_table_covers_every_kernel_name_the_case_tables_produce():
    have = {n for _, f, g in al.CONV for n in (f, g)} - {None}
    missing = al.conv_names() - have
    assert not missing, f"forward / dgrad kernels without an alignment row: {sorted(missing)}"
    have_wg = {n for _, n, _, _ in al.WGRAD}
    missing = al.wgrad_names() - have_wg
    assert not missing, f"weight-gradient kernels without an alignment row: {sorted(missing)}"
    # the enumeration is not vacuous
    assert len(al.conv_names()) >= 20 and len(al.wgrad_names()) >= 7
    # and goes through the library: a name the library stops producing would be caught by the row test, a new one here
    for case, fwd, dgrad in wp.CASES[:3]:
        assert wp.kernel_name(wp.desc_of(case), wp.FWD) == fwd


def test_every_kernel_of_the_table_is_classed():
    """LDS-DMA (copies 16 bytes at a time from its source: tests/test_alignment_gpu.py compares a displaced call with the
    child that has no such kernels) or register-staged (any 4-byte aligned address: the bits of the aligned call)."""
    for _, f, g in al.CONV:
        for n in (f, g):
            if n is None or n in al.LDS_DMA:
                continue
            assert n.startswith("igemm2_kernel<") or n in (al.STEM, al.GEMV), n
    for n in al.LDS_DMA:
        assert "dma" in n or "winograd" in n
    for _, n, _, _ in al.WGRAD:
        if n not in al.WGRAD_LDS_DMA:
            assert n.startswith("wgrad2_kernel<") or n in (al.STEM_WG, al.GEMV), n
    for n in al.WGRAD_LDS_DMA:
        assert "dma" in n or "winograd" in n


def test_statistics_slots_follow_the_alignment_of_y():
    """dcfp_conv2d_fwd_stat_slots is a host function of (descriptor, y, image stride): no statistics epilogue for a y
    the 16-byte epilogue cannot store to - the stem included, whose kernel has no other store."""
    from dcfp_amd import _lib
    L = _lib.lib()
    rows = [(2, 40, 128, 192, 256, 1, 1, 0, 1), (2, 96, 96, 160, 200, 3, 1, 4, 4), (2, 3, 64, 128, 128 // 2, 3, 2, 1, 1),
            (2, 3, 64, 256, 64, 3, 2, 1, 1)]
    got = 0
    for case in rows:
        d = _desc(case)
        on = L.dcfp_conv2d_fwd_stat_slots(C.byref(d), C.c_void_p(0x10000), 0)
        if on <= 0:
            continue
        got += 1
        for k in (1, 2, 3):
            assert L.dcfp_conv2d_fwd_stat_slots(C.byref(d), C.c_void_p(0x10000 + 4 * k), 0) == 0, (case, k)
        Cout, Ho, Wo = d.Cout, d.Hout, d.Wout
        assert L.dcfp_conv2d_fwd_stat_slots(C.byref(d), C.c_void_p(0x10000), (Cout + 1) * Ho * Wo) == on      # whole quads
        assert L.dcfp_conv2d_fwd_stat_slots(C.byref(d), C.c_void_p(0x10000), Cout * Ho * Wo + 2) == 0, case
    assert got >= 3


def test_workspace_queries_cover_the_fallbacks():
    """A call with an operand off the grid runs another kernel in the workspace the descriptor-level query sized: the
    direct kernel's permuted copy under a fused Winograd conv, the general weight gradient under the stem's."""
    from dcfp_amd import _lib
    L = _lib.lib()
    wino = _desc((2, 96, 96, 160, 200, 3, 1, 4, 4))
    for which in (FWD, DGRAD):
        M, Ck = (200, 96) if which == FWD else (96, 200)
        ck = (Ck + 15) // 16 * 16
        assert L.dcfp_conv2d_workspace_bytes(C.byref(wino), which) >= 9 * ck * 256 * 4
    stem = _desc((2, 3, 64, 128, 64, 3, 2, 1, 1))
    assert L.dcfp_conv2d_workspace_bytes(C.byref(stem), WGRAD) > 0


def test_displaced_places_and_guards():
    for k in (1, 2, 3):
        t = torch.randn(2, 3, 5, 8)
        g = al.displaced(t, k)
        assert g.view.data_ptr() % 16 == 4 * k and g.view.is_contiguous() and torch.equal(g.view, t) and g.guards_intact()
        assert g.buf.numel() >= t.numel() + 128 and g.unwritten() == 0
        for where in (0, 63, g.buf.numel() - 1):
            g.buf[where] = 0.0
            assert not g.guards_intact(), where
            g.buf.view(torch.int32)[where] = al.GUARD_BITS
            assert g.guards_intact()
        # a quiet NaN is not the guard: bits are compared
        g.buf[1] = float("nan")
        assert not g.guards_intact()
        e = al.displaced_empty((4, 6), k)
        assert e.view.data_ptr() % 16 == 4 * k and e.unwritten() == 24 and bool(torch.isnan(e.view).all())
        e.view[1, 2] = 1.0
        assert e.unwritten() == 23 and e.guards_intact()
        s = al.displaced_slice((2, 3, 5, 8), k, 2, 7, src=t)
        assert torch.equal(s.view, t) and s.guards_intact() and s.view.stride() == (7 * 40, 40, 8, 1)
        assert (s.view.data_ptr() - 4 * 2 * 40) % 16 == 4 * k
        s.buf[s._spans[0][1]] = 1.0           # the first float of the next channel, between the two images' slices
        assert not s.guards_intact()
        p = al.displaced_pitched(t, k, 12)
        assert p.view.data_ptr() % 16 == 4 * k and torch.equal(p.view, t) and p.guards_intact()
        assert p.view.stride() == (3 * 5 * 12, 5 * 12, 12, 1)
        full = p.view.as_strided((2, 3, 5, 12), p.view.stride(), p.view.storage_offset())
        assert float(full[..., 8:].abs().max()) == 0.0                          # zero tails
        lead = p.view.as_strided((4,), (1,), p.view.storage_offset() - 4)
        assert float(lead.abs().max()) == 0.0                                   # pitch - W readable zeros in front
    from dcfp_amd import ops
    assert ops._pitch_of(al.displaced_pitched(torch.randn(2, 3, 5, 8), 1, 12).view) == 12
    assert al.displaced(torch.randn(5), 0).view.data_ptr() % 16 == 0


def test_ops_keys_kept_copies_by_alignment():
    """A call whose source or output is off the grid falls back to a kernel with another layout of the permuted weights:
    ops keeps that copy under a key of its own, never in the buffer the aligned call trusts (wp_valid)."""
    from dcfp_amd import ops
    assert ops._grid_variant(True, True) == ""
    assert len({ops._grid_variant(a, b) for a in (True, False) for b in (True, False)}) == 4
    t = al.displaced(torch.randn(2, 4, 4, 4), 1).view
    assert not ops._on_grid(t, 64) and ops._on_grid(torch.randn(2, 4, 4, 4), 64) and not ops._on_grid(torch.randn(8), 6)
