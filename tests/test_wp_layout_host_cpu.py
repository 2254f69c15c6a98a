"""CPU: the host functions that decide where a conv keeps its permuted / transformed weight copy.

ops.refresh_wp() rebuilds every kept copy from dcfp_conv2d_wp_layout's description while the conv itself builds the same
copy on demand (wp_valid = 0) into a buffer of dcfp_conv2d_workspace_bytes: (a) over a seeded descriptor sweep the
description always fits that buffer, its block count is the one the refresh kernel's grid assumes and its padding and row
permutation are self-consistent; (b) the case table the GPU test runs (tests/_wp_cases.py) routes where it says and
covers every forward / dgrad kernel the sweep meets on a kept copy."""
import ctypes as C

import pytest

from _wp_cases import CASES, FWD, DGRAD, UNUSED_COPY, block_count, desc_of, extent_bytes, keeps_copy, kernel_name, \
    layout, sweep

WP_BLOCK_ELEMS = 2048          # DCFP_WP_BLOCK_ELEMS of include/dcfp_hip.h
SWEEP = sweep(4000, 20261018)


@pytest.fixture(scope="module")
def swept():
    """[(case, pass, kernel name, WpEntry, workspace bytes)] for every (descriptor, pass) of the sweep with a layout."""
    from dcfp_amd import _lib
    L = _lib.lib()
    out = []
    for case in SWEEP:
        d = desc_of(case)
        for which in (FWD, DGRAD):
            rc, e = layout(d, which)
            if rc != 0:
                continue
            out.append((case, which, kernel_name(d, which), e, L.dcfp_conv2d_workspace_bytes(C.byref(d), which),
                        L.dcfp_conv2d_workspace_is_scratch(C.byref(d), which)))
    return out


def test_header_block_size_is_the_one_assumed_here():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "dcfp_hip.h")).read()
    assert int(re.search(r"#define\s+DCFP_WP_BLOCK_ELEMS\s+(\d+)", src).group(1)) == WP_BLOCK_ELEMS


def test_layout_fits_the_workspace_over_a_sweep(swept):
    assert len(swept) > 4000, len(swept)          # most descriptors have a layout in both passes
    fams = {}
    for case, which, name, e, nbytes, scratch in swept:
        ctx = (case, which, name, (e.T, e.Ck, e.CkP, e.M, e.Mpad, e.perm8), nbytes)
        assert not scratch, ctx                                   # a described copy is a kept one
        assert extent_bytes(e) <= nbytes, ctx
        elems = e.CkP * e.Mpad * (1 if e.perm8 >= 2 else e.T)
        assert e.n_blocks == (elems + WP_BLOCK_ELEMS - 1) // WP_BLOCK_ELEMS == block_count(e), ctx
        assert e.Mpad >= e.M and e.CkP >= e.Ck, ctx
        assert e.perm8 in (0, 1, 2, 3), ctx
        if e.perm8 == 1:
            assert e.Mpad % 256 == 0, ctx
        if e.perm8 >= 2:
            assert e.T == 16 and name.startswith("winograd_f2x2_3x3"), ctx
        else:
            assert e.T == case[5] * case[5], ctx
        assert (e.perm8 == 1) == name.startswith("igemm2_dma8_kernel"), ctx
        N, Cin, H, W, Cout, k, s, p, d = case
        assert (e.M, e.Ck) == ((Cout, Cin) if which == FWD else (Cin, Cout)), ctx
        # element (m, c, t) of the copy is w[m*sAm + c*sAc + t] of the [Cout, Cin, k, k] tensor
        assert (e.sAm, e.sAc) == ((Cin * k * k, k * k) if which == FWD else (k * k, Cin * k * k)), ctx
        fams[name] = fams.get(name, 0) + 1
    # the sweep is wide enough to mean something: every perm8 value and a spread of kernels
    assert {e.perm8 for _, _, _, e, _, _ in swept} == {0, 1, 2, 3}
    assert len(fams) >= 20, sorted(fams)


def test_case_table_routes_as_written_and_covers_the_sweep(swept):
    table = set()
    for case, fwd, dgrad in CASES:
        d = desc_of(case)
        for which, want in ((FWD, fwd), (DGRAD, dgrad)):
            if want is None:
                continue
            assert kernel_name(d, which) == want, (case, which, kernel_name(d, which))
            assert keeps_copy(d, which), (case, which)
            table.add(want)
    met = {name for _, _, name, _, _, _ in swept}
    assert table == met, (sorted(table - met), sorted(met - table))
    assert set(UNUSED_COPY) <= table


def test_case_table_block_counts_span_one_to_hundreds():
    """The one-launch test needs entries of one block and of hundreds for the refresh kernel's binary search."""
    counts = []
    for case, fwd, dgrad in CASES:
        d = desc_of(case)
        counts += [layout(d, which)[1].n_blocks for which, want in ((FWD, fwd), (DGRAD, dgrad)) if want is not None]
    assert min(counts) == 1 and max(counts) >= 256 and len(counts) >= 25, sorted(counts)
