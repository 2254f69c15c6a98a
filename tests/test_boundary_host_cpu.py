"""CPU: the host side of the label-boundary transform - the brute-force reference against a
closed form, boundary_dilation, the launchers' validation (which runs before any HIP call), the missing CPU path,
and the conditions the GPU cases must meet so that none of them compares background against background."""
import ctypes

import numpy as np
import pytest
import torch

import _boundary_ref as R


def test_reference_closed_form_probe():
    out = R.reference(R.probe(), 19, 4, 255)
    assert int((out != 255).sum()) == 41 * 53 - 33 * 45 + 81 == 769
    assert int((out == 5).sum()) == 1 and out[20, 30] == 5
    assert set(np.unique(out).tolist()) == {3, 5, 255}
    assert (out[4:16, 4:26] == 255).all() and (out[:4] == 3).all() and (out[16:25, 26:35] != 255).all()


def test_reference_invalid_values_erode_and_come_out_as_background():
    l = np.full((9, 9), 2, dtype=np.int32)
    l[4, 4] = -1
    out = R.reference(l, 19, 1, 77)
    assert out.dtype == np.int32 and out[4, 4] == 77
    assert int((out == 77).sum()) == 49 - 9 + 1          # d = 1: the border ring and the 8 round the hole stay
    assert (out[3:6, 3:6] == [[2, 2, 2], [2, 77, 2], [2, 2, 2]]).all()
    l = np.full((11, 11), 2, dtype=np.int64)
    l[5, 5] = 19                                                            # == C: invalid
    out = R.reference(l, 19, 1, 255)
    inner = out[1:-1, 1:-1]
    assert int((inner == 2).sum()) == 8 and out[5, 5] == 255 and int((out == 255).sum()) == 81 - 9 + 1


@pytest.mark.parametrize("size,d", [((1024, 2048), 46), ((1025, 2049), 46), ((769, 769), 22), ((512, 512), 14),
                                    ((480, 480), 14), ((65, 65), 2), ((10, 10), 1)])
def test_boundary_dilation(size, d):
    from dcfp_amd.utils.edge_utils import boundary_dilation
    assert boundary_dilation(*size) == d
    assert boundary_dilation(size[0], size[1], 0.02) == d


def test_boundary_dilation_is_at_least_one():
    from dcfp_amd.utils.edge_utils import boundary_dilation
    assert boundary_dilation(3, 3) == 1 and boundary_dilation(1, 1, 0.0) == 1


@pytest.mark.parametrize("name", ["dcfp_label_boundary_i32", "dcfp_label_boundary_i64"])
def test_launcher_validation_needs_no_gpu(name):
    from dcfp_amd import _lib
    L = _lib.lib()
    fn = getattr(L, name)
    need = L.dcfp_label_boundary_workspace_bytes(2, 5, 9)
    assert need >= 2 * 5 * 9
    buf = (ctypes.c_int64 * 4096)()                       # host memory: never dereferenced, validation comes first
    a = ctypes.addressof(buf)
    lab, out, ws = a, a + 8192, a + 16384
    ok = dict(labels=lab, out=out, N=2, H=5, W=9, C=19, d=2, bg=255, ws=ws, wsb=need)

    def call(**kw):
        v = dict(ok, **kw)
        return fn(v["labels"], v["out"], v["N"], v["H"], v["W"], v["C"], v["d"], v["bg"], v["ws"], v["wsb"], None)
    bad = _lib.E_BADDESC
    assert call(labels=None) == bad and call(out=None) == bad and call(ws=None) == bad
    assert call(N=0) == bad and call(H=0) == bad and call(W=-1) == bad
    assert call(d=0) == bad and call(d=-3) == bad
    assert call(C=0) == bad
    assert call(out=lab) == bad
    assert call(wsb=need - 1) == bad and call(wsb=0) == bad
    assert call(C=256) == _lib.E_UNSUPPORTED and call(C=1000) == _lib.E_UNSUPPORTED
    assert call(C=256, d=0) == bad                        # a bad descriptor is reported before an unsupported one


def test_workspace_bytes_are_computed_in_64_bits():
    from dcfp_amd import _lib
    L = _lib.lib()
    assert L.dcfp_label_boundary_workspace_bytes(0, 5, 5) == 0
    assert L.dcfp_label_boundary_workspace_bytes(4, 1024, 2048) == 2 * 4 * 1024 * 2048
    big = L.dcfp_label_boundary_workspace_bytes(64, 65536, 65536)
    assert big >= 64 * 65536 * 65536 > 2 ** 32


def test_label_boundary_has_no_cpu_path():
    from dcfp_amd import evaluate, ops
    from dcfp_amd.utils import edge_utils
    with pytest.raises(RuntimeError):
        ops.label_boundary(torch.zeros(5, 9, dtype=torch.int32), 19, 2)
    with pytest.raises(RuntimeError):
        edge_utils.mask_to_boundary(torch.zeros(2, 5, 9, dtype=torch.int64), 19)
    with pytest.raises(RuntimeError):
        evaluate.boundary_confusion_matrix(torch.zeros(1, 5, 9, dtype=torch.int64),
                                           torch.zeros(1, 5, 9, dtype=torch.int32), 19)


@pytest.mark.parametrize("case", R.CASES + R.LONG_ROWS, ids=R.case_id)
def test_gpu_cases_have_interior_and_boundary(case):
    lab, ref = R.case_data(case)
    C, d = case[4], case[5]
    valid = (lab >= 0) & (lab < C)
    interior = R.interior_mask(lab, C, d)
    assert np.array_equal(interior, valid & (ref == 255))
    share = interior.sum() / valid.sum()
    print(R.case_id(case), "interior", int(interior.sum()), "share %.3f" % share)
    assert share >= 0.01 and interior.sum() >= 256
    assert 1.0 - share >= 0.01
    assert (~valid).any() and (lab == -1).any() and (lab == 255).any()


@pytest.mark.parametrize("case,share", list(zip(R.CASES, (0.368, 0.096, 0.543, 0.298, 0.084, 0.184, 0.200, 0.208,
                                                          0.015))), ids=lambda v: R.case_id(v) if isinstance(v, tuple) else None)
def test_gpu_cases_interior_share_is_the_recorded_one(case, share):
    lab, _ = R.case_data(case)
    valid = (lab >= 0) & (lab < case[4])
    assert abs(R.interior_mask(lab, case[4], case[5]).sum() / valid.sum() - share) < 5e-4


@pytest.mark.parametrize("case", R.DEGENERATE, ids=R.case_id)
def test_degenerate_cases_have_no_interior(case):
    lab, ref = R.case_data(case)
    C = case[4]
    valid = (lab >= 0) & (lab < C)
    assert not R.interior_mask(lab, C, case[5]).any()
    assert np.array_equal(ref, np.where(valid, lab, 255))


def test_long_rows_carry_runs_across_chunks():
    """The added long-row cases have interior pixels whose horizontal run crosses a multiple of 1024."""
    for case in R.LONG_ROWS:
        lab, _ = R.case_data(case)
        interior = R.interior_mask(lab, case[4], case[5])
        for edge in (1024, 2048):
            assert (interior[:, :, edge - 1] & interior[:, :, edge]).any(), (case, edge)
