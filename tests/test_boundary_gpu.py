"""GPU: ops.label_boundary, utils.edge_utils.mask_to_boundary, evaluate.boundary_confusion_matrix / boundary_iou against
the brute-force numpy restatement of tests/_boundary_ref.py.  Labels are integers: every comparison is exact equality.
tests/test_boundary_host_cpu.py asserts on the reference alone that the cases hold interior and boundary pixels."""
import numpy as np
import pytest
import torch

import _boundary_ref as R

pytestmark = pytest.mark.gpu
DTYPES = (torch.int32, torch.int64)


def _t(a):
    return torch.from_numpy(np.array(a))                  # (a copy: the shared case data is read-only)


def _run(lab_np, C, d, dtype, dev, background=255):
    from dcfp_amd import ops
    x = _t(lab_np).to(dtype).to(dev)
    keep = x.clone()
    out = ops.label_boundary(x, C, d, background)
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    assert torch.equal(x, keep), "the input was written to"
    return out.cpu().numpy().astype(np.int64)


def _diff(got, ref):
    bad = np.argwhere(got != ref)
    return "%d differ, first at %s: got %s, reference %s" % (
        len(bad), bad[:4].tolist(), [int(got[tuple(b)]) for b in bad[:4]], [int(ref[tuple(b)]) for b in bad[:4]])


@pytest.mark.parametrize("dtype", DTYPES, ids=("i32", "i64"))
@pytest.mark.parametrize("case", R.CASES + R.DEGENERATE + R.LONG_ROWS, ids=R.case_id)
def test_label_boundary_equals_reference(cuda, case, dtype):
    lab, ref = R.case_data(case)
    got = _run(lab, case[4], case[5], dtype, cuda)
    assert np.array_equal(got, ref), _diff(got, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=("i32", "i64"))
def test_probe_769(cuda, dtype):
    got = _run(R.probe(), 19, 4, dtype, cuda)
    assert got.shape == (41, 53)                          # [H, W] in, [H, W] out
    assert int((got != 255).sum()) == 769 and int((got == 5).sum()) == 1
    assert np.array_equal(got, R.reference(R.probe(), 19, 4, 255))


@pytest.mark.parametrize("dtype", DTYPES, ids=("i32", "i64"))
def test_non_contiguous_view(cuda, dtype):
    from dcfp_amd import ops
    case = R.CASES[2]
    lab, ref = R.case_data(case)
    wide = torch.full((2, 64, 100), 7, dtype=dtype, device=cuda)
    wide[:, :, 18:82] = _t(lab).to(dtype).to(cuda)
    view = wide[:, :, 18:82]
    assert not view.is_contiguous()
    out = ops.label_boundary(view, case[4], case[5])
    assert out.is_contiguous() and out.shape == view.shape
    assert np.array_equal(out.cpu().numpy().astype(np.int64), ref)
    assert bool((wide[:, :, :18] == 7).all()) and bool((wide[:, :, 82:] == 7).all())


def test_offset_view_that_is_not_16_byte_aligned(cuda):
    """A contiguous tensor that starts 4 bytes into its storage takes the element-access kernels."""
    from dcfp_amd import ops
    case = R.CASES[2]
    lab, ref = R.case_data(case)
    flat = torch.zeros(2 * 64 * 64 + 1, dtype=torch.int32, device=cuda)
    view = flat[1:].view(2, 64, 64)
    view.copy_(_t(lab).to(torch.int32))
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    out = ops.label_boundary(view, case[4], case[5])
    assert np.array_equal(out.cpu().numpy().astype(np.int64), ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=("i32", "i64"))
def test_repeated_runs_give_the_same_bits(cuda, dtype):
    from dcfp_amd import ops
    case = R.CASES[6]
    lab, _ = R.case_data(case)
    x = _t(lab).to(dtype).to(cuda)
    a = ops.label_boundary(x, case[4], case[5])
    b = ops.label_boundary(x, case[4], case[5])
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=("i32", "i64"))
def test_background_19(cuda, dtype):
    case = R.CASES[0]
    lab, _ = R.case_data(case)
    ref = R.reference(lab, 19, 2, 19)
    got = _run(lab, 19, 2, dtype, cuda, background=19)
    assert np.array_equal(got, ref), _diff(got, ref)
    assert got.max() == 19 and got.min() >= 0


def test_mask_to_boundary_uses_d_2_at_65x65(cuda):
    from dcfp_amd.utils.edge_utils import mask_to_boundary
    lab = R.make_map("dense", 2, 65, 65, 19, 21, 22)
    ref = R.reference(lab, 19, 2, 255)
    assert not np.array_equal(ref, R.reference(lab, 19, 1, 255)) and not np.array_equal(ref, R.reference(lab, 19, 3, 255))
    got = mask_to_boundary(_t(lab).to(cuda), 19)
    assert got.shape == (2, 65, 65) and np.array_equal(got.cpu().numpy(), ref)
    one = mask_to_boundary(_t(lab[1]).to(torch.int32).to(cuda), 19, dilation_ratio=0.02, background=19)
    assert one.shape == (65, 65) and one.dtype == torch.int32
    assert np.array_equal(one.cpu().numpy().astype(np.int64), R.reference(lab[1], 19, 2, 19))


def test_boundary_confusion_matrix_and_iou(cuda):
    from dcfp_amd import evaluate
    from dcfp_amd.utils.edge_utils import boundary_dilation
    C, ratio = 19, 0.03
    assert boundary_dilation(33, 65, ratio) == 2
    gt, gt_b = R.case_data(R.CASES[0])
    pred = np.roll(gt, (2, 3), axis=(1, 2))
    pred_b = R.reference(pred, C, 2, C)
    counted = gt_b != 255
    want = np.zeros((C, C + 1), dtype=np.int64)
    np.add.at(want, (gt_b[counted], pred_b[counted]), 1)
    assert want[:, C].sum() > 0 and np.diag(want[:, :C]).sum() > 0

    conf = evaluate.boundary_confusion_matrix(_t(gt).to(cuda), _t(pred).to(torch.int32).to(cuda),
                                              C, dilation_ratio=ratio)
    assert conf.dtype == torch.int64 and tuple(conf.shape) == (C, C + 1)
    got = conf.cpu().numpy()
    assert np.array_equal(got, want)
    # the reference's own count, gt * C + pred over the pixels where the prediction is a class
    pred_ref = R.reference(pred, C, 2, 255)
    ok = counted & (pred_ref != 255)
    binc = np.bincount(gt_b[ok] * C + pred_ref[ok], minlength=C * C).reshape(C, C)
    assert np.array_equal(got[:, :C], binc)

    again = evaluate.boundary_confusion_matrix(_t(gt).to(cuda), _t(pred).to(torch.int32).to(cuda),
                                               C, dilation_ratio=ratio, out=conf)
    assert again is conf and np.array_equal(conf.cpu().numpy(), 2 * want)

    mean, per_class = evaluate.boundary_iou(_t(want).to(cuda))
    w = want.astype(np.float64)
    tp, pos, res = np.diag(w[:, :C]), w.sum(1), w[:, :C].sum(0)
    iou = tp / np.maximum(1.0, pos + res - tp)
    assert np.array_equal(per_class.cpu().numpy(), iou) and mean == pytest.approx(iou.mean(), abs=1e-15)
    assert 0.0 < mean < 1.0
