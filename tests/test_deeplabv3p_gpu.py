"""GPU: DeepLabv3+ (networks.deeplabv3p) on the MI355X.

* ops.DecoderConcatFn against an fp64 ATen composite (1x1 conv + BatchNorm + ReLU, interpolate, cat) at a ragged
  layer1 width (175, a pruned one) and on a row-pitched concat, in train and eval mode;
* the whole model against the reference's record (tests/golden/model_v3p_r50_2x65x65.npz): loss, both heads' logits,
  per-tensor gradients (tests/_parity.py, unchanged rules);
* the slim model of the reference's global_percent 0.5 pruning (ragged widths 175 / 146 / 147) against its logits;
* the data-parallel path at world size 1 bit-identical to the plain step (SyncBN through the node);
* tools/train.py -> score.pth -> tools/prune.py with --model deeplabv3p;
* the decoder's first 3x3 conv on the Winograd kernels at BASELINE config 3 shapes."""
import copy
import sys

import pytest
import torch
import torch.nn.functional as F

import _model_cases as mc       # (run as a script - the data-parallel child - this file's directory is on sys.path)

pytestmark = pytest.mark.gpu
TAG = "v3p_r50_2x65x65"


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("Cl,hw,HW", [(175, (17, 33), (33, 65)), (256, (64, 128), (128, 256))])
def test_decoder_concat_vs_fp64_composite(cuda, train, Cl, hw, HW):
    from dcfp_amd import ops
    from dcfp_amd.networks import _exec
    from dcfp_amd.networks.deeplabv3p import Decoder
    N, Cx = 2, 512
    g = torch.Generator().manual_seed(5)
    dec = Decoder(19, True, low_level_inplanes=Cl)
    with torch.no_grad():
        dec.conv1.weight.copy_(torch.randn(dec.conv1.weight.shape, generator=g) * 0.05)
        dec.bn1.weight.copy_(1.0 + 0.2 * torch.randn(48, generator=g))
        dec.bn1.bias.copy_(0.1 * torch.randn(48, generator=g))
        dec.bn1.running_mean.copy_(0.1 * torch.randn(48, generator=g))
        dec.bn1.running_var.copy_(1.0 + 0.3 * torch.rand(48, generator=g))
    ref = copy.deepcopy(dec).double()
    dec2 = copy.deepcopy(dec).to(cuda).train(train)          # (for the no_grad call below)
    dec = dec.to(cuda).train(train)
    ref = ref.to(cuda).train(train)
    x64 = torch.randn(N, Cx, *hw, generator=g, dtype=torch.float64).to(cuda).requires_grad_(True)
    low64 = torch.relu(torch.randn(N, Cl, *HW, generator=g, dtype=torch.float64)).to(cuda).requires_grad_(True)
    dcat = torch.randn(N, Cx + 48, *HW, generator=g).to(cuda)
    x = x64.detach().float().requires_grad_(True)
    low = low64.detach().float().requires_grad_(True)

    pitch = dec.concat_pitch((N, Cx + 48) + tuple(HW))
    cfg = {"bn": _exec._bn_args(dec.bn1), "pitch": pitch, "owner": dec, "align": True}
    cat = ops.decoder_concat(x, low, cfg, dec.conv1.weight, dec.bn1.weight, dec.bn1.bias)
    assert ops._pitch_of(cat) == pitch                      # (0 at 33 x 65: the 3x3 conv reads that shape dense)
    if HW == (128, 256):
        assert pitch >= HW[1] + 4                           # the row-pitched concat of the training graph
    cat.backward(dcat)

    a = F.interpolate(x64, size=HW, mode="bilinear", align_corners=True)
    # the ReLU with the kernel's mask: a pre-activation within fp32 rounding of 0 may take either side (one such element
    # moves d low by ~1e-3 relative at 2 x 48 x 128 x 256), which is not what this test is about
    b = ref.bn1(ref.conv1(low64)) * (cat.detach()[:, Cx:] > 0).double()
    want = torch.cat((a, b), 1)
    want.backward(dcat.double())
    torch.cuda.synchronize()
    assert _rel(cat.detach(), want.detach()) <= 1e-5
    assert _rel(x.grad, x64.grad) <= 1e-5
    assert _rel(low.grad, low64.grad) <= 1e-4
    assert _rel(dec.conv1.weight.grad, ref.conv1.weight.grad) <= 1e-4
    assert _rel(dec.bn1.weight.grad, ref.bn1.weight.grad) <= 1e-4
    assert _rel(dec.bn1.bias.grad, ref.bn1.bias.grad) <= 1e-5
    assert _rel(dec.bn1.running_mean, ref.bn1.running_mean) <= 1e-5
    assert _rel(dec.bn1.running_var, ref.bn1.running_var) <= 1e-5
    assert int(dec.bn1.num_batches_tracked) == int(ref.bn1.num_batches_tracked)
    # no_grad: the same values (a dense concat for the inference conv)
    with torch.no_grad():
        cfg2 = {"bn": _exec._bn_args(dec2.bn1), "pitch": 0, "owner": dec2, "align": True}
        cat2 = ops.decoder_concat(x.detach(), low.detach(), cfg2, dec2.conv1.weight, dec2.bn1.weight, dec2.bn1.bias)
    assert _rel(cat2, want.detach()) <= 1e-5


def test_forward_backward_vs_reference_golden(cuda, capsys):
    mc.forward_backward_vs_golden(TAG, cuda, capsys)


def test_slim_model_matches_reference(cuda, tmp_path):
    def ragged_widths(slim):
        assert slim.decoder.conv1.weight.shape[1] == 175
        assert slim.decoder.last_conv[0].weight.shape[0] == 146 and slim.decoder.last_conv[3].weight.shape[0] == 147
    mc.slim_model_logits_check("deeplabv3p", "v3pr50", cuda, tmp_path, ragged_widths)


def test_decoder_first_conv_on_winograd_at_config3(cuda):
    """BASELINE config 3 (4x3x1024x2048): the concat is 4 x 560 x 256 x 512, row-pitched for decoder.last_conv.0, whose
    three passes run on the Winograd kernels (the weight gradient and the data gradient on the fused ones)."""
    from dcfp_amd import _lib, ops
    from dcfp_amd.networks.deeplabv3p import Decoder
    dec = Decoder(19, True)
    shape = (4, 560, 256, 512)
    pitch = dec.concat_pitch(shape)
    assert pitch >= 512 + 4
    d = ops._desc(shape, tuple(dec.last_conv[0].weight.shape), 1, 1, 1, pitch, pitch)
    names = [ops.conv_kernel_name(d, k) for k in (_lib.CONV_FWD, _lib.CONV_DGRAD, _lib.CONV_WGRAD)]
    assert all(n.startswith("winograd_f2x2_3x3") for n in names), names
    assert "fused" in names[2], names
    assert bool(_lib.lib().dcfp_conv2d_pitch_supported(ctypes_byref(d)))


def ctypes_byref(d):
    import ctypes
    return ctypes.byref(d)


def test_data_parallel_bit_identical_to_plain(cuda):
    mc.data_parallel_bit_identical(__file__)


def test_train_then_prune_tools(cuda, tmp_path):
    mc.train_then_prune(TAG, ("decoder.last_conv.0", "decoder.conv1"), tmp_path)


if __name__ == "__main__" and "--ddp-child" in sys.argv:
    mc.ddp_child("deeplabv3p", 29543, lambda m: m.decoder.bn1)
