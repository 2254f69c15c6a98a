"""What the tests of the two fused votes (whole-image: _vote_ref / test_vote_gpu, sliding-window: _slide_ref /
test_slide_gpu) share: the tolerance rule, seeded labels and the comparison of a kernel's result with float64."""
import torch


def tolerance_of(truth64, ref32, tensors):
    """-> (truth fp64, tol, e_ref, M): tol = 4 * e_ref + 2^-23 * M with e_ref = max |fp32 chain - fp64 chain| and
    M = max |logits| over `tensors` (None entries are skipped).  4: the kernel sums in another order than the two-pass
    chain; the second term is one fp32 unit of the largest input, so that a luckily rounded reference does not demand
    more than fp32 holds."""
    e_ref = float((ref32.double() - truth64).abs().max())
    M = max(float(t.abs().max()) for t in tensors if t is not None)
    return truth64, 4.0 * e_ref + 2.0 ** -23 * M, e_ref, M


def labels_for(seed, N, C, out_hw, ignore=255):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, C, (N,) + tuple(out_hw), generator=g)
    gt[torch.rand(gt.shape, generator=g) < 0.1] = ignore
    return gt


def held_to_truth(what, scores, pred, truth, tol, e_ref, M):
    """Scores lie within tol of float64; pred equals the float64 argmax wherever the float64 top-two gap exceeds 2 * tol
    (within tol the order cannot change there); the pixels left out are at most 0.5 %."""
    err = float((scores.double().cpu() - truth).abs().max())
    if truth.shape[1] > 1:
        top = truth.topk(2, dim=1).values
        decided = (top[:, 0] - top[:, 1]) > 2 * tol
    else:
        decided = torch.ones_like(truth[:, 0], dtype=torch.bool)
    left_out = 1.0 - float(decided.float().mean())
    wrong = int((pred.cpu().long() != truth.argmax(1))[decided].sum())
    print(f"{what}: e_ref {e_ref:.3e} M {M:.2f} tol {tol:.3e} kernel err {err:.3e} left out {left_out:.5f} wrong {wrong}")
    assert not bool(torch.isnan(truth).any())
    assert err <= tol
    assert wrong == 0
    assert left_out <= 0.005
