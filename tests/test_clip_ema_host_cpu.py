"""Gradient-norm clipping and weight EMA on the arena optimizers, the parts that need no GPU: the restated norm and
coefficient against torch.nn.utils.clip_grad_norm_, constructor refusals, the torch fallback of both optimizers on a CPU
model, ema_state_dict, the state-file fingerprint rules and the driver's arguments."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

import _clip_ema_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("max_norm", [0.5, 3.0, 1e4])
def test_restated_norm_and_coefficient_against_clip_grad_norm(max_norm):
    """On fp64 CPU tensors torch's norm is an fp64 norm: the restated sum of squares agrees to rel 1e-12, and the
    restated coefficient - from torch's norm rounded to fp32 - equals torch's coefficient rounded to fp32 up to the
    one ulp that rounding the norm first can cost."""
    arrays = ref.values("randn")
    params = [torch.nn.Parameter(torch.zeros(a.shape, dtype=torch.float64)) for a in arrays]
    for p, a in zip(params, arrays):
        p.grad = torch.from_numpy(a.astype(np.float64))
    before = [p.grad.clone() for p in params]
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    sq, per = ref.sqnorm64(arrays)
    assert abs(sq - float(total) ** 2) <= 1e-12 * sq
    for a, s in zip(arrays, per):
        assert abs(s - float(np.sum(a.astype(np.float64) ** 2))) <= 1e-12 * s
    norm = ref.norm32(sq)
    assert norm == np.float32(float(total))
    coef = ref.coef32(norm, max_norm)
    t_coef = min(1.0, max_norm / (float(total) + 1e-6))
    assert abs(float(coef) - float(np.float32(t_coef))) <= float(np.spacing(np.float32(t_coef)))
    big = max(range(len(arrays)), key=lambda i: arrays[i].size)           # ... and torch really scaled by it
    assert torch.allclose(params[big].grad, before[big] * t_coef, rtol=1e-15, atol=0)


def test_restated_edge_values():
    assert ref.coef32(ref.norm32(float("inf")), 1.0) == 0.0
    assert math.isnan(ref.coef32(ref.norm32(float("nan")), 1.0))
    assert ref.coef32(np.float32(0.0), 1.0) == 1.0
    sq, _ = ref.sqnorm64(ref.values("huge"))
    assert math.isfinite(sq) and math.isfinite(float(ref.norm32(sq)))        # 1e25-sized gradients: finite in fp64
    sq, _ = ref.sqnorm64(ref.values("tiny"))
    assert sq > 0                                                            # 1e-30: the squares underflow fp32, not fp64


# ------------------------------------------------------------------------------------------------ constructors
@pytest.mark.parametrize("cls", ["FusedSGD", "FusedAdamW"])
def test_constructor_refusals(cls):
    from dcfp_amd import optimizer as om
    make = getattr(om, cls)
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            make(p, lr=0.1, max_grad_norm=bad)
    for bad in (0.5, 1.0, 0.0, 1.5, -0.9, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            make(p, lr=0.1, ema_decay=bad)
    opt = make(p, lr=0.1, max_grad_norm=2.0, ema_decay=0.999)
    assert opt.max_grad_norm == 2.0 and opt.ema_decay == 0.999
    plain = make(p, lr=0.1)
    assert plain.max_grad_norm is None and plain.ema_decay is None and "ema" not in plain._ARENA_STATE
    with pytest.raises(RuntimeError, match="ema_decay"):
        plain.ema_state_dict(torch.nn.Linear(1, 1))


def test_build_optimizer_reads_the_config():
    from dcfp_amd import optimizer as om

    class A:
        no_decay = "bias"; optim = "adamw"; betas = "0.9,0.999"; learning_rate = 1e-3; weight_decay = 1e-2; momentum = 0.9
        clip_grad_norm = 0.25; ema_decay = 0.99
    opt = om.build_optimizer(A, torch.nn.Linear(3, 2))
    assert type(opt) is om.FusedAdamW and opt.max_grad_norm == 0.25 and opt.ema_decay == 0.99
    A.optim = "sgd"
    del A.clip_grad_norm, A.ema_decay
    opt = om.build_optimizer(A, torch.nn.Linear(3, 2))
    assert type(opt) is om.FusedSGD and opt.max_grad_norm is None and opt.ema_decay is None


# ------------------------------------------------------------------------------------------------ the CPU fallback
def _model():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))


def _groups(m):
    ps = list(m.parameters())
    return [{"params": ps[:3]}, {"params": ps[3:], "weight_decay": 0.0}]


def _backward(m, it):
    g = torch.Generator().manual_seed(50 + it)
    x = torch.randn(4, 7, generator=g)
    # (the last Linear takes no part: its parameters have no gradient)
    (m[2](m[1](m[0](x))) * 30.0).square().sum().backward()


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_cpu_fallback_equals_torch_clip_step_and_lerp(kind):
    from dcfp_amd import optimizer as om
    MAXN, DECAY = 0.5, 0.9
    a, b = _model(), None
    b = copy.deepcopy(a)
    if kind == "sgd":
        mine = om.FusedSGD(_groups(a), lr=0.05, momentum=0.9, weight_decay=1e-2, max_grad_norm=MAXN, ema_decay=DECAY)
        theirs = torch.optim.SGD(_groups(b), lr=0.05, momentum=0.9, weight_decay=1e-2)
    else:
        mine = om.FusedAdamW(_groups(a), lr=0.05, weight_decay=1e-2, max_grad_norm=MAXN, ema_decay=DECAY)
        theirs = torch.optim.AdamW(_groups(b), lr=0.05, weight_decay=1e-2)
    ema = [p.detach().clone() for p in b.parameters()]
    for it in range(3):
        mine.zero_grad()
        theirs.zero_grad()
        _backward(a, it)
        _backward(b, it)
        raw = [None if p.grad is None else p.grad.clone() for p in a.parameters()]
        mine.step()
        total = torch.nn.utils.clip_grad_norm_(b.parameters(), MAXN)
        assert float(total) > MAXN                       # the clip bites on every step
        theirs.step()
        for e, p in zip(ema, b.parameters()):
            if p.grad is not None:
                e.copy_(torch.lerp(e, p.detach(), 1.0 - DECAY))
        assert ref.torch_bits_equal(mine.grad_norm(), total)
        for p, q, g0 in zip(a.parameters(), b.parameters(), raw):
            assert torch.equal(p, q), (kind, it)
            if g0 is None:
                assert p.grad is None
            else:
                assert ref.torch_bits_equal(p.grad, g0), "the optimizer scaled p.grad"
        for p, e in zip(a.parameters(), ema):
            assert torch.equal(mine.state.get(p, {}).get("ema", p.detach()), e), (kind, it)
    pairs = mine.grad_sqnorms()
    assert len(pairs) == 4 and all(s.dtype == torch.float64 for _, s in pairs)      # (two parameters have no gradient)
    assert abs(math.sqrt(sum(float(s) for _, s in pairs)) - float(total)) <= 1e-5 * float(total)
    # the average travels in the optimizer's state_dict and ema_state_dict has the model's keys
    sd = mine.state_dict()
    assert all("ema" in st for st in sd["state"].values())
    esd = mine.ema_state_dict(a)
    assert list(esd) == list(a.state_dict())
    for (name, p), e in zip(a.named_parameters(), ema):
        assert torch.equal(esd[name], e) and esd[name].data_ptr() != p.data_ptr()
    # ema_weights swaps and restores bit for bit; no step inside
    before = [p.detach().clone() for p in a.parameters()]
    with mine.ema_weights():
        for p, e in zip(a.parameters(), ema):
            assert torch.equal(p, e)
        with pytest.raises(RuntimeError, match="ema_weights"):
            mine.step()
    for p, q, e in zip(a.parameters(), before, ema):
        assert ref.torch_bits_equal(p.detach(), q) and torch.equal(mine._ema_of(p), e)


def test_restated_lerp_against_torch():
    g = torch.Generator().manual_seed(9)
    e, p = torch.randn(4097, generator=g), torch.randn(4097, generator=g)
    mine = ref.lerp32(e.numpy(), p.numpy(), 0.999)
    theirs = torch.lerp(e, p, 1.0 - 0.999).numpy()
    assert np.abs(mine.view(np.int32) - theirs.view(np.int32)).max() <= 1     # fused or not: one ulp at the most


# ------------------------------------------------------------------------------------------------ state files
def _fp(**over):
    from dcfp_amd import train_state

    class Args:
        pass
    a = Args()
    for field, attr in train_state.ARG_FIELDS:
        setattr(a, attr, None)
    a.optim = "sgd"
    for k, v in over.items():
        setattr(a, k, v)
    return train_state.fingerprint(a, torch.nn.Linear(2, 2), 19, 1)


def test_fingerprint_fields_and_the_old_file_rule():
    from dcfp_amd import train_state
    fields = [f for f, _ in train_state.ARG_FIELDS]
    assert "clip_grad_norm" in fields and "ema_decay" in fields
    now = _fp()
    old = {k: v for k, v in now.items() if k not in ("clip_grad_norm", "ema_decay")}      # written before the fields existed
    train_state.check_fingerprint(old, now)                                               # continues with neither flag
    with pytest.raises(ValueError, match="ema_decay"):
        train_state.check_fingerprint(old, _fp(ema_decay=0.999))
    with pytest.raises(ValueError, match="clip_grad_norm"):
        train_state.check_fingerprint(old, _fp(clip_grad_norm=1.0))
    with pytest.raises(ValueError, match="ema_decay"):                                    # written with EMA, run without
        train_state.check_fingerprint(_fp(ema_decay=0.999), now)
    with pytest.raises(ValueError, match="clip_grad_norm"):
        train_state.check_fingerprint(_fp(clip_grad_norm=1.0), _fp(clip_grad_norm=2.0))
    train_state.check_fingerprint(_fp(clip_grad_norm=1.0, ema_decay=0.99), _fp(clip_grad_norm=1.0, ema_decay=0.99))
    lacking = {k: v for k, v in now.items() if k != "optim"}                              # the rule is for these two only
    with pytest.raises(ValueError, match="optim"):
        train_state.check_fingerprint(lacking, now)


# ------------------------------------------------------------------------------------------------ the driver's arguments
def test_train_arguments():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import importlib
    train = importlib.import_module("train")
    parser = train.get_parser()
    args = parser.parse_args([])
    assert args.clip_grad_norm is None and args.ema_decay is None
    train.check_args(args)
    args = parser.parse_args(["--clip-grad-norm", "0.5", "--ema-decay", "0.999"])
    assert args.clip_grad_norm == 0.5 and args.ema_decay == 0.999
    train.check_args(args)
    for bad in (["--clip-grad-norm", "0"], ["--clip-grad-norm", "nan"], ["--clip-grad-norm", "-1"]):
        with pytest.raises(ValueError, match="clip-grad-norm"):
            train.check_args(parser.parse_args(bad))
    for bad in (["--ema-decay", "0.5"], ["--ema-decay", "1"], ["--ema-decay", "nan"]):
        with pytest.raises(ValueError, match="ema-decay"):
            train.check_args(parser.parse_args(bad))
