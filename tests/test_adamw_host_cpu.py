"""CPU: FusedAdamW's host side - construction through build_optimizer, the flags it refuses, bit-identity with
torch.optim.AdamW on CPU parameters (where it applies torch's own functional update to its state), state_dict exchange
with torch.optim.AdamW in both directions, the ABI of DcfpAdamEntry / dcfp_adamw_f32, and the roundoff bound of the GPU
kernel test checked on a numpy fp32 restatement of the kernel's lines."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _adamw_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_optimizer_returns_fused_adamw():
    from dcfp_amd.optimizer import FusedAdamW, build_optimizer

    class A:
        no_decay = "bn,bias"; optim = "adamw"; betas = "0.8,0.95"; learning_rate = 3e-4; weight_decay = 0.05; momentum = 0.9
    m = torch.nn.Module()
    m.conv, m.bn = torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4)
    opt = build_optimizer(A, m)
    assert type(opt) is FusedAdamW and isinstance(opt, torch.optim.Optimizer)
    decay, no_decay = opt.param_groups
    assert [tuple(p.shape) for p in decay["params"]] == [(4, 3, 3, 3)] and len(no_decay["params"]) == 3
    assert decay["weight_decay"] == 0.05 and no_decay["weight_decay"] == 0.0
    for g in opt.param_groups:
        assert g["betas"] == (0.8, 0.95) and g["lr"] == 3e-4 and g["eps"] == 1e-8
        assert g["amsgrad"] is False and g["maximize"] is False
    assert opt.arena() is None and opt.table_rebuilds == 0           # CPU parameters: no arena, no tables


@pytest.mark.parametrize("flag", ["amsgrad", "maximize", "capturable"])
def test_unsupported_flags_raise(flag):
    from dcfp_amd.optimizer import FusedAdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError):
        FusedAdamW(p, **{flag: True})
    sd = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))], **{flag: True}).state_dict()
    with pytest.raises(NotImplementedError):
        FusedAdamW(p).load_state_dict(sd)


SCRIPT = [{"no_grad": (2,)}, {"no_grad": (2,)}, {}, {"before": [("wd", 0, 1e-3), ("wd", 1, 2e-4)], "no_grad": (6,)},
          {"before": ["resume"], "to_none": False}, {}]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_cpu_parameters_are_bit_identical_to_torch_adamw(dtype):
    """Poly learning rate, a late gradient (parameter 2), a missing one (parameter 6), a weight-decay change and
    save / resume: every parameter after every step, and the final state, equal torch.optim.AdamW's bit for bit."""
    from dcfp_amd.optimizer import FusedAdamW
    cpu = torch.device("cpu")
    mine = ac.drive(ac.Run(FusedAdamW, cpu, dtype), SCRIPT)
    ref = ac.drive(ac.Run(torch.optim.AdamW, cpu, dtype), SCRIPT)
    for it in range(len(SCRIPT)):
        for i in range(len(ac.SHAPES)):
            assert torch.equal(mine.history[it][i], ref.history[it][i]), (it, i)
    assert mine.steps_taken() == ref.steps_taken() == [6.0, 6.0, 4.0, 6.0, 6.0, 6.0, 5.0, 6.0]
    a, b = mine.opt.state_dict()["state"], ref.opt.state_dict()["state"]
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].keys() == b[k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        assert all(torch.equal(a[k][n], b[k][n]) and a[k][n].dtype == b[k][n].dtype for n in a[k])
    assert mine.opt.table_rebuilds == 0


def test_state_dict_round_trips_through_torch_adamw():
    from dcfp_amd.optimizer import FusedAdamW
    cpu = torch.device("cpu")
    src = ac.drive(ac.Run(torch.optim.AdamW, cpu, torch.float32), SCRIPT[:3])
    sd0 = src.opt.state_dict()
    fused = ac.Run(FusedAdamW, cpu, torch.float32)
    fused.opt.load_state_dict(sd0)
    sd1 = fused.opt.state_dict()
    back = ac.Run(torch.optim.AdamW, cpu, torch.float32)
    back.opt.load_state_dict(sd1)
    sd2 = back.opt.state_dict()
    for sd in (sd1, sd2):
        assert sd["state"].keys() == sd0["state"].keys()
        for k, st in sd0["state"].items():
            assert sd["state"][k].keys() == st.keys()
            for n, t in st.items():
                assert torch.equal(sd["state"][k][n], t) and sd["state"][k][n].dtype == t.dtype, (k, n)
            assert sd["state"][k]["step"].device.type == "cpu" and sd["state"][k]["step"].dtype == torch.float32
        assert sd["param_groups"] == sd0["param_groups"]
    # a state FusedAdamW wrote itself has torch.optim.AdamW's keys, and torch reads it
    own = ac.drive(ac.Run(FusedAdamW, cpu, torch.float32), SCRIPT[:3]).opt.state_dict()
    assert set(own["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "params"}
    back.opt.load_state_dict(own)
    assert back.opt.param_groups[0]["decoupled_weight_decay"] is True
    assert all(torch.equal(back.opt.state_dict()["state"][k][n], own["state"][k][n]) for k in own["state"]
               for n in own["state"][k])


def test_adam_entry_matches_the_header():
    from dcfp_amd import _lib
    src = open(os.path.join(ROOT, "include", "dcfp_hip.h")).read()
    body = re.search(r"typedef struct DcfpAdamEntry \{(.*?)\} DcfpAdamEntry;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(d.split()[-1].lstrip("*"), "*" in d, d) for d in (s.strip() for s in body.split(";")) if d]
    assert [f[0] for f in fields] == ["param", "grad", "exp_avg", "exp_avg_sq", "n", "first_chunk"]
    assert [f[0] for f in fields] == [n for n, _ in _lib.AdamEntry._fields_]
    off = 0
    for name, is_ptr, decl in fields:                                # every member is 8 bytes wide: no padding anywhere
        assert is_ptr or decl.startswith("int64_t"), decl
        assert getattr(_lib.AdamEntry, name).offset == off and getattr(_lib.AdamEntry, name).size == 8
        off += 8
    assert ctypes.sizeof(_lib.AdamEntry) == 48 == off
    args = re.search(r"int dcfp_adamw_f32\((.*?)\);", src, flags=re.S).group(1).split(",")
    kinds = [_lib._P if "*" in a or "dcfp_stream_t" in a else {"int": _lib._I, "int64_t": _lib._L, "float": _lib._F}[a.split()[0]]
             for a in args]
    assert _lib.SIGNATURES["dcfp_adamw_f32"] == (_lib._I, kinds)
    assert int(re.search(r"#define DCFP_SGD_CHUNK (\d+)", src).group(1)) == _lib.SGD_CHUNK == ac.CHUNK


def test_argument_errors_do_not_need_a_gpu():
    from dcfp_amd import _lib
    L = _lib.lib()
    entry = _lib.AdamEntry()
    tab = ctypes.cast(ctypes.pointer(entry), ctypes.c_void_p)
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.03, None)
    assert L.dcfp_adamw_f32(None, 1, 1, *tail) == _lib.E_BADDESC
    assert L.dcfp_adamw_f32(tab, -1, 1, *tail) == _lib.E_BADDESC
    assert L.dcfp_adamw_f32(tab, 1, -1, *tail) == _lib.E_BADDESC
    assert L.dcfp_adamw_f32(tab, 1, 2 ** 31, *tail) == _lib.E_BADDESC
    assert L.dcfp_adamw_f32(tab, 0, 5, *tail) == 0                   # nothing to do: no launch
    assert L.dcfp_adamw_f32(tab, 1, 0, *tail) == 0


@pytest.mark.parametrize("case", list(ac.KERNEL_CASES))
def test_numpy_fp32_restatement_stays_within_the_kernel_bound(case):
    """The bound the GPU test holds the kernel to (derivation: _adamw_cases) is not tighter than fp32 arithmetic allows:
    the same lines in numpy fp32 - which rounds every product on its own, where the kernel uses an fma - stay inside it
    on the test's inputs."""
    step, lr, wd, beta1, state = ac.KERNEL_CASES[case]
    host, live = ac.kernel_inputs(state)
    sc = ac.scalars(step, lr, wd, beta1)
    x32 = {k: host[k][live] for k in "pgmv"}
    ref = ac.reference(*(x32[k].astype(np.float64) for k in "pgmv"), sc)
    out = ac.restate32(*(x32[k] for k in "pgmv"), sc)
    worst = ac.worst_ratios(out, ref)
    print("[numpy fp32 %s] worst |err|/bound: m %.3f v %.3f p %.3f" % (case, worst["m"], worst["v"], worst["p"]))
    assert max(worst.values()) <= 1.0, worst
    assert (x32["g"] == 0).any() and (x32["g"][x32["g"] != 0] ** 2 > 0).all()      # exact zeros, and g*g never underflows
    if lr == 0.0 and wd == 0.0:
        assert np.array_equal(out["p"].view(np.int32), x32["p"].view(np.int32))
    if beta1 == 0.0:
        assert np.array_equal(out["m"].view(np.int32), x32["g"].view(np.int32))
