"""GPU: ops.label_components / ops.component_pixel (csrc/components.hip) against the numpy restatement of the
contract in tests/_resample_ref.py - equality of the label map, the counts, the label list, the sizes and the selected
pixels.  T is the tile edge of the kernel's tile pass (kTile); every grid size below is derived from it so that single
tiles, partial tiles, several tiles and the 2048-pixel blocks of the linear passes are all crossed."""
import ctypes
import random

import numpy as np
import pytest
import torch

import _resample_ref as R

pytestmark = pytest.mark.gpu

T = 64                       # kTile of csrc/components.hip
_cache = {"masks": R.pattern_masks(T)}


def masks():
    return _cache["masks"]


def reference(name):
    """The restatement's labelling of a pattern mask, computed once."""
    key = ("ref", name)
    if key not in _cache:
        _cache[key] = R.label_components(masks()[name])
    return _cache[key]


def mask_sample(mask, cls=1):
    """A mask as a sample: raw ids 0 / cls, identity maps, no padding."""
    H, W = mask.shape
    return dict(raw=np.where(mask, cls, 0).astype(np.uint8), row_map=np.arange(H, dtype=np.int32),
                col_map=np.arange(W, dtype=np.int32), grid=(H, W), cls=cls)


def run(samples, id_table=None):
    """-> (Components, device label tensors) of one launch over `samples`."""
    from dcfp_amd import ops
    dev = torch.device("cuda")
    maps, recs, labels, off = [], [], [], 0
    for s in samples:
        rm, cm = np.asarray(s["row_map"], np.int32), np.asarray(s["col_map"], np.int32)
        recs.append((len(rm), len(cm), s["grid"][0], s["grid"][1], off, off + len(rm), s["cls"]))
        off += len(rm) + len(cm)
        maps += [rm, cm]
        labels.append(torch.from_numpy(np.ascontiguousarray(s["raw"])).to(dev))
    d_maps = torch.from_numpy(np.concatenate(maps)).to(dev)
    d_id = None if id_table is None else torch.from_numpy(id_table).to(dev)
    return ops.label_components(labels, recs, d_maps, d_id, 255), labels


def check(comp, s, expect):
    lab, roots, sizes = expect
    assert comp.counts()[s] == len(roots)
    assert np.array_equal(comp.label_map(s).cpu().numpy(), lab)
    assert np.array_equal(comp.labels(s).cpu().numpy(), roots)
    assert np.array_equal(comp.component_sizes(s).cpu().numpy(), sizes)


@pytest.mark.parametrize("name", sorted(masks()))
def test_pattern(name):
    m = masks()[name]
    comp, _ = run([mask_sample(m)])
    check(comp, 0, reference(name))
    n_ref = len(reference(name)[1])
    if name in ("corner_diag", "corner_anti", "serpentine", "spiral"):
        assert n_ref == 1                       # a missing diagonal or a broken merge chain splits these
    if name.startswith("checker_"):
        # joined only through diagonals: one component on any grid with two rows and two columns; on a single row
        # or column the set pixels have no diagonal neighbour and every one is a component of its own
        assert n_ref == (1 if min(m.shape) >= 2 else (m.size + 1) // 2)
    if name == "corner_apart":
        assert n_ref == 2
    if name == "isolated":
        assert n_ref == ((m.shape[0] + 1) // 2) * ((m.shape[1] + 1) // 2)       # the capacity of the lists, reached


def blocky_source(seed=3):
    """40x70 raw ids in blocks, among them 3 (which the table sends to ignore) and none of class 5."""
    rng = np.random.RandomState(seed)
    coarse = rng.choice(np.array([7, 8, 11, 26, 3], dtype=np.uint8), size=(10, 14))
    return np.ascontiguousarray(np.kron(coarse, np.ones((4, 5), dtype=np.uint8)))


def id_table():
    t = np.arange(256, dtype=np.uint8)
    for raw, train in ((7, 0), (8, 1), (11, 2), (26, 13), (3, 255)):
        t[raw] = train
    return t


def scaled_sample(raw, f, crop, cls):
    from dcfp_amd.datasets import base
    H, W = raw.shape
    dst_h, dst_w = max(1, int(round(H * f))), max(1, int(round(W * f)))
    rm, cm = base.resize_taps(H, dst_h, f)[:, 3], base.resize_taps(W, dst_w, f)[:, 3]
    assert np.array_equal(rm, R.nearest_map(H, dst_h, f)) and np.array_equal(cm, R.nearest_map(W, dst_w, f))
    return dict(raw=raw, row_map=rm, col_map=cm, grid=(max(dst_h, crop[0]), max(dst_w, crop[1])), cls=cls)


def expected(s, table):
    return R.label_components(R.class_mask(s["raw"], table, s["row_map"], s["col_map"], s["grid"], s["cls"]))


@pytest.mark.parametrize("f", [0.5, 1.0, 1.3, 2.0])
def test_nearest_maps_and_padding(f):
    """The mask is read through the augmentation's nearest maps; at f = 0.5 and 1.0 the source is smaller than the
    48x96 crop, so part of the grid is padding: background that joins nothing."""
    raw, table = blocky_source(), id_table()
    samples = [scaled_sample(raw, f, (48, 96), cls) for cls in (0, 1, 13)]
    comp, _ = run(samples, table)
    for i, s in enumerate(samples):
        exp = expected(s, table)
        check(comp, i, exp)
        dst_h, dst_w = len(s["row_map"]), len(s["col_map"])
        got = comp.label_map(i).cpu().numpy()
        assert (got[dst_h:] == -1).all() and (got[:, dst_w:] == -1).all()
        assert len(exp[1]) >= 1


def test_absent_class_and_ignored_id():
    raw, table = blocky_source(), id_table()
    assert (raw == 3).any() and not (table[raw] == 5).any()
    samples = [scaled_sample(raw, 1.3, (48, 64), 5),        # a class the sample does not hold
               scaled_sample(raw, 1.3, (48, 64), 3),        # raw id 3 is there, but the table sends it to 255
               scaled_sample(raw, 1.3, (48, 64), 255)]      # ... where it is found
    comp, _ = run(samples, table)
    assert comp.counts()[:2] == [0, 0] and comp.counts()[2] >= 1
    for i, s in enumerate(samples):
        check(comp, i, expected(s, table))
    assert (comp.label_map(0) == -1).all()


def eighteen():
    rng = np.random.RandomState(11)
    samples = []
    for i in range(18):
        H, W = int(rng.randint(1, 3 * T)), int(rng.randint(1, 3 * T))
        raw = rng.randint(0, 4, size=(H, W)).astype(np.uint8)
        crop = (int(rng.randint(1, 2 * T)), int(rng.randint(1, 2 * T)))
        samples.append(scaled_sample(raw, (0.7, 1.0, 1.6)[i % 3], crop, i % 4))
    return samples


def test_eighteen_samples_in_one_call():
    """Records travel by value, 16 to a launch: 18 samples of different sizes, scales and classes, and a
    component_pixel call over all of them with n == 0 for every third."""
    from dcfp_amd import ops
    samples = eighteen()
    comp, _ = run(samples)
    exp = [expected(s, None) for s in samples]
    for i in range(18):
        check(comp, i, exp[i])
    rng = random.Random(5)
    n = [0 if i % 3 == 0 or len(exp[i][1]) == 0 else rng.randint(1, len(exp[i][1])) for i in range(18)]
    sizes = comp.sizes(n)
    assert sizes == [0 if v == 0 else int(exp[i][2][v - 1]) for i, v in enumerate(n)]
    k = [0 if v == 0 else rng.randint(0, sizes[i] - 1) for i, v in enumerate(n)]
    yx = ops.component_pixel(comp, n, k).cpu().numpy()
    assert sum(v > 0 for v in n) >= 8
    for i, v in enumerate(n):
        want = (-1, -1) if v == 0 else R.kth_pixel(exp[i][0], exp[i][1][v - 1], k[i])
        assert tuple(yx[i]) == want, i


@pytest.mark.parametrize("name", ["serpentine", "random40_odd"])
def test_component_pixel(name):
    """k = 0, size - 1 and five seeded ranks for every component: seven copies of the mask in one labelled batch, one
    call per component with the seven ranks."""
    from dcfp_amd import ops
    comp, _ = run([mask_sample(masks()[name])] * 7)
    lab, roots, sizes = reference(name)
    check(comp, 6, (lab, roots, sizes))
    rng = random.Random(7)
    flat = lab.reshape(-1)
    for n in range(1, len(roots) + 1):
        size = int(sizes[n - 1])
        assert comp.sizes([n] * 7) == [size] * 7
        where = np.flatnonzero(flat == roots[n - 1])
        ks = [0, size - 1] + [rng.randint(0, size - 1) for _ in range(5)]
        yx = ops.component_pixel(comp, [n] * 7, ks).cpu().numpy()
        assert (yx[:, 0] * lab.shape[1] + yx[:, 1]).tolist() == where[ks].tolist(), n
    yx = ops.component_pixel(comp, [0, 1] * 3 + [0], [0] * 7).cpu().numpy()
    assert yx[0::2].tolist() == [[-1, -1]] * 4 and (yx[1::2] >= 0).all()


def test_two_calls_give_identical_buffers():
    samples = [mask_sample(masks()["random40_big"]), mask_sample(masks()["serpentine"]), mask_sample(masks()["random60"])]
    a, _ = run(samples)
    b, _ = run(samples)
    assert a.counts() == b.counts()
    for i in range(len(samples)):
        assert torch.equal(a.label_map(i), b.label_map(i))
        assert torch.equal(a.labels(i), b.labels(i))
        assert torch.equal(a.component_sizes(i), b.component_sizes(i))


def test_bad_records_are_rejected_on_the_host():
    from dcfp_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda")
    H, W = 20, 30
    need = L.dcfp_components_workspace_bytes(H, W)
    assert need >= 2 * 4 * H * W
    raw = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    maps = torch.arange(H + W, dtype=torch.int32, device=dev)
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.empty(1, dtype=torch.int32, device=dev)

    def call(label=raw.data_ptr(), row_off=0, col_off=H, cls=1, work_off=0, work_bytes=need):
        rec = (_lib.CcSample * 1)(_lib.CcSample(label, H, W, H, W, H, W, row_off, col_off, cls, 0, work_off))
        return L.dcfp_label_components_u8(rec, 1, ctypes.c_void_p(maps.data_ptr()), maps.numel(), None,
                                          ctypes.c_void_p(work.data_ptr()), work_bytes, ctypes.c_void_p(counts.data_ptr()),
                                          None)
    assert call(label=None) == _lib.E_BADDESC
    assert call(col_off=H + 1) == _lib.E_BADDESC           # the column map would end one entry past the table
    assert call(row_off=-1) == _lib.E_BADDESC
    assert call(cls=256) == _lib.E_BADDESC and call(cls=-1) == _lib.E_BADDESC
    assert call(work_bytes=need - 4) == _lib.E_BADDESC     # the slice is one entry short
    assert call(work_off=16) == _lib.E_BADDESC             # ... or starts too late
    assert call() == 0
    torch.cuda.synchronize()
    assert counts.item() == 0
