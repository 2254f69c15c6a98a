"""GPU: ops.png_deflate_labels (csrc/png.hip) against the plain Python restatement of the stream format in
tests/_png_ref.py.  Everything is bytes: the device streams equal the restatement's byte for byte, decode through zlib
and through PIL to lut[pred & 255], and two calls give the same bytes.  N = 2 images, P = 2 tables (the identity and
a random permutation) in every case."""
import io
import zlib

import numpy as np
import pytest
import torch

import _png_ref as R

pytestmark = pytest.mark.gpu
RUNS = [1, 2, 3, 4, 257, 258, 259, 260, 261, 262, 516, 517, 518, 519, 520, 775]
VALUES = [0, 143, 144, 255, 1, 2]


def rect_maps(rng, N, H, W, classes=19):
    m = np.empty((N, H, W), dtype=np.int32)
    for n in range(N):
        m[n] = rng.randint(0, classes)
        for _ in range(6):
            y, x = rng.randint(0, H), rng.randint(0, W)
            m[n, y:y + rng.randint(1, H + 1), x:x + rng.randint(1, W + 1)] = rng.randint(0, classes)
    return m


def crafted(shift):
    """Rows of the runs RUNS, rotated by the row number (+ shift), values cycling through VALUES; then two rows equal
    to the row above (all-zero filtered rows), two rows of constant 2, and rows of constant 4 and 6 (filtered: all 2)."""
    rows = []
    for y in range(len(RUNS)):
        k = (y + shift) % len(RUNS)
        order = RUNS[k:] + RUNS[:k]
        rows.append(np.concatenate([np.full(L, VALUES[(i + y) % len(VALUES)], dtype=np.int32)
                                    for i, L in enumerate(order)]))
    rows += [rows[-1], rows[-1]]
    # two rows of constant 2 (the second one filters to zeros), then constants 4 and 6: their filtered rows are all 2,
    # one run together with the filter byte
    rows += [np.full_like(rows[0], v) for v in (2, 2, 4, 6)]
    return np.stack(rows)


def cases():
    rng = np.random.RandomState(7)
    out = {}
    for H, W in [(1, 1), (3, 2), (2, 257), (5, 259), (7, 263), (9, 520), (33, 777), (16, 2049), (3, 4099)]:
        out["rect_%dx%d" % (H, W)] = rect_maps(rng, 2, H, W)
    out["crafted"] = np.stack([crafted(0), crafted(5)])
    out["random_8x300"] = rng.randint(0, 256, (2, 8, 300)).astype(np.int32)
    out["constant_64x64"] = np.stack([np.full((64, 64), 7, dtype=np.int32), np.full((64, 64), 200, dtype=np.int32)])
    out["over_255_12x70"] = rng.randint(256, 301, (2, 12, 70)).astype(np.int32)
    # beyond the format's own cases: more rows than one pass of the stream kernel's scan takes (256), and the widest
    # row the encoder accepts (the most bytes per lane, the largest LDS buffers), half of it noise
    out["tall_600x5"] = rect_maps(rng, 2, 600, 5)
    wide = rect_maps(rng, 2, 2, 8192)
    wide[:, :, 4096:] = rng.randint(0, 256, (2, 2, 4096))
    out["wide_2x8192"] = wide
    return out


CASES = cases()


@pytest.fixture(scope="module")
def luts():
    return np.stack([np.arange(256, dtype=np.uint8), np.random.RandomState(3).permutation(256).astype(np.uint8)])


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_streams_equal_the_restatement(cuda, luts, name):
    from PIL import Image
    from dcfp_amd import evaluate, ops
    pred = CASES[name]
    N, H, W = pred.shape
    P = luts.shape[0]
    d_pred, d_luts = torch.from_numpy(pred).to(cuda), torch.from_numpy(luts).to(cuda)

    def run():
        streams, offsets, lengths = ops.png_deflate_labels(d_pred, d_luts)
        offsets, lengths = offsets.cpu().tolist(), lengths.cpu().tolist()
        data = streams[:sum(lengths)].cpu().numpy().tobytes()
        return data, offsets, lengths
    data, offsets, lengths = run()
    assert offsets == [int(v) for v in np.cumsum([0] + lengths[:-1])]              # compacted, in stream order
    palette = [int(v) for v in np.random.RandomState(5).randint(0, 256, 3 * 256)]
    for n in range(N):
        for p in range(P):
            s = n * P + p
            image = luts[p][pred[n] & 255]
            got = data[offsets[s]:offsets[s] + lengths[s]]
            assert lengths[s] <= ops.png_deflate_bound(H, W) == R.bound(H, W)
            assert zlib.decompress(got) == R.filtered_rows(image).tobytes(), (n, p)
            assert got == R.deflate_labels(image), (n, p)
            with Image.open(io.BytesIO(evaluate.png_container(got, H, W, palette if p == 0 else None))) as im:
                im.load()
                assert im.mode == ("P" if p == 0 else "L") and np.array_equal(np.asarray(im), image), (n, p)
    assert run() == (data, offsets, lengths)                                       # deterministic


def test_crafted_rows_are_what_the_case_promises():
    """(no GPU work: the crafted image's filtered rows hold the run lengths and the special rows it is there for)"""
    image = (crafted(0) & 255).astype(np.uint8)
    f = R.filtered_rows(image)
    assert sorted(L for _, L in R.runs(image[0].tolist())) == sorted(RUNS)
    T = len(RUNS)
    assert not f[T, 1:].any() and not f[T + 1, 1:].any() and not f[T + 3, 1:].any()
    assert (image[T + 2] == 2).all() and (image[T + 3] == 2).all()
    assert R.runs(f[T + 4].tolist()) == [(2, image.shape[1] + 1)] == R.runs(f[T + 5].tolist())


def test_identity_table_is_the_default_and_encode_label_pngs_splits_the_buffer(cuda, luts):
    from PIL import Image
    from dcfp_amd import evaluate, ops
    pred = CASES["rect_33x777"]
    d_pred = torch.from_numpy(pred).to(cuda)
    streams, offsets, lengths = ops.png_deflate_labels(d_pred)
    lengths = lengths.cpu().tolist()
    data = streams[:sum(lengths)].cpu().numpy().tobytes()
    assert len(lengths) == 2 and data[:lengths[0]] == R.deflate_labels((pred[0] & 255).astype(np.uint8))
    palette = [int(v) for v in np.random.RandomState(6).randint(0, 256, 3 * 19)]
    files = evaluate.encode_label_pngs(d_pred, luts, [palette, None])
    assert len(files) == 2 and all(len(f) == 2 for f in files)
    for n in range(2):
        for p in range(2):
            with Image.open(io.BytesIO(files[n][p])) as im:
                assert im.mode == "PL"[p] and np.array_equal(np.asarray(im), luts[p][pred[n] & 255])
                assert p == 1 or im.getpalette()[:57] == palette


def test_arguments_are_validated(cuda):
    from dcfp_amd import ops
    good = torch.zeros((1, 4, 4), dtype=torch.int32, device=cuda)
    for bad in (good.cpu(), good.long(), good[0], good.transpose(1, 2)[:, :, :2]):
        with pytest.raises(RuntimeError):
            ops.png_deflate_labels(bad)
    for bad in (torch.zeros((5, 256), dtype=torch.uint8, device=cuda), torch.zeros((1, 255), dtype=torch.uint8, device=cuda),
                torch.zeros((1, 256), dtype=torch.int32, device=cuda), torch.zeros((1, 256), dtype=torch.uint8)):
        with pytest.raises(RuntimeError):
            ops.png_deflate_labels(good, bad)
    with pytest.raises(RuntimeError):
        ops.png_deflate_labels(torch.zeros((1, 1, 8193), dtype=torch.int32, device=cuda))
