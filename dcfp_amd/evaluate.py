"""Evaluation helpers — the device-side half of evaluate.py:113-143,145-247,340-380: whole-image, sliding-window and
multi-scale(+flip) prediction, on-device argmax and confusion matrix, mIoU.  Inference runs the
conv kernels with the eval-mode BatchNorm folded into their epilogues (one kernel per
conv+BN+ReLU); `predict_labels`, `predict_vote` and `predict_sliding_vote` never materialise the full-resolution
logits."""
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from math import ceil

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .networks import _exec
from .utils.edge_utils import mask_to_boundary


@torch.no_grad()
def predict_whole(net, image):
    """evaluate.py:186-196: full-resolution logits of the main head."""
    prediction = net(image)
    if isinstance(prediction, list):
        prediction = prediction[0]
    elif isinstance(prediction, dict):
        prediction = prediction["pred"]
    return prediction


def pad(image, target_size):
    """evaluate.py:113-117: zero padding at the bottom / right up to the tile size."""
    rows_missing = target_size[0] - image.shape[2]
    cols_missing = target_size[1] - image.shape[3]
    return F.pad(image, (0, cols_missing, 0, rows_missing), mode="constant", value=0.0).contiguous()


@torch.no_grad()
def predict_sliding(net, image, tile_size, classes):
    """evaluate.py:145-184: tiles of `tile_size` with 1/3 overlap (stride ceil(tile_h * 2/3) in both directions, as the
    reference computes it), the last row / column of tiles shifted back inside the image, every tile zero-padded to the
    tile size before the network sees it.  The reference sums the tiles' logits and the per-pixel tile count on the host;
    here both accumulators stay on the device, the image is never copied back."""
    image_size = image.shape
    overlap = 1 / 3
    stride = ceil(tile_size[0] * (1 - overlap))
    tile_rows = int(ceil((image_size[2] - tile_size[0]) / stride) + 1)
    tile_cols = int(ceil((image_size[3] - tile_size[1]) / stride) + 1)
    full_probs = torch.zeros((image_size[0], classes, image_size[2], image_size[3]), device=image.device)
    count = torch.zeros((1, 1, image_size[2], image_size[3]), device=image.device)
    for row in range(tile_rows):
        for col in range(tile_cols):
            x1, y1 = int(col * stride), int(row * stride)
            x2 = min(x1 + tile_size[1], image_size[3])
            y2 = min(y1 + tile_size[0], image_size[2])
            x1 = max(int(x2 - tile_size[1]), 0)
            y1 = max(int(y2 - tile_size[0]), 0)
            img = image[:, :, y1:y2, x1:x2]
            prediction = net(pad(img, tile_size))
            if isinstance(prediction, list):
                prediction = prediction[0]
            elif isinstance(prediction, dict):
                prediction = prediction["pred"]
            count[:, :, y1:y2, x1:x2] += 1
            full_probs[:, :, y1:y2, x1:x2] += prediction[:, :, 0:img.shape[2], 0:img.shape[3]]
    full_probs /= count
    return full_probs


@torch.no_grad()
def predict_multiscale(net, image, tile_size, scales, classes, flip_evaluation, align_corner, whole=True):
    """evaluate.py:198-227 (same signature): average over the scales of the logits of the resized image - whole-image
    or sliding-window - optionally averaged with the mirrored image's, resized back to the input size."""
    N_, C_, H_, W_ = image.shape
    full = torch.zeros((N_, classes, H_, W_), device=image.device)

    def run(im):
        return predict_whole(net, im) if whole else predict_sliding(net, im, tile_size, classes)
    for scale in scales:
        scale = float(scale)
        hs, ws = int(H_ * scale), int(W_ * scale)
        img = ops.upsample_bilinear(image, (hs, ws), align_corner)
        probs = run(img)
        if flip_evaluation:
            flipped = run(torch.flip(img, [3]))
            probs = 0.5 * (probs + torch.flip(flipped, [3]))
        full += ops.upsample_bilinear(probs, (H_, W_), align_corner)
    full /= len(scales)
    return full


def _vote_scales(image, scales, flip, align_corner):
    """Per scale of a fused vote, as predict_multiscale steps through them: (the image resized to the scale, its size
    (hs, ws), the weight of each of the scale's passes - the plain one and, with `flip`, the mirrored one)."""
    H_, W_ = image.shape[2:]
    for scale in scales:
        scale = float(scale)
        hs, ws = int(H_ * scale), int(W_ * scale)
        yield ops.upsample_bilinear(image, (hs, ws), align_corner), (hs, ws), (0.5 if flip else 1.0) / len(scales)


@torch.no_grad()
def predict_vote(net, image, scales, flip, align_corner, out_hw=None, labels=None, conf=None, want_scores=False,
                 ignore_index=255):
    """predict_multiscale(whole=True) + argmax (+ confusion matrix) without any N x C x hs x ws tensor: per scale the
    network's low-resolution logits of the resized image (and of its mirror image with `flip`), then ONE
    ops.multiscale_vote launch over all of them.  out_hw: the top-left crop of the image that is
    predicted (the unpadded size after pad_inf), default the whole image; labels int64 [N,out_h,out_w] with conf
    int64 [C,C]: counted into conf in the same launch.  -> (pred int32 [N,out_h,out_w], scores fp32
    [N,C,out_h,out_w] or None).  net: a Seg_Model or a deploy.Engine."""
    _exec.require_device(image)
    H_, W_ = image.shape[2:]
    maps = []
    for img, hw, weight in _vote_scales(image, scales, flip, align_corner):
        maps.append((net.lowres_logits(img)[0], hw, False, weight))
        if flip:
            maps.append((net.lowres_logits(torch.flip(img, [3]))[0], hw, True, weight))
    return ops.multiscale_vote(maps, (H_, W_), (H_, W_) if out_hw is None else out_hw, align_corner, labels=labels,
                               conf=conf, want_scores=want_scores, ignore_index=ignore_index)


def sliding_tiles(h, w, tile_size):
    """The tile grid of predict_sliding (evaluate.py:145-184) for an h x w image -> (ys, xs): tile t = r * len(xs) + c
    covers [ys[r], min(ys[r] + tile_h, h)) x [xs[c], min(xs[c] + tile_w, w)).  The stride ceil(tile_h * 2/3) serves both
    axes, as in the reference.  ValueError where the reference divides 0 by 0: a grid without tiles (an image much
    smaller than the tile) and a pixel under no tile (tile_w below the stride with more than one column)."""
    th, tw = int(tile_size[0]), int(tile_size[1])
    h, w = int(h), int(w)
    stride = ceil(th * (1 - 1 / 3))
    rows = int(ceil((h - th) / stride) + 1)
    cols = int(ceil((w - tw) / stride) + 1)
    what = "sliding_tiles: a %d x %d image with %d x %d tiles (stride %d)" % (h, w, th, tw, stride)
    if rows < 1 or cols < 1:
        raise ValueError(what + " has %d x %d tiles: the image is too small for the tile" % (rows, cols))
    ys = [max(min(r * stride + th, h) - th, 0) for r in range(rows)]
    xs = [max(min(c * stride + tw, w) - tw, 0) for c in range(cols)]
    for origins, extent, size in ((ys, th, h), (xs, tw, w)):
        covered = 0
        for o in origins:
            if o > covered:
                raise ValueError(what + " leaves pixels under no tile (from %d on along an axis of %d)" % (covered, size))
            covered = max(covered, min(o + extent, size))
        if covered < size:
            raise ValueError(what + " leaves pixels under no tile (from %d on along an axis of %d)" % (covered, size))
    return ys, xs


# predict_sliding_vote's default tile_batch: as many tile pixels per network call as a whole-image batch of four
# 1025 x 2049 images has - the activations the tools' default --batch-size 4 already asks for with --whole True
TILE_PIXELS_PER_CALL = 4 * 1025 * 2049


@torch.no_grad()
def predict_sliding_vote(net, image, tile_size, scales, flip, align_corner, out_hw=None, labels=None, conf=None,
                         want_scores=False, ignore_index=255, tile_batch=None):
    """predict_multiscale(whole=False) + argmax (+ confusion matrix) without any full-resolution logits: per scale the
    resized image is cut into the tiles of predict_sliding in one launch (and once more mirrored with `flip`), the
    network runs on the stacked tiles, at most `tile_batch` tiles x N images per call, and its low-resolution logits go
    into one [T,N,C,lh,lw] buffer per pass; then ONE ops.sliding_vote launch over all passes.  The other
    arguments and the result are predict_vote's.  tile_batch bounds the peak memory of the network's activations; the
    default keeps tiles x N x tile_h x tile_w within TILE_PIXELS_PER_CALL (769 x 769 tiles: 14 for one image, 3 for
    four).  Batching changes the network's input shape only, not its arithmetic per image.  RuntimeError where a limit
    of the launch is exceeded (ops.SLIDE_MAX_PASSES passes, ops.SLIDE_MAX_TILES_PER_AXIS tile rows / columns); ValueError from
    sliding_tiles.  net: a Seg_Model or a deploy.Engine."""
    _exec.require_device(image)
    N_, _, H_, W_ = image.shape
    th, tw = int(tile_size[0]), int(tile_size[1])
    n_passes = len(scales) * (2 if flip else 1)
    if not 1 <= n_passes <= ops.SLIDE_MAX_PASSES:
        raise RuntimeError("predict_sliding_vote: %d scales%s are %d passes, one launch takes 1 .. %d (SLIDE_MAX_PASSES)"
                           % (len(scales), " with flip" if flip else "", n_passes, ops.SLIDE_MAX_PASSES))
    if tile_batch is None:
        tile_batch = TILE_PIXELS_PER_CALL // (N_ * th * tw)
    tile_batch = max(1, int(tile_batch))
    passes = []
    for scale, (img, (hs, ws), weight) in zip(scales, _vote_scales(image, scales, flip, align_corner)):
        ys, xs = sliding_tiles(hs, ws, (th, tw))
        if max(len(ys), len(xs)) > ops.SLIDE_MAX_TILES_PER_AXIS:
            raise RuntimeError("predict_sliding_vote: %d x %d tiles at scale %g, one launch takes %d per axis "
                               "(SLIDE_MAX_TILES_PER_AXIS)" % (len(ys), len(xs), float(scale),
                                                               ops.SLIDE_MAX_TILES_PER_AXIS))
        T = len(ys) * len(xs)
        for mirrored in ((False, True) if flip else (False,)):
            tiles = ops.gather_tiles(img, ys, xs, (th, tw), mirrored)
            logits = None
            for t0 in range(0, T, tile_batch):
                t1 = min(T, t0 + tile_batch)
                low = net.lowres_logits(tiles[t0:t1].reshape((t1 - t0) * N_, tiles.shape[2], th, tw))[0]
                if t0 == 0 and t1 == T:
                    logits = low.reshape((T, N_) + tuple(low.shape[1:]))
                    break
                if logits is None:
                    logits = torch.empty((T, N_) + tuple(low.shape[1:]), dtype=torch.float32, device=image.device)
                logits[t0:t1] = low.reshape((t1 - t0, N_) + tuple(low.shape[1:]))
            del tiles
            passes.append((logits, (hs, ws), (th, tw), ys, xs, mirrored, weight))
    return ops.sliding_vote(passes, (H_, W_), (H_, W_) if out_hw is None else out_hw, align_corner, labels=labels,
                            conf=conf, want_scores=want_scores, ignore_index=ignore_index)


def pad_inf_size(h, w, stride=8):
    """evaluate.py:119-123: the next size of the form stride*k + 1 on both axes."""
    return h + (stride + 1 - h % stride) % stride, w + (stride + 1 - w % stride) % stride


def pad_inf(image):
    """evaluate.py:119-130: zero padding at the bottom / right up to 8k+1 on both axes."""
    return pad(image, pad_inf_size(image.shape[2], image.shape[3]))


def generate_size(h, w, size, mode):
    """evaluate.py:132-141: the size an image is resized to so that its long / short side becomes `size`."""
    if mode == "long":
        f_scale = size * 1.0 / max(h, w)
    elif mode == "short":
        f_scale = size * 1.0 / min(h, w)
    else:
        raise NotImplementedError(mode)
    return int(h * f_scale + 0.5), int(w * f_scale + 0.5)


def generate_size_image(image, size, mode):
    """evaluate.py:132-143 on the device."""
    return ops.upsample_bilinear(image, generate_size(image.shape[2], image.shape[3], size, mode), False)


def save_palette_png(pred, palette, path):
    """evaluate.py:346-350: a [H,W] class map as an 8-bit palette PNG (palette: flat list of R, G, B)."""
    from PIL import Image
    import numpy as np
    im = Image.fromarray(np.ascontiguousarray(np.asarray(pred, dtype=np.uint8)))
    im.putpalette([int(v) for v in palette])
    im.save(path)


_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_pinned = {}


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)))


def png_container(stream_bytes, H, W, palette=None):
    """An 8-bit PNG file around a finished zlib stream of H filtered rows of W bytes (ops.png_deflate_labels; DESIGN
    §15): colour type 3 with a PLTE chunk for `palette` (flat R, G, B list, at most 256 entries), grey without one.
    Pure host; the only pass over data is the CRC of the compressed bytes."""
    if H < 1 or W < 1:
        raise ValueError("png_container: H, W >= 1 expected, got %r x %r" % (H, W))
    chunks = [_PNG_SIGNATURE, _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0 if palette is None else 3, 0, 0, 0))]
    if palette is not None:
        plte = bytes(int(v) for v in palette)
        if len(plte) == 0 or len(plte) % 3 or len(plte) > 768:
            raise ValueError("png_container: a palette is 1 .. 256 R, G, B triples, got %d values" % len(plte))
        chunks.append(_png_chunk(b"PLTE", plte))
    chunks += [_png_chunk(b"IDAT", bytes(stream_bytes)), _png_chunk(b"IEND", b"")]
    return b"".join(chunks)


def reverse_id_table(dataset):
    """uint8 [256]: train id -> the dataset's label id, by the dataset's own id2trainId(reverse=True) - what
    evaluate_test.py:153 applies to a prediction before it saves the submission PNG."""
    return dataset.id2trainId(np.arange(256, dtype=np.uint8), reverse=True)


def encode_label_pngs(pred, luts, palettes):
    """pred int32 [N,H,W] on the device, luts uint8 [P,256] (tensor or array; None: the identity), palettes: P flat
    R, G, B lists or None (grey) -> [N][P] PNG files as bytes, file [n][p] showing luts[p][pred[n] & 255].  The streams
    are deflated on the device (ops.png_deflate_labels); two device-to-host copies per call - the P*N lengths, then
    exactly the compressed bytes into a pinned buffer - and the map itself never leaves the device."""
    if luts is not None and not isinstance(luts, torch.Tensor):
        luts = torch.from_numpy(np.ascontiguousarray(np.asarray(luts, dtype=np.uint8)))
    if luts is not None:
        luts = luts.reshape(-1, 256).to(pred.device).contiguous()
    P = 1 if luts is None else int(luts.shape[0])
    if len(palettes) != P:
        raise ValueError("encode_label_pngs: one palette (or None) per lookup table expected")
    N, H, W = (int(v) for v in pred.shape)
    streams, _, lengths = ops.png_deflate_labels(pred, luts)
    lengths = lengths.cpu().tolist()                                      # copy 1 (synchronises)
    total = int(sum(lengths))
    key = (pred.device.index, torch.cuda.current_stream().cuda_stream)
    host = _pinned.get(key)
    if host is None or host.numel() < total:
        host = _pinned[key] = torch.empty(max(total, 1 << 20), dtype=torch.uint8).pin_memory()
    host[:total].copy_(streams[:total], non_blocking=True)                # copy 2
    torch.cuda.current_stream().synchronize()
    raw = host.numpy()
    files, at = [], 0
    for n in range(N):
        files.append([])
        for p in range(P):
            s = n * P + p
            files[n].append(png_container(raw[at:at + lengths[s]].tobytes(), H, W, palettes[p]))
            at += lengths[s]
    return files


class PngWriter:
    """Writes finished byte strings to paths on at most 4 threads of its own, so that the next batch does not wait for
    the file system.  drain() waits for everything handed in and re-raises the first exception; leaving the `with`
    block drains."""

    def __init__(self, threads=4):
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(4, int(threads))))
        self.pending = []

    @staticmethod
    def _write(path, data):
        with open(path, "wb") as f:
            f.write(data)

    def write(self, path, data):
        self.pending.append(self.pool.submit(self._write, path, data))

    def drain(self):
        pending, self.pending = self.pending, []
        errors = []
        for f in pending:
            try:
                f.result()
            except Exception as e:  # noqa: BLE001  (every write is waited for before the first error is raised)
                errors.append(e)
        if errors:
            raise errors[0]

    def close(self):
        try:
            self.drain()
        finally:
            self.pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


@torch.no_grad()
def predict_labels(net, image):
    """argmax of predict_whole without the N x C x H x W tensor: low-resolution logits of the
    main head -> fused upsample+argmax kernel -> int32 [N,H,W]."""
    _exec.require_device(image)
    lowres = net.lowres_logits(image)[0]
    return ops.upsample_argmax(lowres, image.shape[2:], net.align_corner)


def get_confusion_matrix(gt_label, pred_label, class_num, ignore_index=255, out=None):
    """evaluate.py:229-247 on the device (int64 [C,C]); pixels with gt == ignore are skipped, as the
    reference does by masking before the call (evaluate.py:344-347)."""
    return ops.confusion_matrix(pred_label.to(torch.int32), gt_label.to(torch.int64), class_num,
                                ignore_index, out)


def mean_iou(confusion_matrix):
    """evaluate.py:374-380: IoU per class = tp / (pos + res - tp); mean over classes."""
    cm = confusion_matrix.double()
    pos, res, tp = cm.sum(1), cm.sum(0), cm.diag()
    iou = tp / torch.clamp(pos + res - tp, min=1.0)
    return iou.mean().item(), iou


def boundary_confusion_matrix(gt_label, pred_label, class_num, dilation_ratio=0.02, ignore_index=255, out=None):
    """evaluate.py:352-362 on the device -> int64 [C, C+1].  Both maps are reduced to their class boundaries
    (utils.edge_utils.mask_to_boundary); what is left of the ground truth is counted, everything else of it is
    ignore.  A counted pixel that the prediction does not mark as boundary is a miss of its ground-truth class and
    lands in column C (the reference lets 255 alias into gt*C + pred there)."""
    gt_b = mask_to_boundary(gt_label.to(torch.int64), class_num, dilation_ratio, ignore_index)
    pred_b = mask_to_boundary(pred_label.to(torch.int32), class_num, dilation_ratio, class_num)
    if out is not None and (out.dtype != torch.int64 or tuple(out.shape) != (class_num, class_num + 1)
                            or not out.is_contiguous()):
        raise RuntimeError("boundary_confusion_matrix: out must be a contiguous int64 [C, C+1] tensor")
    # the [C, C+1] matrix is the first C rows of the (C+1)-class one: its last row (gt == C) stays empty because
    # the ground truth holds classes below C or ignore only
    full = torch.zeros((class_num + 1, class_num + 1), dtype=torch.int64, device=gt_b.device)
    ops.confusion_matrix(pred_b, gt_b, class_num + 1, ignore_index, full)
    if out is None:
        return full[:class_num].clone()
    out += full[:class_num]
    return out


def boundary_iou(confusion_matrix):
    """IoU per class over boundary pixels from the [C, C+1] matrix: tp / max(1, pos + res - tp) with pos the row
    sums (misses included) and res the column sums over the class columns."""
    cm = confusion_matrix.double()
    Cn = cm.shape[0]
    pos, res, tp = cm.sum(1), cm[:, :Cn].sum(0), cm[:, :Cn].diag()
    iou = tp / torch.clamp(pos + res - tp, min=1.0)
    return iou.mean().item(), iou
