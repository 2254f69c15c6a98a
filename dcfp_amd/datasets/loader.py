"""TrainLoader / EvalLoader: host threads decode, one pinned staging buffer and one copy per batch, the device does the rest.

A batch costs the host the file decoding, the random draws and a few KiB of tables (base.pack_batch); sources, label
maps and tables travel in one pinned uint8 buffer and ops.augment_batch / ops.balance_weight produce the tensors the
model takes.  Indices are sharded by rank the way torch's DistributedSampler does (seeded permutation per epoch, padded
to a multiple of the world size, rank-strided).

With a `resample` dataset the indices run over the dataset's epoch index (`pre_processing` at the start of every epoch,
`locate(i)` -> file and class), the class is the `balance=2` target, and a batch is built in stages, because the crop
offset depends on the device's answer: pre-crop draws; one staged copy of sources, label maps and nearest
maps; ops.label_components; counts, then sizes, to the host; the n and k draws; ops.component_pixel; jitter and mirror
draws; tables, ops.augment_batch and ops.balance_weight as before.  That is three small blocking copies per batch
(counts; the sizes gathered right after; the pixels) in two round-trip stages - the accepted cost of placing the crop on
the device's labelling.  Each sample of such a batch draws from its own child generator,
random.Random(self.rng.getrandbits(64)), created in sample order, so that no sample's draws wait for another's answer;
the order within a sample is the reference's.

EvalLoader serves the `val` and `test` splits through the same staging and the same kernel (identity tables, id ->
trainId, normalisation through LUT B): in file order, every file exactly once across the ranks (rank r takes r,
r + world, ...; no wrap-around padding, the last batch may be short), a batch cut where the source size changes."""
import random
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch


def _align16(n):
    return (n + 15) & ~15


class TrainLoader:
    def __init__(self, dataset, batch_size, device, seed=0, num_workers=4, rank=None, world_size=None, shuffle=True,
                 target_class=None):
        """target_class: for balance == 2 on a dataset without `resample`, an int or a callable (dataset index) ->
        class; a `resample` dataset brings the class of every sample itself (dataset.locate)."""
        import torch.distributed as dist
        if rank is None or world_size is None:
            on = dist.is_available() and dist.is_initialized()
            rank, world_size = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
        self.resample = bool(getattr(dataset, "resample", False))
        if dataset.balance == 2 and target_class is None and not self.resample:
            raise ValueError("balance=2 needs a `resample` dataset or target_class")
        self.dataset, self.batch_size, self.device = dataset, int(batch_size), torch.device(device)
        self.seed, self.rank, self.world_size, self.shuffle = int(seed), int(rank), int(world_size), shuffle
        self.target_class = target_class
        self.epoch = 0
        self.rng = random.Random(self.seed + self.rank)          # the augmentation draws, in sample order
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(num_workers)))
        if self.resample:
            dataset.seed = self.seed                                 # every rank builds the same epoch index
        self.num_samples = -(-len(dataset) // self.world_size)
        self._id_table = None
        self.last_pixels = None          # resample: the pixel every sample's crop was placed on (None: plain draws)
        self._cursor = None              # (epoch being iterated, batches of it already yielded); None: between epochs
        self._skip = 0                   # batches the next __iter__ leaves out (load_state_dict)

    def __len__(self):
        return self.num_samples // self.batch_size

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        self._cursor, self._skip = None, 0

    def state_dict(self):
        """Where the loader stands: the epoch, the batches of it already yielded and the draw generator's state.  That is
        all of it: the order of an epoch (and a `resample` dataset's epoch index) is a function of (seed, epoch), and the
        draws of a batch - the per-sample child generators of the `resample` path included - are taken from `self.rng`
        when the batch is collated, never for a batch that is only decoding ahead."""
        epoch, batch = self._cursor if self._cursor is not None else (self.epoch, self._skip)
        if batch >= len(self):           # the epoch's last batch has been yielded: the next one starts
            epoch, batch = epoch + 1, 0
        return {"epoch": int(epoch), "batch": int(batch), "rng": self.rng.getstate()}

    def load_state_dict(self, state):
        """The next __iter__ continues the epoch of `state` behind its cursor; the batches before it are not decoded."""
        epoch, batch = int(state["epoch"]), int(state["batch"])
        if epoch < 0 or not 0 <= batch < max(1, len(self)):
            raise ValueError("TrainLoader.load_state_dict: batch %d of epoch %d does not exist (%d batches per epoch)"
                             % (batch, epoch, len(self)))
        rng = state["rng"]
        self.rng.setstate((rng[0], tuple(rng[1]), rng[2]))
        self.epoch, self._skip, self._cursor = epoch, batch, None

    def indices(self, epoch):
        """This rank's sample order of one epoch (DistributedSampler's: permutation, wrap-around padding, stride)."""
        n = len(self.dataset)
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + int(epoch))
            order = torch.randperm(n, generator=g).tolist()
        else:
            order = list(range(n))
        total = self.num_samples * self.world_size
        while len(order) < total:
            order += order[:total - len(order)]
        return order[self.rank:total:self.world_size]

    def _submit(self, idx):
        return [self.pool.submit(self.dataset.decode, self.dataset.locate(i)[0]) for i in idx]

    def __iter__(self):
        self.dataset.pre_processing(self.epoch, None)
        idx = self.indices(self.epoch)
        epoch, first = self.epoch, self._skip
        self.epoch += 1
        self._skip = 0
        self._cursor = (epoch, first)
        batches = [idx[i:i + self.batch_size] for i in range(0, len(self) * self.batch_size, self.batch_size)]
        batches = batches[first:]                          # a restored cursor: the batches before it are never decoded
        pending = self._submit(batches[0]) if batches else None
        for b, cur in enumerate(batches):
            decoded = [f.result() for f in pending]
            pending = self._submit(batches[b + 1]) if b + 1 < len(batches) else None     # decode ahead of the device
            out = self.collate(decoded, cur)
            self._cursor = (epoch, first + b + 1)
            yield out
        self._cursor = None

    def collate(self, decoded, idx=None):
        """decoded: [(uint8 [H,W,3] BGR, uint8 [H,W] or None)] -> (images, labels) on the device."""
        ds = self.dataset
        hws = [im.shape[:2] for im, _ in decoded]
        if self.resample and ds.split == "train":
            return self.collate_resample(decoded, idx)
        params = [ds.draw_params(self.rng, hw) for hw in hws]
        return self.apply(decoded, params, idx)

    def collate_resample(self, decoded, idx):
        """The staged batch of a `resample` dataset (module docstring); idx: the batch's indices into the epoch index."""
        from .. import ops
        from . import base
        ds, cfg = self.dataset, self.dataset.aug_config
        hws = [im.shape[:2] for im, _ in decoded]
        n = len(decoded)
        classes = [ds.locate(i)[1] for i in idx]
        rngs = [random.Random(self.rng.getrandbits(64)) for _ in range(n)]
        params = [base.draw_pre(r, hw, cfg) for r, hw in zip(rngs, hws)]
        maps, recs, off = [], [], 0
        for p, (H, W), c in zip(params, hws, classes):
            maps += [base.resize_taps(H, p.dst_h, p.f_scale)[:, 3], base.resize_taps(W, p.dst_w, p.f_scale)[:, 3]]
            recs.append((p.dst_h, p.dst_w, max(p.dst_h, cfg.crop_h), max(p.dst_w, cfg.crop_w), off, off + p.dst_h, c))
            off += p.dst_h + p.dst_w
        views = self._stage([np.ascontiguousarray(np.concatenate(maps)).view(np.uint8)] +
                            [im.reshape(-1) for im, _ in decoded] + [lab.reshape(-1) for _, lab in decoded])
        d_maps = views[0].view(torch.int32)
        d_images = [views[1 + i].view(hws[i][0], hws[i][1], 3) for i in range(n)]
        d_labels = [views[1 + n + i].view(hws[i][0], hws[i][1]) for i in range(n)]
        comp = ops.label_components(d_labels, recs, d_maps, self._device_id_table(), ds.ignore_label)

        steps = [base.crop_steps(r, p, cfg) for r, p in zip(rngs, params)]
        asked, pixels = [next(g) for g in steps], [None] * n

        def answer(values):
            for i, g in enumerate(steps):
                if asked[i] is None:
                    continue
                try:
                    asked[i] = g.send(values[i])
                except StopIteration as done:
                    asked[i], pixels[i] = None, done.value
        answer(comp.counts())
        if any(q is not None for q in asked):
            answer(comp.sizes([q[1] if q else 0 for q in asked]))
            yx = ops.component_pixel(comp, [q[1] if q else 0 for q in asked], [q[2] if q else 0 for q in asked])
            answer(yx.tolist())
        self.last_pixels = pixels
        return self.apply(decoded, params, idx, sources=(d_images, d_labels), target=classes)

    def _device_id_table(self):
        if self._id_table is None:
            self._id_table = torch.from_numpy(self.dataset.id_table()).to(self.device)
        return self._id_table

    def _stage(self, parts):
        """uint8 arrays -> their device views: one pinned buffer, one copy."""
        offs, total = [], 0
        for p in parts:
            offs.append(total)
            total += _align16(p.size)
        stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()
        for p, o in zip(parts, offs):
            host[o:o + p.size] = p
        dev = stage.to(self.device, non_blocking=True)
        return [dev[o:o + p.size] for p, o in zip(parts, offs)]

    def apply(self, decoded, params, idx=None, sources=None, target=None):
        """sources: (images, label maps) already on the device (the resample path staged them before the crop draws);
        target: the balance=2 classes of the samples, else they come from `target_class`."""
        ds = self.dataset
        from .. import ops
        hws = [im.shape[:2] for im, _ in decoded]
        crop = (ds.crop_h, ds.crop_w)
        if ds.split != "train":
            crop = tuple(hws[0])
            if any(tuple(hw) != crop for hw in hws):
                raise ValueError("a %s batch takes sources of one size" % ds.split)
        taps, lut_a, lut_b, recs = ds.pack_batch(params, hws, crop)
        with_labels = decoded[0][1] is not None
        parts = [taps.view(np.uint8).reshape(-1), lut_b.view(np.uint8).reshape(-1)]
        if lut_a is not None:
            parts.append(lut_a)
        if sources is None:
            parts += [im.reshape(-1) for im, _ in decoded]
            if with_labels:
                parts += [lab.reshape(-1) for _, lab in decoded]
        views = self._stage(parts)
        d_taps = views.pop(0).view(torch.int32).view(-1, 4)
        d_lut_b = views.pop(0).view(torch.float32)
        d_lut_a = views.pop(0) if lut_a is not None else None
        n = len(decoded)
        if sources is None:
            d_images = [views[i].view(hws[i][0], hws[i][1], 3) for i in range(n)]
            d_labels = [views[n + i].view(hws[i][0], hws[i][1]) for i in range(n)] if with_labels else None
        else:
            d_images, d_labels = sources
        images, labels, hist = ops.augment_batch(d_images, d_labels, recs, d_taps, d_lut_a, d_lut_b,
                                                 self._device_id_table(), crop, ds.ignore_label)
        if not with_labels:
            return images, None
        if ds.balance > 0 and ds.split == "train":
            if ds.balance == 2 and target is None:
                t = self.target_class
                if t is None:
                    target = [ds.locate(i)[1] for i in idx]
                else:
                    target = [t(i) if callable(t) else int(t) for i in (idx if idx is not None else range(n))]
            weight = ops.balance_weight(labels, hist, ds.num_classes, ds.balance, ds.ignore_label,
                                        target if ds.balance == 2 else None, ds.beta)
            return images, {"ori": labels, "weight": weight}
        return images, labels


def cut_batches(stream, batch_size, key):
    """Consecutive items of `stream` in lists of at most batch_size that agree in key(item)."""
    batch = []
    for item in stream:
        if batch and (len(batch) == batch_size or key(item) != key(batch[0])):
            yield batch
            batch = []
        batch.append(item)
    if batch:
        yield batch


class EvalLoader(TrainLoader):
    """Batches of a `val` / `test` dataset: (images fp32 [n,3,H,W], labels int64 [n,H,W] or None, metas) with
    metas[i] = {'name', 'size': (H, W)}.  Every file is served exactly once across the ranks - unlike the reference's
    DistributedSampler, which repeats files to even the shards and so counts them twice in the confusion matrix
    (DESIGN §12)."""

    def __init__(self, dataset, batch_size, device, num_workers=4, rank=None, world_size=None):
        if dataset.split not in ("val", "test"):
            raise ValueError("EvalLoader serves the val and test splits, not %r" % (dataset.split,))
        if int(batch_size) < 1:
            raise ValueError("EvalLoader: batch_size must be at least 1")
        super().__init__(dataset, batch_size, device, seed=0, num_workers=num_workers, rank=rank, world_size=world_size,
                         shuffle=False, target_class=0)      # (balance weights are a train-split matter: no target)
        self.ahead = 2 * self.batch_size

    def indices(self, epoch=0):
        """This rank's files, in file order: r, r + world, ..."""
        return list(range(self.rank, len(self.dataset.files), self.world_size))

    def batches(self, sizes):
        """The batches (lists of file indices) this rank serves when file i has size sizes[i]."""
        return list(cut_batches(self.indices(), self.batch_size, lambda i: tuple(sizes[i])))

    def __len__(self):
        """Batches of this rank if all files have one size (a size change adds one)."""
        return -(-len(self.indices()) // self.batch_size)

    def _decoded(self):
        """(file index, decoded) in order, `ahead` files decoding on the pool beyond the one handed out."""
        idx, pending, nxt = self.indices(), deque(), 0
        while pending or nxt < len(idx):
            while nxt < len(idx) and len(pending) <= self.ahead:
                pending.append((idx[nxt], self.pool.submit(self.dataset.decode, idx[nxt])))
                nxt += 1
            i, f = pending.popleft()
            yield i, f.result()

    def __iter__(self):
        for batch in cut_batches(self._decoded(), self.batch_size, lambda it: it[1][0].shape[:2]):
            decoded = [d for _, d in batch]
            images, labels = self.collate(decoded, [i for i, _ in batch])
            metas = [{"name": self.dataset.files[i]["name"], "size": tuple(int(v) for v in d[0].shape[:2])}
                     for i, d in batch]
            yield images, labels, metas
