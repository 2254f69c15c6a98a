"""TrainLoader: host threads decode, one pinned staging buffer and one copy per batch, the device does the rest.

A batch costs the host the file decoding, the random draws and a few KiB of tables (base.pack_batch); sources, label
maps and tables travel in one pinned uint8 buffer and ops.augment_batch / ops.balance_weight produce the tensors the
model takes.  Indices are sharded by rank the way torch's DistributedSampler does (seeded permutation per epoch, padded
to a multiple of the world size, rank-strided)."""
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch


def _align16(n):
    return (n + 15) & ~15


class TrainLoader:
    def __init__(self, dataset, batch_size, device, seed=0, num_workers=4, rank=None, world_size=None, shuffle=True,
                 target_class=None):
        """target_class: for balance == 2, an int or a callable (dataset index) -> class; the reference takes it from
        its `resample` sampler, which is out of scope."""
        import torch.distributed as dist
        if rank is None or world_size is None:
            on = dist.is_available() and dist.is_initialized()
            rank, world_size = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
        if dataset.balance == 2 and target_class is None:
            raise ValueError("balance=2 needs target_class (the `resample` sampler is out of scope)")
        self.dataset, self.batch_size, self.device = dataset, int(batch_size), torch.device(device)
        self.seed, self.rank, self.world_size, self.shuffle = int(seed), int(rank), int(world_size), shuffle
        self.target_class = target_class
        self.epoch = 0
        self.rng = random.Random(self.seed + self.rank)          # the augmentation draws, in sample order
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(num_workers)))
        self.num_samples = -(-len(dataset) // self.world_size)
        self._id_table = None

    def __len__(self):
        return self.num_samples // self.batch_size

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

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
        return [self.pool.submit(self.dataset.decode, i) for i in idx]

    def __iter__(self):
        idx = self.indices(self.epoch)
        self.epoch += 1
        batches = [idx[i:i + self.batch_size] for i in range(0, len(self) * self.batch_size, self.batch_size)]
        pending = self._submit(batches[0]) if batches else None
        for b, cur in enumerate(batches):
            decoded = [f.result() for f in pending]
            pending = self._submit(batches[b + 1]) if b + 1 < len(batches) else None     # decode ahead of the device
            yield self.collate(decoded, cur)

    def collate(self, decoded, idx=None):
        """decoded: [(uint8 [H,W,3] BGR, uint8 [H,W] or None)] -> (images, labels) on the device."""
        ds = self.dataset
        hws = [im.shape[:2] for im, _ in decoded]
        params = [ds.draw_params(self.rng, hw) for hw in hws]
        return self.apply(decoded, params, idx)

    def apply(self, decoded, params, idx=None):
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
        parts += [im.reshape(-1) for im, _ in decoded]
        if with_labels:
            parts += [lab.reshape(-1) for _, lab in decoded]
        offs, total = [], 0
        for p in parts:
            offs.append(total)
            total += _align16(p.size)
        stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()
        for p, o in zip(parts, offs):
            host[o:o + p.size] = p
        dev = stage.to(self.device, non_blocking=True)
        views = [dev[o:o + p.size] for p, o in zip(parts, offs)]
        d_taps = views.pop(0).view(torch.int32).view(-1, 4)
        d_lut_b = views.pop(0).view(torch.float32)
        d_lut_a = views.pop(0) if lut_a is not None else None
        n = len(decoded)
        d_images = [views[i].view(hws[i][0], hws[i][1], 3) for i in range(n)]
        d_labels = [views[n + i].view(hws[i][0], hws[i][1]) for i in range(n)] if with_labels else None
        if self._id_table is None:
            self._id_table = torch.from_numpy(ds.id_table()).to(self.device)
        images, labels, hist = ops.augment_batch(d_images, d_labels, recs, d_taps, d_lut_a, d_lut_b, self._id_table,
                                                 crop, ds.ignore_label)
        if not with_labels:
            return images, None
        if ds.balance > 0 and ds.split == "train":
            target = None
            if ds.balance == 2:
                t = self.target_class
                target = [t(i) if callable(t) else int(t) for i in (idx if idx is not None else range(n))]
            weight = ops.balance_weight(labels, hist, ds.num_classes, ds.balance, ds.ignore_label, target, ds.beta)
            return images, {"ori": labels, "weight": weight}
        return images, labels
