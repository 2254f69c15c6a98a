"""Cityscapes (`CSdatasets.py` of the reference): 19 classes, the id -> trainId table, list-file parsing, decoding."""
import os.path as osp

import numpy as np

from .base import BaseDataSet

CLASS_WEIGHTS = [0.8373, 0.918, 0.866, 1.0345, 1.0166, 0.9969, 0.9754, 1.0489, 0.8786, 1.0023, 0.9539, 0.9843,
                 1.1116, 0.9037, 1.0865, 1.0955, 1.0865, 1.1529, 1.0507]
_TRAIN_IDS = {7: 0, 8: 1, 11: 2, 12: 3, 13: 4, 17: 5, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13,
              27: 14, 28: 15, 31: 16, 32: 17, 33: 18}


class DataSet(BaseDataSet):
    def __init__(self, root, list_path, max_iters=None, split="train", crop_size=(321, 321),
                 mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), scale=True, mirror=True, brightness=True,
                 ignore_label=255, balance=0, longsize=-1, shortsize=-1, **kwargs):
        super().__init__(split=split, crop_size=crop_size, mean=mean, std=std, scale=scale, mirror=mirror,
                         brightness=brightness, ignore_label=ignore_label, balance=balance, longsize=longsize,
                         shortsize=shortsize, **kwargs)
        self.num_classes = 19
        self.root, self.list_path = root, list_path
        self._class_weights = None
        self.id_to_trainid = {k: _TRAIN_IDS.get(k, ignore_label) for k in range(-1, 34)}
        self.cmap_labels = np.array([[128, 64, 128], [244, 35, 232], [70, 70, 70], [102, 102, 156], [190, 153, 153],
                                     [153, 153, 153], [250, 170, 30], [220, 220, 0], [107, 142, 35], [152, 251, 152],
                                     [70, 130, 180], [220, 20, 60], [255, 0, 0], [0, 0, 142], [0, 0, 70],
                                     [0, 60, 100], [0, 80, 100], [0, 0, 230], [119, 11, 32]])
        with open(list_path) as f:
            lines = [line.strip().split() for line in f if line.strip()]
        self.files = []
        if split == "test":
            self.img_ids = [item[0] for item in lines]
            for image_path in self.img_ids:
                self.files.append({"img": osp.join(root, image_path),
                                   "name": osp.splitext(osp.basename(image_path))[0]})
        else:
            self.img_ids = lines
            if max_iters is not None:
                self.img_ids = self.img_ids * int(np.ceil(float(max_iters) / len(self.img_ids)))
            for image_path, label_path in self.img_ids:
                self.files.append({"img": osp.join(root, image_path), "label": osp.join(root, label_path),
                                   "name": osp.splitext(osp.basename(label_path))[0]})
        if self.resample:
            self.load_index(osp.join(osp.dirname(list_path),
                                     "label_index_CStest.pkl" if split == "test" else "label_index_CS.pkl"))

    @property
    def class_weights(self):
        """The reference's per-class loss weights, on the current device (built on first use: the dataset itself
        needs no GPU)."""
        import torch
        if self._class_weights is None:
            self._class_weights = torch.tensor(CLASS_WEIGHTS, dtype=torch.float32,
                                               device="cuda" if torch.cuda.is_available() else "cpu")
        return self._class_weights
