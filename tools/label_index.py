#!/usr/bin/env python
"""Write the class index of the `resample` sampler: label_index_<DATASET>.pkl.

For every file of the train list: id -> trainId, ignore -> num_classes, bincount; the file joins the list of every
class it holds.  The pickle is a plain dict {str(class): [{'idx': file index, 'name': file name}, ...], 'label_f':
float64 [num_classes] list lengths}, the format of the reference's label_index.py: a file written by either side loads
in the other.  The dataset looks for it in the directory of its list file.

    python tools/label_index.py --dataset CS|CTX|COCO --data-para '{"root": ..., "list_path": ".../train.lst"}' --save-dir ...

Host numpy: this runs once per dataset."""
import argparse
import json
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def get_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--dataset", type=str, default="CS")
    p.add_argument("--save-dir", type=str, default=None, help="default: the directory of the list file")
    p.add_argument("--data-para", type=str, default="{}", help='JSON: "root" and "list_path" of the dataset')
    return p


def build_index(dataset):
    index = {str(c): [] for c in range(dataset.num_classes)}
    for idx, item in enumerate(dataset.files):
        label = dataset.id2trainId(dataset.decode(idx)[1])
        label[label == dataset.ignore_label] = dataset.num_classes
        count = np.bincount(label.reshape(-1), minlength=dataset.num_classes + 1)[:dataset.num_classes]
        for c in np.flatnonzero(count > 0):
            index[str(int(c))].append({"idx": idx, "name": item["name"]})
    index["label_f"] = np.array([len(index[str(c)]) for c in range(dataset.num_classes)], dtype=np.float64)
    return index


def main(argv=None):
    from dcfp_amd.datasets import build_dataset
    args = get_parser().parse_args(argv)
    para = json.loads(args.data_para)
    para.pop("resample", None)                       # the index is what `resample` needs: build the plain dataset
    dataset = build_dataset(args.dataset, split="train", data_dir="train", data_para=para)
    index = build_index(dataset)
    save_dir = args.save_dir or os.path.dirname(os.path.abspath(para["list_path"]))
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, "label_index_%s.pkl" % args.dataset)
    with open(path, "wb") as f:
        pickle.dump(index, f)
    empty = [c for c in range(dataset.num_classes) if not index[str(c)]]
    print("%s: %d files, list lengths %s" % (path, len(dataset.files), index["label_f"].astype(int).tolist()))
    if empty:
        print("classes in no file (resample=True will refuse this index): %s" % empty)
    return path


if __name__ == "__main__":
    main()
