"""dcfp_amd.datasets: the data layer of the reference (`datasets/`) with the augmentation chain on the device.

`build_dataset` has the reference's signature; the dataset root and list file come from `data_para` (keys `root`,
`list_path`) instead of the reference's machine-specific `mypath.Path`.  Cityscapes (`CS`, 19 classes), Pascal-Context
(`CTX`, 59) and COCO-Stuff (`COCO`, 171) are built.  ADE20K (`ADE`, 150) is not: `build_dataset("ADE", ...)` raises
NotImplementedError (pinned by tests/test_datasets_host_cpu.py); the kernels and heads serve 150 classes all the same.
`data_para={"resample": true}` selects the reference's class-balanced `resample` sampler; it needs the class index
that `tools/label_index.py` writes next to the list file."""
from . import coco as COCOdatasets
from . import cs as CSdatasets
from . import ctx as CTXdatasets
from .base import AugConfig, AugParams, BaseDataSet, draw_crop, draw_params, draw_pre  # noqa: F401
from .loader import EvalLoader, TrainLoader  # noqa: F401

_DATASETS = {"CS": CSdatasets, "CTX": CTXdatasets, "COCO": COCOdatasets}


def build_dataset(dataset, split="val", data_dir="val", crop_size=(512, 512), scale=False, mirror=False,
                  brightness=False, ignore_label=255, balance=0, longsize=-1, shortsize=-1, data_para={}):
    if dataset not in _DATASETS:
        raise NotImplementedError("dataset %r: only %s are built (DESIGN §13)" % (dataset, sorted(_DATASETS)))
    para = dict(data_para)
    try:
        root, list_path = para.pop("root"), para.pop("list_path")
    except KeyError:
        raise ValueError("data_para must name the dataset's `root` and `list_path` (split %r of %r)" % (data_dir, dataset))
    return _DATASETS[dataset].DataSet(root, list_path, split=split, crop_size=crop_size, scale=scale, mirror=mirror,
                                      brightness=brightness, ignore_label=ignore_label, balance=balance,
                                      longsize=longsize, shortsize=shortsize, **para)
