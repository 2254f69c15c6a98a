"""COCO-Stuff (`COCOdatasets.py` of the reference): 171 classes, a list of sample names, raw label k -> class k - 1."""
from .base import NameListDataSet


class DataSet(NameListDataSet):
    KEY, NUM_CLASSES = "COCO", 171
    LABEL_DIR, LABEL_SUFFIX = "annotations", "_labelTrainIds.png"
