"""Pascal-Context (`CTXdatasets.py` of the reference): 59 classes, a list of sample names, raw label k -> class k - 1."""
from .base import NameListDataSet


class DataSet(NameListDataSet):
    KEY, NUM_CLASSES = "CTX", 59
    LABEL_DIR, LABEL_SUFFIX = "labels", ".png"
