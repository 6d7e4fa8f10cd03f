"""MI355X-native (gfx950) inference engine for the DBNet++ -> SVTRv2 -> CTC invoice OCR hot path.

Importing the package is cheap and CPU-safe; ``DBNetPP`` / ``SVTRv2`` / ``Engine`` (batched OCR over pages of mixed sizes) load ``lib/libocrvi.so`` on first use and
raise if it is missing (there is no CPU fallback).  ``DBLoss`` / ``SVTRv2Loss`` / ``compute_metrics`` / ``compute_cer`` / ``compute_acc`` /
``validate_detection`` / ``validate_recognition`` (``val.py``) mirror the reference's validation loops on the device; ``DetectionDataset``
(``data.py``) builds the detection batches they consume from polygon annotations.  ``find_document_contour`` / ``document_mask`` /
``find_document_quad`` / ``find_document_quads`` (``pipeline.py``) find the document's corners for the rectification stage;
``estimate_skew`` / ``estimate_skews`` / ``skew_quad`` / ``deskew`` estimate a page's rotation and straighten it."""
from .vocab import VOCAB, Tokenizer  # noqa: F401


def __getattr__(name):
    if name == "DBNetPP":
        from .det import DBNetPP
        return DBNetPP
    if name == "SVTRv2":
        from .rec import SVTRv2
        return SVTRv2
    if name == "Engine":
        from .engine import Engine
        return Engine
    if name == "DetectionDataset":   # the reference's detection dataloader without augmentation: validation batches from polygons (data.py)
        from .data import DetectionDataset
        return DetectionDataset
    if name in _VAL_NAMES:      # validation: the reference's loss values, pixel metrics, CER and accuracy (val.py)
        from . import val
        return getattr(val, name)
    if name in _DOCFIND_NAMES:  # the document finder: mask -> corners on the host, the library's own mask on the device (pipeline.py)
        from . import pipeline
        return getattr(pipeline, name)
    if name in _SKEW_NAMES:     # the skew estimate: scores on the device, pick and quad on the host (pipeline.py)
        from . import pipeline
        return getattr(pipeline, name)
    raise AttributeError(name)


_VAL_NAMES = ("DBLoss", "compute_metrics", "SVTRv2Loss", "compute_cer", "compute_acc", "validate_detection", "validate_recognition")
_SKEW_NAMES = ("Skew", "estimate_skew", "estimate_skews", "skew_quad", "deskew")
_DOCFIND_NAMES = ("find_document_contour", "document_mask", "find_document_quad", "find_document_quads")
