"""The cases of tests/golden/jpeg_encode_cases.npz and the reference's encode of each, computed once and shared by
tests/test_jpeg_encode_cpu.py and tests/test_gpu_jpeg_encode.py.  Reads the archive only (no PIL)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpegenc_ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "jpeg_encode_cases.npz"))
NAMES = [str(n) for n in Z["names"]]
KIND = {str(n): str(k) for n, k in zip(Z["names"], Z["kinds"])}
MODE = {str(n): str(m) for n, m in zip(Z["names"], Z["modes"])}
QUALITY = {str(n): int(q) for n, q in zip(Z["names"], Z["quality"])}
SUB = {"420": "4:2:0", "444": "4:4:4", "grey": "4:2:0"}
PAGE = "page_500x380_420_q95"

_REF = {}


def image(name) -> np.ndarray:
    if KIND[name] == "sha":
        from ocr_vi_invoice_amd import synth
        assert name == PAGE
        return synth.make_invoice(7, 500, 380, lines=14)[0]
    return Z["i_" + name]


def ref(name):
    """The reference's encode of a case, computed once; callers leave it unchanged."""
    if name not in _REF:
        _REF[name] = jpegenc_ref.encode(image(name), QUALITY[name], SUB[MODE[name]])
    return _REF[name]
