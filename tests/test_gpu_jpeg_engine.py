"""Engine.run on JPEG bytes (ocr_vi_invoice_amd/engine.py) against Engine.run on the arrays pipeline.imdecode returns for the same files:
the same boxes, scores and strings, whatever the mix of arrays and files, with and without captured graphs, for a page that is turned by
its EXIF orientation and rectified.  The files are three synthetic invoices of tests/golden/jpeg_cases.npz; random weights give a map
without text structure, so bars are blended into it as tests/test_gpu_engine.py does (kernel + 0.25 binary)."""
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DET_SIZE = 320
Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz"))
FILES = ["page_500x380", "inv1_420x320", "inv2_320x420"]
# page 2 is stored 320 x 420 and carries EXIF orientation 6: it decodes to 420 x 320; its document's corners are given in that page
QUADS = [None, None, [(12, 10), (300, 16), (306, 400), (8, 396)]]


def _with_orientation(buf: bytes, k: int) -> bytes:
    tiff = b"II*\0" + struct.pack("<IH", 8, 1) + struct.pack("<HHIHH", 0x0112, 3, 1, k, 0) + struct.pack("<I", 0)
    seg = b"Exif\0\0" + tiff
    return buf[:2] + b"\xff\xe1" + struct.pack(">H", len(seg) + 2) + seg + buf[2:]


def _pp():
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    return DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)   # pipeline2.py:213-216 defaults


class _Set:
    def __init__(self):
        from ocr_vi_invoice_amd import pipeline
        from ocr_vi_invoice_amd.engine import plan_rectified
        self.files = [Z["j_" + n].tobytes() for n in FILES]
        self.files[2] = _with_orientation(self.files[2], 6)
        self.arrays = pipeline.imdecode(self.files)
        sizes = [tuple(a.shape[:2]) for a in self.arrays]
        assert sizes == [(500, 380), (420, 320), (420, 320)]
        _, _, shapes, _, _ = plan_rectified(sizes, QUADS, DET_SIZE)
        self.kern = []
        for (H, W) in shapes:
            k = np.zeros((1, H, W), np.float32)
            for j in range((H - 30) // 40):
                k[0, 20 + 40 * j:32 + 40 * j, W // 8 + 3 * j:W - W // 8] = 0.75
            self.kern.append(torch.from_numpy(k).cuda())

    def hook(self, prob, idx):
        torch.add(torch.stack([self.kern[i] for i in idx]), prob, alpha=0.25, out=prob)


@pytest.fixture(scope="module")
def data():
    return _Set()


_CACHE = {}


def _models():
    from ocr_vi_invoice_amd import DBNetPP, SVTRv2, weights
    if "m" not in _CACHE:
        _CACHE["m"] = (DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype="f16x2"),
                       SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype="f16x2"))
    return _CACHE["m"]


def _engine(data, **kw):
    from ocr_vi_invoice_amd import Engine
    det, rec = _models()
    args = dict(det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=data.hook)
    args.update(kw)
    return Engine(det, rec, _pp(), **args)


def _want(data):
    """Engine.run on the decoded arrays, once."""
    if "want" not in _CACHE:
        _CACHE["want"] = _engine(data).run(data.arrays, QUADS)
        assert all(len(w[0]) >= 3 for w in _CACHE["want"])
    return _CACHE["want"]


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, ((gb, gs, gt), (wb, ws, wt)) in enumerate(zip(got, want)):
        assert len(gb) == len(wb), (i, len(gb), len(wb))
        for a, b in zip(gb, wb):
            assert a.dtype == b.dtype and np.array_equal(a, b), i
        assert gs == ws, i
        assert gt == wt, i


def test_engine_on_jpeg_bytes_equals_engine_on_decoded_arrays(data):
    want = _want(data)
    eng = _engine(data)
    _assert_same(eng.run(data.files, QUADS), want)
    assert eng.stats["jpeg"] == 3 and eng.stats["rectified"] == 1
    assert 0 < eng.stats["jpeg_stream_bytes"] < sum(3 * a.shape[0] * a.shape[1] for a in data.arrays)      # less than raw RGB over the bus
    _assert_same(eng.run(data.files, QUADS), want)              # the captured graphs again, streams and tables rewritten


def test_mixed_arrays_and_files_with_and_without_graphs(data):
    want = _want(data)
    mixed = [data.arrays[0].cpu().numpy(), bytearray(data.files[1]), memoryview(data.files[2])]
    _assert_same(_engine(data).run(mixed, QUADS), want)
    _assert_same(_engine(data).run([data.files[0], data.arrays[1], data.files[2]], QUADS), want)
    _assert_same(_engine(data, graphs=False).run(data.files, QUADS), want)
    _assert_same(_engine(data, det_chunk=1).run(data.files, QUADS), want)


def test_enhanced_jpeg_page(data):
    enh = [False, True, False]
    _assert_same(_engine(data).run(data.files, QUADS, enh), _engine(data).run(data.arrays, QUADS, enh))


def test_corrupt_file_raises_naming_its_page_and_the_next_run_is_clean(data):
    want = _want(data)
    eng = _engine(data)
    bad = data.files[1][:len(data.files[1]) // 2]               # a header that parses, a scan that ends early
    with pytest.raises(ValueError, match="page 1"):
        eng.run([data.files[0], bad, data.files[2]], QUADS)
    with pytest.raises(ValueError, match="page 1.*progressive"):
        eng.run([data.files[0], Z["j_progressive_33x17"].tobytes(), data.files[2]], QUADS)
    with pytest.raises(ValueError, match="page 2"):
        eng.run([data.files[0], data.files[1], b"\xff\xd8\xff"], QUADS)
    _assert_same(eng.run(data.files, QUADS), want)
