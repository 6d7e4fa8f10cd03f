"""Engine.run on PNG bytes (ocr_vi_invoice_amd/engine.py) against Engine.run on the arrays pipeline.imdecode returns for the same files:
the same boxes, scores and strings, alone, mixed with JPEG and array pages in one call, with a quad and with enhance; and the other doors
PNG bytes come in through, detect_and_recognize and DetectionDataset.  The files are synthetic invoices of tests/golden/png_cases.npz
(an RGB one and a bilevel one) and of jpeg_cases.npz; random weights give a map without text structure, so bars are blended into it as
tests/test_gpu_engine.py does (kernel + 0.25 binary)."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DET_SIZE = 320
HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "png_cases.npz"))
J = np.load(os.path.join(HERE, "golden", "jpeg_cases.npz"))
# pages: a PNG RGB invoice 420 x 320, a PNG bilevel one 320 x 420 (rectified), a JPEG one 500 x 380 and an array 300 x 260
QUADS = [None, [(10, 12), (400, 16), (406, 300), (8, 296)], None, None]


def _pp():
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    return DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)   # pipeline2.py:213-216 defaults


class _Set:
    def __init__(self):
        from ocr_vi_invoice_amd import pipeline, synth
        from ocr_vi_invoice_amd.engine import plan_rectified
        self.files = [Z["f_inv1_420x320"].tobytes(), Z["f_inv2_320x420"].tobytes(), J["j_page_500x380"].tobytes()]
        self.extra = synth.make_invoice(11, 300, 260, lines=7)[0]                  # a page that is an array in every run
        self.arrays = pipeline.imdecode(self.files) + [torch.from_numpy(self.extra).cuda()]
        self.pages = self.files + [self.extra]
        sizes = [tuple(a.shape[:2]) for a in self.arrays]
        assert sizes == [(420, 320), (320, 420), (500, 380), (300, 260)]
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


def test_engine_on_png_bytes_equals_engine_on_decoded_arrays(data):
    """Two PNG pages (one rectified), a JPEG page and an array page in one call."""
    from ocr_vi_invoice_amd import pipeline
    want = _want(data)
    eng = _engine(data)
    _assert_same(eng.run(data.pages, QUADS), want)
    assert eng.stats["png"] == 2 and eng.stats["jpeg"] == 1 and eng.stats["rectified"] == 1 and eng.stats["png_parse_s"] > 0
    assert eng.stats["png_stream_bytes"] == sum(pipeline.png_info(f)["stream_bytes"] for f in data.files[:2]) == 420 * (1 + 960) + 320 * (1 + 53)
    _assert_same(eng.run(data.pages, QUADS), want)              # the captured graphs again, streams and tables rewritten


def test_png_pages_alone_and_in_other_containers(data):
    want = _want(data)
    got = _engine(data).run([bytearray(data.files[0]), memoryview(data.files[1])], QUADS[:2])
    _assert_same(got, want[:2])
    _assert_same(_engine(data, graphs=False).run(data.pages, QUADS), want)
    _assert_same(_engine(data, det_chunk=1).run(data.pages, QUADS), want)


def test_enhanced_png_page(data):
    enh = [True, False, False, True]
    _assert_same(_engine(data).run(data.pages, QUADS, enh), _engine(data).run(data.arrays, QUADS, enh))


def test_corrupt_png_raises_naming_its_page_and_the_next_run_is_clean(data):
    want = _want(data)
    eng = _engine(data)
    bad = bytearray(data.files[1])
    bad[len(bad) // 2] ^= 0x20                                  # a header that parses, IDAT data that do not
    with pytest.raises(ValueError, match="page 1.*CRC"):
        eng.run([data.files[0], bytes(bad), data.files[2], data.extra], QUADS)
    assert eng.stats["png"] == 0 and eng.stats["jpeg"] == 0     # nothing was launched
    with pytest.raises(ValueError, match="page 3.*truncated"):
        eng.run([data.files[0], data.files[1], data.files[2], data.files[0][:200]], QUADS)
    _assert_same(eng.run(data.pages, QUADS), want)


def test_detect_and_recognize_takes_png_bytes(data):
    from ocr_vi_invoice_amd import pipeline
    det, rec = _models()
    a = pipeline.detect_and_recognize(data.files[0], det, rec, _pp(), det_size=DET_SIZE)
    b = pipeline.detect_and_recognize(data.arrays[0], det, rec, _pp(), det_size=DET_SIZE)
    assert len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1] and a[2] == b[2]
    pages = pipeline.detect_and_recognize_pages(data.files[:2], det, rec, _pp(), det_size=DET_SIZE)
    arrays = pipeline.detect_and_recognize_pages(data.arrays[:2], det, rec, _pp(), det_size=DET_SIZE)
    _assert_same(pages, arrays)


def test_detection_dataset_reads_a_png_file(tmp_path):
    from ocr_vi_invoice_amd import data as D
    name = "pil_RGBA_std"                                       # 45 x 52
    polys = [[[5, 5], [40, 6], [38, 30], [6, 28]], [[10, 32], [45, 33], [44, 42], [11, 41]]]
    ann = {"annotations": [{"polygon": p, "text": "x"} for p in polys]}
    (tmp_path / "a.json").write_text(json.dumps(ann))
    (tmp_path / "a.png").write_bytes(Z["f_" + name].tobytes())
    keys = ("image", "gt", "mask", "thresh_map", "thresh_mask")
    ds = D.DetectionDataset(str(tmp_path), image_size=64, thresh_maps=True)
    a = next(ds.batches(1))
    b = next(D.DetectionDataset(samples=[(Z["p_" + name], polys)], image_size=64, thresh_maps=True).batches(1))
    c = next(D.DetectionDataset(samples=[(Z["f_" + name].tobytes(), polys)], image_size=64, thresh_maps=True).batches(1))
    assert ds.blank == [] and a["image"].abs().sum() > 0
    assert all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) for k in keys)
    # a PNG the library refuses, and one it finds corrupt while inflating, raise naming the file and are not blanked
    for sub, payload, word in (("interlaced", bytearray(Z["f_" + name].tobytes()), "Adam7"), ("corrupt", bytearray(Z["f_" + name].tobytes()), "CRC")):
        d = tmp_path / sub
        d.mkdir()
        if sub == "interlaced":                                  # IHDR's interlace byte, and its CRC put right again
            payload[28] = 1
            payload[29:33] = zlib.crc32(bytes(payload[12:29])).to_bytes(4, "big")
        else:
            payload[len(payload) // 2] ^= 1
        (d / "e.json").write_text(json.dumps(ann))
        (d / "e.png").write_bytes(bytes(payload))
        bad = D.DetectionDataset(str(d), image_size=64)
        with pytest.raises(ValueError, match=f"e.png.*{word}"):
            bad[0]
        assert bad.blank == []
