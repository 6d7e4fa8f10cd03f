"""``Engine(confidence=True)`` against the engine without it and against ``pipeline.detect_and_recognize(page, confidence=True)`` for each
page alone, in the setup of tests/test_gpu_engine.py (320-pixel detector side, SVTRv2-tiny, a rendered text kernel blended into the
random-weight map): the same boxes, scores and strings, and per character the same span and the same score, exactly -- the recogniser's
kernels are chosen by shape and not by the batch's row count, so a crop alone computes what it computes inside a batch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DET_SIZE = 320
SIZES = [(1000, 760), (900, 700), (640, 640)]         # three small pages of two detector shapes: 320x256 twice, 320x320
SEEDS = [11, 12, 14]


def _pp():
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    return DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)


class _Set:
    """The pages and, per page, the rendered text kernel at its detector shape (tests/test_gpu_engine.py: kernel + 0.25 binary)."""

    def __init__(self):
        from ocr_vi_invoice_amd import synth
        from ocr_vi_invoice_amd.engine import plan_buckets
        self.pages, self.kern = [], []
        shapes, scales, _ = plan_buckets(SIZES, DET_SIZE)
        for (h, w), seed, (H, W), (sh, sw) in zip(SIZES, SEEDS, shapes, scales):
            img, boxes = synth.make_invoice(seed, h, w, lines=8)
            self.pages.append(img)
            k = np.zeros((1, H, W), np.float32)
            for x, y, bw, bh in boxes:
                x0, x1 = int(x * sw) + 2, int((x + bw) * sw) - 2
                y0, y1 = int(y * sh) + 1, int((y + bh) * sh) - 1
                if x1 - x0 >= 3 and y1 - y0 >= 2:
                    k[0, y0:y1, x0:x1] = 0.75
            self.kern.append(torch.from_numpy(k).cuda())

    def hook(self, prob, idx):
        torch.add(torch.stack([self.kern[i] for i in idx]), prob, alpha=0.25, out=prob)


class _BlendedDet:
    def __init__(self, det, data):
        self.det, self.data, self.page = det, data, 0

    def __call__(self, x):
        return {"binary": torch.add(self.data.kern[self.page][None], self.det(x)["binary"], alpha=0.25)}


@pytest.fixture(scope="module")
def data():
    return _Set()


_CACHE = {}


def _setup(data, dtype):
    """Models, the engine's plain results (the parent's entry point) and the per-page results with confidences, once per mode."""
    if dtype not in _CACHE:
        from ocr_vi_invoice_amd import DBNetPP, Engine, SVTRv2, pipeline, weights
        det = DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype=dtype)
        rec = SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype=dtype)
        plain = Engine(det, rec, _pp(), det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=data.hook).run(data.pages)
        wrap, alone = _BlendedDet(det, data), []
        for i, p in enumerate(data.pages):
            wrap.page = i
            alone.append(pipeline.detect_and_recognize(p, wrap, rec, _pp(), "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), rec_batch_size=64,
                                                       confidence=True))
        _CACHE[dtype] = (det, rec, plain, alone)
    return _CACHE[dtype]


def _assert_same_boxes(got, want):
    for (gb, gs, gt), (wb, ws, wt) in zip(got, want):
        assert len(gb) == len(wb)
        assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(gb, wb))
        assert gs == ws and gt == wt


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_engine_confidence_equals_the_plain_engine_and_the_page_alone(data, dtype):
    from ocr_vi_invoice_amd import Engine
    from ocr_vi_invoice_amd.rec import Recognition
    det, rec, plain, alone = _setup(data, dtype)
    assert sum(len(r[0]) for r in plain) > 10 and all(len(r[0]) > 0 for r in plain)
    eng = Engine(det, rec, _pp(), det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=data.hook, confidence=True)
    got = eng.run(data.pages)
    assert all(len(r) == 4 for r in got) and all(len(r) == 4 for r in alone)
    _assert_same_boxes([r[:3] for r in got], plain)                     # confidence changes no box, score or string
    _assert_same_boxes([r[:3] for r in alone], plain)
    n_chars = 0
    for i, ((_, _, texts, recs), (_, _, _, want)) in enumerate(zip(got, alone)):
        assert len(recs) == len(texts) == len(want)
        for j, (r, w, t) in enumerate(zip(recs, want, texts)):
            assert isinstance(r, Recognition) and r.text == t == w.text, (i, j)
            assert len(r.text) == len(r.char_scores) == len(r.spans)
            assert r.spans == w.spans, (i, j, r.spans, w.spans)
            assert r.char_scores == w.char_scores, (i, j, np.abs(np.log(r.char_scores) - np.log(w.char_scores)).max())
            assert r.score == w.score and r.log_prob is None and w.log_prob is not None and w.log_prob <= 0
            assert all(0 <= t0 <= t1 < 64 for t0, t1 in r.spans) and all(0.0 < s <= 1.0 for s in r.char_scores)
            n_chars += len(r.text)
    assert n_chars > 20
    # a second run replays the captured graph into the same buffers
    again = eng.run(data.pages)
    assert [[tuple(r) for r in pg[3]] for pg in again] == [[tuple(r) for r in pg[3]] for pg in got]


def test_engine_confidence_with_annotate_and_the_one_shot_wrapper(data):
    from ocr_vi_invoice_amd import Engine, pipeline
    det, rec, plain, alone = _setup(data, "f16x2")
    kw = dict(det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=data.hook)
    both = Engine(det, rec, _pp(), annotate=True, confidence=True, **kw).run(data.pages)
    only = Engine(det, rec, _pp(), annotate=True, **kw).run(data.pages)
    assert all(len(r) == 5 for r in both) and all(len(r) == 4 for r in only)
    _assert_same_boxes([r[:3] for r in both], plain)
    for b, o, a, p in zip(both, only, alone, data.pages):
        assert b[3].is_cuda and b[3].dtype == torch.uint8 and tuple(b[3].shape) == p.shape and torch.equal(b[3], o[3])
        assert [tuple(r)[:4] for r in b[4]] == [tuple(r)[:4] for r in a[3]]
    assert Engine(det, rec, _pp(), confidence=True, **kw).run([]) == []
    # the one-shot wrapper and char_boxes on its rectangles, on the plain random-weight detector
    pp = _pp()
    pp.max_candidates = 20
    pages = pipeline.detect_and_recognize_pages(data.pages[2:], det, rec, pp, "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), rec_batch_size=64,
                                                confidence=True)
    one = pipeline.detect_and_recognize(data.pages[2], det, rec, pp, "cuda:0", det_size=DET_SIZE, confidence=True)
    assert len(pages) == 1 and len(pages[0]) == 4
    _assert_same_boxes([pages[0][:3]], [one[:3]])
    assert [tuple(r)[:4] for r in pages[0][3]] == [tuple(r)[:4] for r in one[3]]
    h, w = data.pages[2].shape[:2]
    for box, r in zip(one[0], one[3]):
        rect = pipeline.crop_rect((h, w), box)
        if rect[2] > 0 and rect[3] > 0:
            cb = pipeline.char_boxes(rect, r)
            assert cb.shape == (len(r.text), 4) and (cb[:, 0] >= rect[0]).all() and (cb[:, 0] + cb[:, 2] <= rect[0] + rect[2]).all()
