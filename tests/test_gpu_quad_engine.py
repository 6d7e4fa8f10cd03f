"""Engine(crop="quad") (ocr_vi_invoice_amd/engine.py) against the per-page call it batches, pipeline.detect_and_recognize(crop="quad"):
the same boxes, scores and strings whatever the batching knobs, with crop="rect" unchanged.  The detector's map gets rotated rectangles
painted into it, so the boxes are tilted text lines: the case the oriented crop exists for."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DET_SIZE = 320
SIZES = [(1000, 760), (760, 1000), (1000, 760), (760, 1000)]      # four pages of two sizes
SEEDS = [31, 32, 33, 34]
# page 3 is rectified first (its document's corners) and enhanced
QUADS = [None, None, None, [(40, 30), (960, 50), (940, 720), (30, 700)]]
ENHANCE = [False, False, False, True]
ANGLES = [5, -5, 12, -12]


def _pp():
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor
    return DBPostProcessor(thresh=0.3, box_thresh=0.5, max_candidates=1000, unclip_ratio=1.6)   # pipeline2.py:213-216 defaults


class _Set:
    """The pages and, per page, a map of rotated rectangles at its detector shape (random weights give a map without text structure: the
    blend is kernel + 0.25 binary, as bench.py's)."""

    def __init__(self):
        from ocr_vi_invoice_amd import synth
        from ocr_vi_invoice_amd.engine import plan_rectified
        self.pages = [synth.make_invoice(seed, h, w, lines=10)[0] for (h, w), seed in zip(SIZES, SEEDS)]
        _, _, shapes, _, _ = plan_rectified(SIZES, QUADS, DET_SIZE)
        self.kern = []
        for p, (H, W) in enumerate(shapes):
            k = np.zeros((1, H, W), np.float32)
            yy, xx = np.mgrid[0:H, 0:W]
            rows = (H - 40) // 48
            for j in range(rows):
                a = math.radians(ANGLES[(j + p) % 4])
                u, v = (math.cos(a), math.sin(a)), (-math.sin(a), math.cos(a))
                dx, dy = xx - W / 2, yy - (34 + 48 * j)
                inside = (np.abs(dx * u[0] + dy * u[1]) <= 0.27 * W) & (np.abs(dx * v[0] + dy * v[1]) <= 5)
                k[0][inside] = 0.75
            self.kern.append(torch.from_numpy(k).cuda())

    def hook(self, prob, idx):
        torch.add(torch.stack([self.kern[i] for i in idx]), prob, alpha=0.25, out=prob)


class _BlendedDet:
    """detect_and_recognize's detector for page `page`: the library detector, its binary map blended exactly as the engine's hook does."""

    def __init__(self, det, data):
        self.det, self.data, self.page = det, data, 0

    def __call__(self, x):
        out = self.det(x)
        return {"binary": torch.add(self.data.kern[self.page][None], out["binary"], alpha=0.25)}


@pytest.fixture(scope="module")
def data():
    return _Set()


_CACHE = {}


def _reference(data, dtype, crop):
    """(det, rec, per-page results): computed once per (dtype, crop), shared by the tests."""
    from ocr_vi_invoice_amd import DBNetPP, SVTRv2, pipeline, weights
    if ("models", dtype) not in _CACHE:
        _CACHE[("models", dtype)] = (DBNetPP(pretrained=False, state_dict=weights.make_det_state_dict(seed=21), dtype=dtype),
                                     SVTRv2("tiny", state_dict=weights.make_rec_state_dict("tiny", seed=22), dtype=dtype))
    det, rec = _CACHE[("models", dtype)]
    if (dtype, crop) not in _CACHE:
        wrap, want = _BlendedDet(det, data), []
        for i, p in enumerate(data.pages):
            wrap.page = i
            kw = {} if crop is None else {"crop": crop}      # None: the call as it was before the option existed
            want.append(pipeline.detect_and_recognize(p, wrap, rec, _pp(), "cuda:0", det_size=DET_SIZE, rec_size=(32, 256), rec_batch_size=64,
                                                      quad=QUADS[i], enhance=ENHANCE[i], **kw))
        _CACHE[(dtype, crop)] = want
    return det, rec, _CACHE[(dtype, crop)]


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, ((gb, gs, gt), (wb, ws, wt)) in enumerate(zip(got, want)):
        assert len(gb) == len(wb), (i, len(gb), len(wb))
        for a, b in zip(gb, wb):
            assert a.dtype == b.dtype and np.array_equal(a, b), i
        assert gs == ws, i
        assert gt == wt, i


def _engine(det, rec, data, **kw):
    from ocr_vi_invoice_amd import Engine
    args = dict(det_size=DET_SIZE, rec_size=(32, 256), det_chunk=4, rec_batch=16, prob_hook=data.hook)
    args.update(kw)
    return Engine(det, rec, _pp(), **args)


@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_quad_engine_equals_detect_and_recognize_per_page(data, dtype):
    det, rec, want = _reference(data, dtype, "quad")
    assert all(len(w[0]) >= 3 for w in want) and sum(len(w[0]) for w in want) > 16      # more than one recogniser batch of 16
    eng = _engine(det, rec, data, crop="quad")
    _assert_same(eng.run(data.pages, QUADS, ENHANCE), want)
    assert eng.stats["rectified"] == 1 and eng.stats["enhanced"] == 1 and eng.stats["rec_batches"] >= 2
    _assert_same(eng.run(data.pages, QUADS, ENHANCE), want)                             # the captured graphs, descriptors rewritten


@pytest.mark.parametrize("knob", [dict(graphs=False), dict(rec_batch=64), dict(det_chunk=1)], ids=["eager", "rec_batch_64", "det_chunk_1"])
def test_quad_engine_results_do_not_depend_on_its_batching(data, knob):
    det, rec, want = _reference(data, "f16x2", "quad")
    _assert_same(_engine(det, rec, data, crop="quad", **knob).run(data.pages, QUADS, ENHANCE), want)


def test_rect_mode_is_unchanged_and_quad_mode_is_not_a_no_op(data):
    from ocr_vi_invoice_amd import Engine
    det, rec, today = _reference(data, "f16x2", None)
    _, _, rect = _reference(data, "f16x2", "rect")
    _, _, quad = _reference(data, "f16x2", "quad")
    _assert_same(rect, today)
    _assert_same(_engine(det, rec, data, crop="rect").run(data.pages, QUADS, ENHANCE), today)
    _assert_same(_engine(det, rec, data).run(data.pages, QUADS, ENHANCE), today)        # the default
    # boxes and scores are the same in both modes, only what the recogniser sees changes
    for (qb, qs, qt), (rb, rs, rt) in zip(quad, rect):
        assert qs == rs and len(qb) == len(rb) and all(np.array_equal(a, b) for a, b in zip(qb, rb))
    assert sum(a != b for (_, _, qt), (_, _, rt) in zip(quad, rect) for a, b in zip(qt, rt)) >= 1
    with pytest.raises(ValueError, match="crop"):
        Engine(det, rec, _pp(), det_size=DET_SIZE, crop="diag")


def test_painted_boxes_are_tilted(data):
    """The descriptors of the painted lines are real rotations (not the fallback), wider than tall."""
    from ocr_vi_invoice_amd import pipeline
    _, _, want = _reference(data, "f16x2", "quad")
    tilted = 0
    for (boxes, _, _), (h, w) in zip(want[:3], SIZES[:3]):
        crops, mats = pipeline.quad_crops(boxes, (h, w))
        for c, m in zip(crops, mats):
            if abs(m[1]) > 0.05 and c[1] > 2 * c[2]:
                tilted += 1
    assert tilted >= 8
