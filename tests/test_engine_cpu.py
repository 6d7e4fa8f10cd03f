"""CPU side of the batched engine (ocr_vi_invoice_amd/engine.py): the bucket plan against the reference's own arithmetic
(pipeline2.py:33-40), and the per-page box stage ocrvi_db_boxes_pages against the per-page chain it replaces."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def _ref_shape(h, w, image_size):
    """resize_image_for_det's expression, literally (pipeline2.py:35-39)."""
    scale = image_size / max(h, w)
    new_h = int(np.round(h * scale / 32) * 32)
    new_w = int(np.round(w * scale / 32) * 32)
    return (new_h, new_w), (new_h / h, new_w / w)


def test_plan_buckets_matches_the_reference_expression():
    from ocr_vi_invoice_amd.engine import plan_buckets
    sides = [33, 90, 320, 333, 640, 700, 760, 900, 960, 1000, 1001, 1280, 1754, 2480, 3508]
    sizes = [(h, w) for h in sides for w in sides]
    for det_size in (320, 640, 960, 1280):
        ok = [(h, w) for h, w in sizes if min(_ref_shape(h, w, det_size)[0]) > 0]
        shapes, scales, buckets = plan_buckets(ok, det_size)
        for (h, w), s, sc in zip(ok, shapes, scales):
            want_s, want_sc = _ref_shape(h, w, det_size)
            assert s == want_s and sc == want_sc, (h, w, det_size)
        assert sorted(i for v in buckets.values() for i in v) == list(range(len(ok)))
        for shape, idx in buckets.items():
            assert idx == sorted(idx) and all(shapes[i] == shape for i in idx)
    # half-way ties round to even, as np.round does: a 960x1280 (h x w) page at det_size 960 -> 704 x 960, not 736 x 960
    shapes, _, _ = plan_buckets([(960, 1280), (1280, 960)], 960)
    assert shapes == [(704, 960), (960, 704)]
    # two originals of different sizes share a bucket
    shapes, scales, buckets = plan_buckets([(1000, 760), (900, 700)], 320)
    assert shapes == [(320, 256), (320, 256)] and scales[0] != scales[1] and buckets == {(320, 256): [0, 1]}


def test_plan_buckets_rejects_sides_that_round_to_zero():
    from ocr_vi_invoice_amd.engine import plan_buckets
    with pytest.raises(ValueError, match="page 1"):
        plan_buckets([(640, 640), (2000, 90)], 320)      # 90 * 320 / 2000 / 32 = 0.45 -> 0 (cv2.resize raises in the reference)
    with pytest.raises(ValueError, match="page 0"):
        plan_buckets([(0, 100)], 320)
    assert plan_buckets([], 960) == ([], [], {})


def _maps(n, H, W, seed=3, empty=(2,)):
    from ocr_vi_invoice_amd import synth
    rng = np.random.default_rng(seed)
    maps = []
    for i in range(n):
        pm = rng.uniform(0, 0.25, (H, W)).astype(np.float32)
        if i not in empty:
            _, bx = synth.make_invoice(i + seed, H, W, 6)
            for x, y, w, h in bx:
                pm[y + 1:y + h - 1, x + 2:x + w - 2] = rng.uniform(0.6, 0.95)
        maps.append(pm)
    return np.stack(maps)


def test_db_boxes_pages_equals_the_per_page_chain():
    """Page by page: DBPostProcessor -> rescale_boxes with the page's own scale -> crop_rect in the page's own size."""
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor, crop_rect, db_boxes_pages, rescale_boxes
    H, W = 192, 320
    maps = _maps(5, H, W)
    pp = DBPostProcessor(0.3, 0.5, 1000, 1.6)
    scales = [(H / 230, W / 400), (H / 190, W / 321), (0.5, 0.25), (H / 700, W / 1100), (1.0, 1.0)]
    sizes = [(230, 400), (190, 321), (384, 1280), (700, 1100), (H, W)]
    ids = [7, 3, 11, 0, 5]
    for threads in (1, 4):
        res = db_boxes_pages(maps, pp, scales, sizes, ids, threads=threads)
        assert len(res) == 5 and len(res[2][0]) == 0
        for p in range(5):
            b, sc = pp(maps[p][None])
            want = rescale_boxes(b, scales[p][1], scales[p][0])
            polys, rects, scores = res[p]
            assert len(polys) == len(want) and (p == 2 or len(want) > 0)
            for got, w in zip(polys, want):
                assert got.dtype == np.int32 and np.array_equal(got, w)
            assert np.array_equal(rects, np.asarray([(ids[p],) + crop_rect(sizes[p], w) for w in want], np.int32).reshape(-1, 5))
            assert [float(v) for v in scores] == sc


def test_db_boxes_pages_reports_and_redoes_pages_out_of_point_room():
    from ocr_vi_invoice_amd import _lib
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor, db_boxes_pages
    H, W = 192, 320
    maps = _maps(3, H, W, seed=5, empty=())
    pp = DBPostProcessor(0.3, 0.5, 1000, 1.6)
    scales, sizes = [(0.75, 0.8)] * 3, [(256, 400)] * 3
    full = db_boxes_pages(maps, pp, scales, sizes, threads=2)
    need = [sum(len(q) for q in r[0]) for r in full]
    assert min(need) > 8
    # the raw entry: a page past the room reports the points it needs, its rects / counts are still written
    cap, cb = 8, 1000
    pts = np.empty((3, cap, 2), np.int32)
    offs, rects = np.empty((3, cb + 1), np.int32), np.empty((3, cb, 5), np.int32)
    scores, counts, over = np.empty((3, cb), np.float32), np.empty(3, np.int32), np.empty(3, np.int32)
    sh, sw = np.full(3, 0.75), np.full(3, 0.8)
    oh, ow, ids = np.full(3, 256, np.int32), np.full(3, 400, np.int32), np.arange(3, dtype=np.int32)
    _lib.check(_lib.load().ocrvi_db_boxes_pages(maps.ctypes.data, 3, H, W, 0.3, 0.5, 1000, 1.6, 10.0, sw.ctypes.data, sh.ctypes.data,
                                                oh.ctypes.data, ow.ctypes.data, ids.ctypes.data, pts.ctypes.data, cap, offs.ctypes.data,
                                                rects.ctypes.data, scores.ctypes.data, cb, counts.ctypes.data, over.ctypes.data, 2))
    assert over.tolist() == need
    assert counts.tolist() == [len(r[0]) for r in full]
    for p in range(3):
        assert np.array_equal(rects[p, :counts[p]], full[p][1])
    # the helper redoes such a page alone: the same results as with room to spare
    small = db_boxes_pages(maps, pp, scales, sizes, threads=2, cap_points=8)
    for a, b in zip(small, full):
        assert len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_db_boxes_pages_with_equal_scales_equals_db_boxes_batch_and_threads_agree():
    from ocr_vi_invoice_amd.pipeline import DBPostProcessor, db_boxes_batch, db_boxes_pages
    H, W = 160, 256
    maps = _maps(8, H, W, seed=9, empty=(4,))
    pp = DBPostProcessor(0.3, 0.5, 1000, 1.6)
    rects, counts, scores = db_boxes_batch(maps, pp, 0.8, 1.25, (150, 411), page_base=10, threads=4)
    one = db_boxes_pages(maps, pp, [(1.25, 0.8)] * 8, [(150, 411)] * 8, list(range(10, 18)), threads=1)
    eight = db_boxes_pages(maps, pp, [(1.25, 0.8)] * 8, [(150, 411)] * 8, list(range(10, 18)), threads=8)
    assert [len(r[0]) for r in one] == counts.tolist()
    assert np.array_equal(np.concatenate([r[1] for r in one], 0), rects)
    assert np.array_equal(np.concatenate([r[2] for r in one], 0), scores)
    for a, b in zip(one, eight):
        assert len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
