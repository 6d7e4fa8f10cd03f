"""Oriented text crops, host half (include/ocrvi.h, "Oriented text crops"): ocrvi_min_area_quads and ocrvi_quad_crops against the Python
statement in tests/quad_ref.py (integers and fractions), hand-derived known answers, and the reference chain of the device entry.  No GPU."""
import math

import numpy as np
import pytest

import quad_ref as QR
import warp_ref as WR
from oracle import preproc_cpu

PAGE_HW = (2000, 3000)


def _lib_quads(polys):
    from ocr_vi_invoice_amd import pipeline
    return pipeline.min_area_quads(polys)


def _lib_descriptors(quads, flags, page_hw=PAGE_HW, page_id=0):
    """The raw C entry on given quads -> (crops int32 [n,4], m_inv float64 [n,9])."""
    from ocr_vi_invoice_amd import _lib
    quads = np.ascontiguousarray(quads, np.float64).reshape(-1, 4, 2)
    n = len(quads)
    flags = np.ascontiguousarray(flags, np.int32)
    ids = np.full(n, page_id, np.int32)
    hw = np.ascontiguousarray(np.broadcast_to(np.asarray(page_hw, np.int32), (n, 2)))
    crops, m = np.full((n, 4), -7, np.int32), np.full((n, 9), np.nan)
    _lib.check(_lib.load().ocrvi_quad_crops(quads.ctypes.data, flags.ctypes.data, n, ids.ctypes.data, hw.ctypes.data, crops.ctypes.data, m.ctypes.data))
    return crops, m


def _is_translation(m):
    return m[0] == 1 and m[1] == 0 and m[3] == 0 and m[4] == 1 and m[6] == 0 and m[7] == 0 and m[8] == 1


# ---------------------------------------------------------------------------------------------------- known answers, derived by hand
# (polygon, quad in the stated corner order, flag).  Hull vertex 0 is the smallest (x, y); edge 0 leaves it counter-clockwise (y up).
KATS = {
    # every edge of a rectangle gives the rectangle itself: a four-way tie, edge 0 = (0,0) -> (10,0) wins; d = (10, 0), s = 10 x in
    # [0, 100], t = 10 y in [0, 40], area 4000 / 100 = 40
    "axis_rectangle": ([(0, 0), (10, 0), (10, 4), (0, 4)], [(0, 0), (10, 0), (10, 4), (0, 4)], 0),
    # the 3-4-5 rectangle with sides 50 and 10: hull (-6,8) (0,0) (40,30) (34,38); edge 0 has d = (6, -8), |d|^2 = 100, s = 6x - 8y in
    # [-100, 0], t = 8x + 6y in [0, 500], area 100 * 500 / 100 = 500 = 50 * 10; corners (s dx - t dy, s dy + t dx) / 100
    "rect_3_4_5": ([(0, 0), (40, 30), (34, 38), (-6, 8)], [(-6, 8), (0, 0), (40, 30), (34, 38)], 0),
    # a triangle: every edge's rectangle has twice the triangle's area (base * height), so all three tie and edge 0 wins.  Hull (-3,4)
    # (0,0) (8,6), d = (3, -4), s = 3x - 4y in [-25, 0], t = 4x + 3y in [0, 50], area 25 * 50 / 25 = 50; the fourth corner is (-25, 50)
    # -> ((-75 + 200) / 25, (100 + 150) / 25) = (5, 10)
    "triangle": ([(0, 0), (8, 6), (-3, 4)], [(-3, 4), (0, 0), (8, 6), (5, 10)], 0),
    # a tilted square, side (3, 4): four-way tie, the first hull edge (-4,3) -> (0,0) wins and fixes the corner order
    "square_tie": ([(3, 4), (-1, 7), (0, 0), (-4, 3)], [(-4, 3), (0, 0), (3, 4), (-1, 7)], 0),
    # interior, duplicate and collinear points do not matter: the rectangle 12 x 6 with a point on an edge, one inside, one repeated
    "extra_points": ([(0, 0), (6, 0), (12, 0), (12, 6), (5, 3), (0, 6), (12, 6)], [(0, 0), (12, 0), (12, 6), (0, 6)], 0),
    "collinear": ([(0, 0), (2, 2), (5, 5)], [(0, 0), (5, 0), (5, 5), (0, 5)], 1),
    "collinear_axis": ([(4, 1), (9, 1), (-2, 1), (9, 1)], [(-2, 1), (9, 1), (9, 1), (-2, 1)], 1),
    "single_point": ([(7, -3)], [(7, -3)] * 4, 1),
    "two_points": ([(7, -3), (1, 5)], [(1, -3), (7, -3), (7, 5), (1, 5)], 1),
}


@pytest.mark.parametrize("name", sorted(KATS))
def test_known_answers(name):
    poly, quad, flag = KATS[name]
    want = np.array(quad, np.float64)
    ref_q, ref_f = QR.min_area_quad(poly)
    assert ref_f == flag and ref_q.tobytes() == want.tobytes(), (ref_q, ref_f)
    q, f = _lib_quads([np.array(poly)])
    assert f.tolist() == [flag] and q[0].tobytes() == want.tobytes(), (q, f)


def test_3_4_5_rectangle_orders_to_50_by_10():
    quad = KATS["rect_3_4_5"][1]
    assert WR.output_size(WR.order_points(quad)) == (50, 10)
    (pid, w, h, z), m, refused = QR.quad_crop_descriptor(quad, 0, PAGE_HW, 3)
    assert (pid, w, h, z, refused) == (3, 50, 10, 0, False)
    crops, mats = _lib_descriptors([quad], [0], page_id=3)
    assert crops.tolist() == [[3, 50, 10, 0]] and mats[0].tobytes() == m.tobytes()
    # the matrix maps the crop's corners onto the quad's ordered corners: (0,0) -> (0,0), (49,0) -> (40,30), (49,9) -> (34,38), (0,9) -> (-6,8)
    got = WR.project(mats[0], [(0, 0), (49, 0), (49, 9), (0, 9)])
    assert np.abs(got - [(0, 0), (40, 30), (34, 38), (-6, 8)]).max() < 1e-9


def test_range_is_checked():
    from ocr_vi_invoice_amd import _lib, pipeline
    ok = [np.array([(-32768, -32768), (32767, -32768), (32767, 32767), (-32768, 32767)])]
    q, f = pipeline.min_area_quads(ok)
    assert f.tolist() == [0] and q[0].tolist() == [[-32768, -32768], [32767, -32768], [32767, 32767], [-32768, 32767]]
    for bad in ((32768, 0), (0, -32769)):
        pts = np.array([(0, 0), (5, 0), bad], np.int32)
        offs = np.array([0, 3], np.int32)
        out, fl = np.zeros(8), np.zeros(1, np.int32)
        assert _lib.load().ocrvi_min_area_quads(pts.ctypes.data, offs.ctypes.data, 1, out.ctypes.data, fl.ctypes.data) == -1
        with pytest.raises(ValueError):
            pipeline.min_area_quads([np.array([(0, 0), (5, 0), bad])])
        with pytest.raises(ValueError):
            QR.min_area_quad([(0, 0), (5, 0), bad])
    q, f = pipeline.min_area_quads([])
    assert q.shape == (0, 4, 2) and f.shape == (0,)


# ---------------------------------------------------------------------------------------------------- C++ against the Python statement
def _random_polygons(n, seed=20260118):
    rng = np.random.default_rng(seed)
    polys = []
    for i in range(n):
        k = int(rng.integers(3, 41))
        kind = i % 8
        if kind == 0:      # a small grid: duplicates, collinear runs, ties
            p = rng.integers(-4, 5, (k, 2))
        elif kind == 1:    # the range limits
            p = rng.choice([-32768, -32767, 0, 32766, 32767], (k, 2))
        elif kind == 2:    # the whole range
            p = rng.integers(-32768, 32768, (k, 2))
        elif kind == 3:    # collinear points (degenerate), sometimes off the page
            a, b = rng.integers(-20, 21, 2), rng.integers(-3000, 3001, 2)
            p = b[None, :] + rng.integers(-40, 41, (k, 1)) * a[None, :]
        elif kind == 4:    # a thin tilted text line with jitter, like a DB polygon
            ang, cx, cy = rng.uniform(-math.pi / 2, math.pi / 2), rng.uniform(100, 2500), rng.uniform(100, 1800)
            u = np.array([math.cos(ang), math.sin(ang)])
            v = np.array([-u[1], u[0]])
            L, T = rng.uniform(30, 400), rng.uniform(4, 30)
            ts = rng.uniform(-1, 1, (k, 2))
            ts[:min(k, 4)] = [(-1, -1), (1, -1), (1, 1), (-1, 1)][:min(k, 4)]
            p = np.rint(np.array([cx, cy]) + ts[:, :1] * L * u + ts[:, 1:] * T * v).astype(np.int64)
        elif kind == 5:    # exactly 45 degrees: the ordering picks one corner twice and the descriptor falls back
            a, w, x0, y0 = int(rng.integers(20, 200)), int(rng.integers(2, 15)), int(rng.integers(-50, 2000)), int(rng.integers(-50, 1500))
            p = np.array([(x0, y0), (x0 + a, y0 + a), (x0 + a - w, y0 + a + w), (x0 - w, y0 + w)])
        else:              # a page-sized cloud, with repeated points
            p = rng.integers(-100, 3200, (k, 2))
            p[k // 2:] = p[:k - k // 2] if kind == 7 else p[k // 2:]
        polys.append(np.asarray(p, np.int64))
    return polys


def test_library_equals_the_python_statement_on_random_polygons():
    from ocr_vi_invoice_amd import pipeline
    polys = _random_polygons(2400)
    quads, flags = pipeline.min_area_quads(polys)
    crops, mats = pipeline.quad_crops(polys, PAGE_HW, page_id=5)
    n_flag = n_refused = 0
    for i, p in enumerate(polys):
        q, f = QR.min_area_quad(p)
        assert f == flags[i] and q.tobytes() == quads[i].tobytes(), (i, p.tolist(), q, quads[i])
        desc, m, refused = QR.quad_crop_descriptor(q, f, PAGE_HW, 5)
        assert list(desc) == crops[i].tolist(), (i, desc, crops[i])
        assert m.tobytes() == mats[i].tobytes(), (i, m, mats[i])
        n_flag += f
        n_refused += refused and not f
        if not refused:        # numpy's solver on the same system is the yardstick of the matrix's accuracy: both map the crop's corners
            rect, dst, w, h, _, np_inv = WR.four_point_geometry(q)          # onto the ordered corners
            assert (w, h) == (desc[1], desc[2])
            scale = max(1.0, np.abs(rect).max())
            assert np.abs(WR.project(m, dst) - rect).max() <= 1e-7 * scale, i
    assert n_flag >= 250 and n_refused >= 250          # both fallbacks are exercised


def test_properties_on_random_polygons():
    polys = _random_polygons(600, seed=7)
    quads, flags = _lib_quads(polys)
    for p, q, f in zip(polys, quads, flags):
        if f:
            continue
        e0, e1 = q[1] - q[0], q[3] - q[0]
        l0, l1 = np.hypot(*e0), np.hypot(*e1)
        assert l0 > 0 and l1 > 0 and abs(e0 @ e1) <= 1e-9 * l0 * l1          # a rectangle
        assert np.abs(q[0] + e0 + e1 - q[2]).max() <= 1e-9 * max(l0, l1)
        d = p.astype(np.float64) - q[0]
        a, b = d @ e0 / l0, d @ e1 / l1                                       # every point inside, within 1e-9 of the side lengths
        assert a.min() >= -1e-9 * l0 and a.max() <= l0 * (1 + 1e-9) and b.min() >= -1e-9 * l1 and b.max() <= l1 * (1 + 1e-9)
        bbox = float(p[:, 0].max() - p[:, 0].min()) * float(p[:, 1].max() - p[:, 1].min())
        assert l0 * l1 <= bbox * (1 + 1e-12)


# ---------------------------------------------------------------------------------------------------- descriptors
def _tilted(deg, cx=400.0, cy=300.0, L=200.0, T=20.0):
    a = math.radians(deg)
    u, v = np.array([math.cos(a), math.sin(a)]), np.array([-math.sin(a), math.cos(a)])
    c = np.array([cx, cy])
    return np.array([c - u * L / 2 - v * T / 2, c + u * L / 2 - v * T / 2, c + u * L / 2 + v * T / 2, c - u * L / 2 + v * T / 2])


def test_tilt_sweep_keeps_the_line_horizontal():
    degs = list(range(-44, 45))
    quads = np.stack([_tilted(d) for d in degs])
    crops, mats = _lib_descriptors(quads, np.zeros(len(degs), np.int32))
    for d, q, c, m in zip(degs, quads, crops, mats):
        desc, rm, refused = QR.quad_crop_descriptor(q, 0, PAGE_HW)
        assert not refused and list(desc) == c.tolist() and rm.tobytes() == m.tobytes(), d
        assert c[1] > c[2] and 198 <= c[1] <= 200 and 18 <= c[2] <= 20, (d, c)
        assert not _is_translation(m) or d == 0
        # the crop's top-left pixel is the quad's top-left corner, its first row runs along the long side
        assert np.abs(WR.project(m, [(0, 0)])[0] - q[0]).max() < 1e-3, d
    # exactly 45 degrees on integer corners: the ordering picks (0, 0) twice, the geometry refuses, the descriptor is the rectangle crop
    q45 = np.array([(100, 50), (240, 190), (230, 200), (90, 60)], np.float64)
    assert WR.order_points(q45).tolist()[0] == WR.order_points(q45).tolist()[1]
    crops, mats = _lib_descriptors([q45], [0])
    desc, rm, refused = QR.quad_crop_descriptor(q45, 0, PAGE_HW)
    assert refused and crops[0].tolist() == list(desc) == [0, 151, 151, 0]
    from ocr_vi_invoice_amd import _lib
    assert _lib.last_error() == ""          # the refusal is control flow: the successful call leaves no stale message behind
    assert mats[0].tolist() == rm.tolist() == [1, 0, 90, 0, 1, 50, 0, 0, 1]


def test_fallback_is_crop_rect():
    """A flagged polygon and a refused quad get crop_rect's rectangle (src/det/test.py:123-130) under a translation; empty -> w = h = 0."""
    from ocr_vi_invoice_amd import pipeline
    hw = (100, 120)
    polys = [np.array([(5, 7), (30, 7), (60, 7)]),          # collinear, inside
             np.array([(-9, 20), (-9, 40)]),                # overhangs the left edge: x -> 0, the width is not reduced by the shift
             np.array([(110, 90), (130, 110)]),             # overhangs right and bottom
             np.array([(200, 300)]),                        # outside: empty
             np.array([(-30, -30), (-20, -30)])]            # outside, above left: clamps to (0, 0), bw = 11 (crop_image's arithmetic)
    crops, mats = pipeline.quad_crops(polys, hw, page_id=2)
    for p, c, m in zip(polys, crops, mats):
        x, y, bw, bh = pipeline.crop_rect(hw, p)
        if bw == 0 or bh == 0:
            bw = bh = 0
        assert c.tolist() == [2, bw, bh, 0], (p.tolist(), c)
        assert m.tolist() == [1, 0, x, 0, 1, y, 0, 0, 1]
    assert crops[3].tolist() == [2, 0, 0, 0]
    # shorter than a pixel: h = int(0.7) = 0 is refused -> the bounding rectangle of the corners
    thin = np.array([(10, 10), (50, 10), (50, 10.7), (10, 10.7)])
    c, m = _lib_descriptors([thin], [0], hw)
    assert c[0].tolist() == [0, 41, 2, 0] and m[0].tolist() == [1, 0, 10, 0, 1, 10, 0, 0, 1]
    desc, rm, refused = QR.quad_crop_descriptor(thin, 0, hw)
    assert refused and list(desc) == [0, 41, 2, 0] and rm.tolist() == m[0].tolist()


def test_translation_descriptor_is_the_rectangle_crop():
    """Under the warp definition an integer translation reads the page unchanged, so the oriented chain on a translation descriptor is the
    reference chain on the rectangle: crop_quad_preprocess == oracle.preproc_cpu on the slice.  (A self-check of tests/quad_ref.py, the
    yardstick of the device tests: it runs no library code.)"""
    rng = np.random.default_rng(3)
    page = rng.integers(0, 256, (90, 140, 3), dtype=np.uint8)
    for (x, y, w, h), size in (((7, 11, 100, 17), (32, 256)), ((0, 0, 140, 90), (32, 256)), ((30, 40, 20, 40), (32, 64)), ((5, 5, 128, 64), (32, 64)),
                               ((139, 89, 1, 1), (48, 320))):
        m = np.array([1, 0, x, 0, 1, y, 0, 0, 1], np.float64)
        assert np.array_equal(QR.warp_replicate(page, m, h, w), page[y:y + h, x:x + w])
        got = QR.crop_quad_preprocess(page, (0, w, h, 0), m, size)
        want = preproc_cpu.preprocess_for_recognition(preproc_cpu.crop_image(page, (x, y, w, h)), size)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert not QR.crop_quad_preprocess(page, (0, 0, 5, 0), np.eye(3).reshape(9)).any()
    # replicate border: a crop that overhangs the left edge repeats column 0 instead of reading zeros
    m = np.array([1, 0, -3, 0, 1, 2, 0, 0, 1], np.float64)
    got = QR.warp_replicate(page, m, 4, 6)
    assert np.array_equal(got[:, :4], np.repeat(page[2:6, :1], 4, axis=1)) and np.array_equal(got[:, 3:], page[2:6, :3])
    assert not np.array_equal(WR.warp_perspective(page, m, 4, 6), got)


# ---------------------------------------------------------------------------------------------------- the public surface
def test_crop_option_is_validated():
    from ocr_vi_invoice_amd import pipeline
    page = np.zeros((64, 64, 3), np.uint8)
    for fn in (pipeline.detect_and_recognize, ):
        with pytest.raises(ValueError, match="crop"):
            fn(page, None, None, pipeline.DBPostProcessor(), crop="diag")
    with pytest.raises(ValueError, match="crop"):
        pipeline.detect_and_recognize_pages([page], None, None, pipeline.DBPostProcessor(), crop="diag")
    import inspect
    from ocr_vi_invoice_amd import engine
    for fn in (pipeline.detect_and_recognize, pipeline.detect_and_recognize_pages, engine.Engine.__init__):
        assert inspect.signature(fn).parameters["crop"].default == "rect"


def test_exports_and_abi_version():
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    for name in ("ocrvi_min_area_quads", "ocrvi_quad_crops", "ocrvi_crop_quad_resize_normalize_pages", "ocrvi_crop_quad_resize_normalize"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert _lib.ABI_VERSION == 5 and lib.ocrvi_abi_version() == 5
    from ocr_vi_invoice_amd import pipeline
    for name in ("min_area_quads", "quad_crops", "preprocess_crops_quad"):
        assert callable(getattr(pipeline, name))
