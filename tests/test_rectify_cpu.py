"""CPU side of the four-point rectification: the numpy reference of the warp (tests/warp_ref.py) on cases whose result is known, the host
geometry ``ocrvi_four_point_transform`` (src/preprocess/scanner.py:13-50) against it, and the engine's bucket plan for rectified pages."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import warp_ref as WR  # noqa: E402

SMALL = [(5.5, 3.2), (48.1, 6.7), (50.3, 33.9), (2.2, 30.1)]
LARGE = [(300.7, 120.2), (2800.4, 410.9), (2650.1, 3900.3), (90.8, 3700.6)]
RECT = [(0, 0), (52, 0), (52, 36), (0, 36)]
DIAMOND = [(10, 0), (20, 10), (10, 20), (0, 10)]
TINY = [(0, 0), (0.5, 0), (0.5, 0.4), (0, 0.4)]              # every side shorter than one pixel
COLLINEAR = [(0, 0), (10, 0), (20, 0), (0, 10)]


def _geom(pts, want_fwd=True):
    """The raw C entry -> (rc, m_fwd [3,3], m_inv [3,3], out_w, out_h)."""
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    q = np.ascontiguousarray(pts, np.float64)
    f, i = np.full(9, np.nan), np.full(9, np.nan)
    w, h = ctypes.c_int32(-7), ctypes.c_int32(-7)
    rc = lib.ocrvi_four_point_transform(q.ctypes.data, f.ctypes.data if want_fwd else None, i.ctypes.data, ctypes.byref(w), ctypes.byref(h))
    return rc, f.reshape(3, 3), i.reshape(3, 3), w.value, h.value


def test_reference_identity_and_translation():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    assert np.array_equal(WR.warp_perspective(img, np.eye(3), 37, 53), img)
    # destination (x, y) reads source (x + 3, y - 2): the image shifted, zero where the source lies outside
    shift = np.array([[1, 0, 3], [0, 1, -2], [0, 0, 1.0]])
    want = np.zeros_like(img)
    want[2:, :50] = img[:35, 3:]
    assert np.array_equal(WR.warp_perspective(img, shift, 37, 53), want)
    # half a pixel to the right: the rounded mean of horizontal neighbours (weights 16384 + 16384), the last column against the border
    half = np.array([[1, 0, 0.5], [0, 1, 0], [0, 0, 1.0]])
    nxt = np.concatenate([img[:, 1:], np.zeros((37, 1, 3), np.uint8)], 1).astype(np.int64)
    assert np.array_equal(WR.warp_perspective(img, half, 37, 53), ((img.astype(np.int64) + nxt) * 16384 + 16384) >> 15)
    # a scaled matrix is the same map
    assert np.array_equal(WR.warp_perspective(img, shift * -2.5, 37, 53), want)


def test_reference_zero_denominator_and_clamp():
    rng = np.random.default_rng(1)
    img = rng.integers(1, 256, (37, 53, 3), dtype=np.uint8)
    # W0 = x - 5 is exactly 0 on column 5: s = 0 there, so that column reads source (0, 0) with weight 32768
    m = np.array([[1, 0, 0], [0, 1, 0], [1, 0, -5.0]])
    X, Y = WR.warp_coords(m, 8, 12)
    assert (X[:, 5] == 0).all() and (Y[:, 5] == 0).all()
    assert np.array_equal(WR.warp_perspective(img, m, 8, 12)[:, 5], np.broadcast_to(img[0, 0], (8, 3)))
    # X0 s beyond int32: the clamp, all four taps outside, zeros
    big = np.array([[1e9, 0, 1e9], [0, 1, 0], [0, 0, 1.0]])
    X, _ = WR.warp_coords(big, 4, 4)
    assert (X == 2147483647).all()
    assert not WR.warp_perspective(img, big, 4, 4).any()
    X, _ = WR.warp_coords(-big, 4, 4)                   # (-big has W0 = -1: the same map)
    assert (X == 2147483647).all()
    neg = np.array([[-1e9, 0, -1e9], [0, 1, 0], [0, 0, 1.0]])
    X, _ = WR.warp_coords(neg, 4, 4)
    assert (X == -2147483648).all() and not WR.warp_perspective(img, neg, 4, 4).any()


@pytest.mark.parametrize("quad,size", [(SMALL, (48, 27)), (LARGE, (2567, 3586)), (RECT, (52, 36))])
def test_geometry_size_and_order(quad, size):
    """out_w / out_h equal the reference's float32 arithmetic, and no permutation of the input changes a single bit of the output."""
    rect, dst, w, h, _, _ = WR.four_point_geometry(quad)
    assert (w, h) == size
    rc, f, i, W, H = _geom(quad)
    assert rc == 0 and (W, H) == (w, h)
    for perm in itertools.permutations(range(4)):
        rc2, f2, i2, W2, H2 = _geom([quad[k] for k in perm])
        assert rc2 == 0 and (W2, H2) == (W, H)
        assert f2.tobytes() == f.tobytes() and i2.tobytes() == i.tobytes(), perm
    # m_fwd is optional; m_inv does not depend on it
    rc3, _, i3, W3, H3 = _geom(quad, want_fwd=False)
    assert rc3 == 0 and i3.tobytes() == i.tobytes() and (W3, H3) == (W, H)
    assert np.array_equal(WR.order_points(quad), WR.order_points(quad[::-1]))


@pytest.mark.parametrize("quad", [SMALL, LARGE])
def test_geometry_matrices(quad):
    """m_fwd maps the ordered corners onto the destination corners, and m_inv . m_fwd (scaled to a unit last element) maps them onto
    themselves.  The yardstick is numpy.linalg.solve on the same 8 x 8 system: the largest distance, in pixels, between its images of the
    four corners and the destination corners.  Measured: 3.6e-15 px on the small quad and 4.5e-13 px on the large one (the system's
    condition number is 3e7 there).  The library eliminates in another order, so it is held to 1000 x numpy's residual on the same quad,
    computed here; it measured 7.1e-15 px and 4.5e-13 px forward, 0 and 1.4e-14 px round trip."""
    rect, dst, w, h, np_fwd, _ = WR.four_point_geometry(quad)
    np_res = np.abs(WR.project(np_fwd, rect) - dst).max()
    assert 0 < np_res < 1e-11
    bound = 1000 * np_res
    rc, f, i, W, H = _geom(quad)
    assert rc == 0 and f[2, 2] == 1.0
    res = np.abs(WR.project(f, rect) - dst).max()
    prod = i @ f
    prod /= prod[2, 2]
    trip = np.abs(WR.project(prod, rect) - rect.astype(np.float64)).max()
    print(f"numpy residual {np_res:.3g} px, library {res:.3g} px, m_inv.m_fwd round trip {trip:.3g} px, bound {bound:.3g} px")
    assert res <= bound
    assert trip <= bound
    # and m_inv maps the destination corners back onto the ordered corners
    assert np.abs(WR.project(i, dst) - rect.astype(np.float64)).max() <= bound


@pytest.mark.parametrize("quad", [DIAMOND, TINY, COLLINEAR], ids=["diamond", "shorter_than_a_pixel", "collinear"])
def test_geometry_refuses_degenerate_quads(quad):
    from ocr_vi_invoice_amd import _lib, pipeline
    if quad is DIAMOND:      # the ordering picks (10, 0) twice
        assert WR.order_points(quad).tolist() == [[10, 0], [10, 0], [20, 10], [10, 20]]
    rc, _, _, _, _ = _geom(quad)
    assert rc == -1                                   # OCRVI_EINVAL
    assert len(_lib.last_error()) > 0
    with pytest.raises(ValueError, match="four_point_transform"):
        pipeline.four_point_geometry(quad)


def test_geometry_refuses_non_finite_and_null():
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    assert _geom([(0, 0), (np.nan, 0), (52, 36), (0, 36)])[0] == -1 and _lib.last_error()
    assert _geom([(0, 0), (1e300, 0), (52, 36), (0, 36)])[0] == -1 and _lib.last_error()      # overflows float32
    w = ctypes.c_int32(0)
    assert lib.ocrvi_four_point_transform(None, None, None, ctypes.byref(w), ctypes.byref(w)) == -1


def test_exports_header_and_abi():
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "ocrvi.h")).read()
    for name in ("ocrvi_four_point_transform", "ocrvi_warp_perspective_u8", "ocrvi_warp_perspective_pages"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "UNPINNED" in header[header.index("ocrvi_warp_perspective_u8") - 3000:header.index("ocrvi_warp_perspective_u8")]
    assert _lib.ABI_VERSION == 5 and lib.ocrvi_abi_version() == 5


def test_plan_rectified_matches_plan_buckets_on_the_rectified_sizes():
    from ocr_vi_invoice_amd.engine import plan_buckets, plan_rectified
    sizes = [(1000, 760), (4000, 3000), (900, 700), (60, 60), (40, 56)]
    quads = [None, LARGE, np.asarray(SMALL)[:, None, :] * 20, None, SMALL]           # (4, 1, 2): a cv2 contour's layout
    out_sizes, mats, shapes, scales, buckets = plan_rectified(sizes, quads, 320)
    want_sizes = []
    for hw, q in zip(sizes, quads):
        if q is None:
            want_sizes.append(hw)
        else:
            _, _, w, h, _, _ = WR.four_point_geometry(np.asarray(q).reshape(4, 2))
            want_sizes.append((h, w))
    assert out_sizes == want_sizes and out_sizes[1] == (3586, 2567) and out_sizes[4] == (27, 48)
    assert (shapes, scales, buckets) == plan_buckets(want_sizes, 320)
    assert [m is None for m in mats] == [True, False, False, True, False]
    for m, q in zip(mats, quads):
        if m is not None:
            assert m.dtype == np.float64 and m.shape == (9,)
            assert m.tobytes() == _geom(np.asarray(q).reshape(4, 2))[2].tobytes()
    # no quads at all: plan_buckets itself
    assert plan_rectified(sizes, None, 320)[2:] == plan_buckets(sizes, 320)
    assert plan_rectified(sizes, [None] * 5, 320)[0] == sizes


def test_plan_rectified_names_the_page_of_a_bad_quad():
    from ocr_vi_invoice_amd.engine import plan_rectified
    sizes = [(100, 80), (100, 80), (100, 80)]
    for bad in (DIAMOND, TINY, COLLINEAR, [(0, 0), (1, 1), (2, 2)], [[0, 0, 1]] * 4, [(0, 0), (50, 0), (50, float("inf")), (0, 40)],
                [(0, 0), (50, 0), (50, float("nan")), (0, 40)], "abcd", 7, [("a", "b")] * 4):
        with pytest.raises(ValueError, match="page 2"):
            plan_rectified(sizes, [None, RECT, bad], 320)
    with pytest.raises(ValueError, match="quads"):
        plan_rectified(sizes, [None, RECT], 320)
    # a quad that rectifies to a page the detector cannot take: plan_buckets' own error, for the rectified size
    with pytest.raises(ValueError, match="page 1"):
        plan_rectified(sizes, [None, [(0, 0), (2000, 0), (2000, 20), (0, 20)], None], 320)


def test_preprocess_image_without_a_quad_and_with_enhance():
    from ocr_vi_invoice_amd import pipeline
    img = np.zeros((8, 8, 3), np.uint8)
    assert pipeline.preprocess_image(img, None) is img
    with pytest.raises(NotImplementedError, match="enhance_document"):
        pipeline.preprocess_image(img, RECT, enhance=True)
