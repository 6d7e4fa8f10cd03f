"""Document finder, host half (include/ocrvi.h, "Document finder"): ocrvi_document_contour and its bit-mask sibling against the Python
statement in tests/docfind_ref.py, the restatement itself on three synthetic photos, and its Otsu against a brute-force float64
between-class variance.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import docfind_ref as DR

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_EXPORTS = ("ocrvi_document_contour", "ocrvi_document_contour_bits", "ocrvi_doc_working_size", "ocrvi_doc_mask_sizes", "ocrvi_doc_mask_pages",
               "ocrvi_doc_grey_u8", "ocrvi_doc_smooth_u8", "ocrvi_doc_histogram", "ocrvi_doc_otsu", "ocrvi_doc_mask_bits")
QUAD = ((30, 20), (150, 35), (165, 170), (18, 150))


def _quad(h, w, quad):
    return DR._inside(h, w, quad).astype(np.uint8) * 255


def _ellipse(h, w, cx, cy, a, b):
    ys, xs = np.mgrid[0:h, 0:w]
    return ((((xs - cx) / a) ** 2 + ((ys - cy) / b) ** 2) <= 1).astype(np.uint8) * 255


def _six_blobs():
    m = np.zeros((220, 400), np.uint8)
    for k, r in enumerate((40, 36, 32, 28, 24)):
        m |= _ellipse(220, 400, 50 + 75 * k, 60, r * 0.9, r)
    m |= _quad(220, 400, ((20, 150), (50, 152), (52, 180), (18, 178)))        # 900-odd pixels: smaller than every ellipse
    return m


def _ring_with_blob():
    m = _ellipse(200, 220, 110, 100, 100, 90) & ~_ellipse(200, 220, 110, 100, 80, 70)
    return m | _quad(200, 220, ((80, 70), (140, 72), (138, 130), (82, 128)))


def _soft():
    hard = _quad(200, 190, QUAD) != 0
    p = np.pad(hard, 2)
    grown = np.logical_or.reduce([p[dy:dy + 200, dx:dx + 190] for dy in range(5) for dx in range(5)])
    rim = 1 + (np.arange(200)[:, None] * 7 + np.arange(190)[None, :] * 13) % 254          # 1 .. 254
    return np.where(hard, 255, np.where(grown, rim, 0)).astype(np.uint8)


def _notched():
    m = _quad(200, 190, QUAD)
    m[80:92, 150:170] = 0            # a notch cut into the right side, well inside 2 % of the perimeter
    return m


def _strided():
    big = np.full((200, 256), 255, np.uint8)        # what lies beyond the mask's columns is foreground: reading it would change the answer
    big[:, :190] = _quad(200, 190, QUAD)
    return big[:, :190]


def _line():
    m = np.zeros((40, 60), np.uint8)
    m[17, 5:50] = 255
    return m


def _pixel():
    m = np.zeros((9, 11), np.uint8)
    m[4, 6] = 1
    return m


# name: (mask, the kind expected, or ... when only agreement with the restatement is asked)
MASKS = {
    "a filled convex quadrilateral": (lambda: _quad(200, 190, QUAD), "polygon"),
    "the same with a notch cut into one side": (_notched, "polygon"),
    "a large ellipse plus a smaller quadrilateral": (lambda: _ellipse(300, 400, 130, 150, 120, 140) | _quad(300, 400, ((280, 60), (380, 70), (375, 200), (285, 190))),
                                                     "polygon"),
    "an ellipse alone": (lambda: _ellipse(300, 260, 130, 150, 120, 140), "rectangle"),
    "six blobs of which only the sixth-largest is a quadrilateral": (_six_blobs, "rectangle"),
    "a ring with a blob inside its hole": (_ring_with_blob, "rectangle"),
    "two contours of equal area": (lambda: _quad(120, 300, ((20, 20), (100, 24), (104, 90), (16, 86))) | _quad(120, 300, ((170, 20), (250, 24), (254, 90), (166, 86))),
                                   "polygon"),
    "a single pixel": (_pixel, ...),
    "a one-pixel line": (_line, ...),
    "an all-zero mask": (lambda: np.zeros((50, 70), np.uint8), None),
    "an all-255 mask": (lambda: np.full((50, 70), 255, np.uint8), ...),
    "a soft mask with values 1..254 at the rim": (_soft, "polygon"),
    "a strided mask": (_strided, "polygon"),
}


def _lib_contour(mask):
    from ocr_vi_invoice_amd import pipeline
    return pipeline.find_document_contour(mask, return_kind=True)


def _same(got, want):
    return (got is None and want is None) or (got is not None and want is not None and got.dtype == np.int32 and np.array_equal(got, want))


def test_exports_match_the_header_and_the_abi_is_still_5():
    from ocr_vi_invoice_amd import _lib
    import ocr_vi_invoice_amd as pkg
    lib = _lib.load()
    with open(os.path.join(HERE, "..", "include", "ocrvi.h")) as f:
        header = f.read()
    for n in NEW_EXPORTS:
        assert n in _lib.EXPORTS and hasattr(lib, n) and re.search(r"\bint " + n + r"\(", header), n
    for k, v in _lib.DOC_POLARITIES.items():
        assert f"#define OCRVI_DOC_{k.upper()} {v}\n" in header
    assert lib.ocrvi_abi_version() == 5 == _lib.ABI_VERSION
    for n in ("find_document_contour", "document_mask", "find_document_quad", "find_document_quads"):
        assert callable(getattr(pkg, n))


@pytest.mark.parametrize("name", list(MASKS))
def test_document_contour_equals_the_restatement(name):
    make, kind = MASKS[name]
    mask = make()
    want, want_kind = DR.document_contour(mask)
    got, got_kind = _lib_contour(mask)
    assert got_kind == want_kind and _same(got, want), (got, got_kind, want, want_kind)
    if kind is not ...:
        assert got_kind == kind


def test_the_cases_are_what_their_names_say():
    from oracle import dbpost_cpu
    cnts = DR.external_contours(MASKS["a large ellipse plus a smaller quadrilateral"][0]())
    first = sorted(cnts, key=dbpost_cpu.contour_area, reverse=True)[0]
    assert len(dbpost_cpu.approx_poly_dp_closed(first, 0.02 * dbpost_cpu.arc_length_closed(first))) > 4      # the ellipse is passed over
    assert len(DR.external_contours(_six_blobs())) == 6
    assert len(DR.external_contours(_ring_with_blob())) == 1 and len(dbpost_cpu.find_contours(_ring_with_blob())) == 3
    a, b = DR.external_contours(MASKS["two contours of equal area"][0]())
    assert dbpost_cpu.contour_area(a) == dbpost_cpu.contour_area(b) and a[:, 0].min() > b[:, 0].max()          # the last found comes first
    assert DR.document_contour(MASKS["two contours of equal area"][0]())[0][:, 0].min() > 150
    assert _lib_contour(MASKS["two contours of equal area"][0]())[0][:, 0].min() > 150                       # and so it does in the library
    blob = _ring_with_blob() & _ellipse(200, 220, 110, 100, 75, 65)                                           # the blob without its ring
    assert _lib_contour(_ring_with_blob())[1] == "rectangle" and _lib_contour(blob)[1] == "polygon" and blob.any()
    soft = _soft()
    assert ((soft > 0) & (soft < 255)).sum() > 100 and not np.array_equal(soft > 0, soft == 255)
    # the notch is deep enough to matter to the border, and the polygon still has four points
    assert len(DR.external_contours(_notched())[0]) > len(DR.external_contours(_quad(200, 190, QUAD))[0])


@pytest.mark.parametrize("name", list(MASKS))
def test_the_bit_mask_sibling_equals_the_byte_form(name):
    from ocr_vi_invoice_amd import _lib
    mask = np.ascontiguousarray(MASKS[name][0]())
    bits = np.ascontiguousarray(DR.pack_bits(mask))
    assert np.array_equal(DR.unpack_bits(bits, *mask.shape) != 0, mask != 0)
    quad, found = np.full((4, 2), -7, np.int32), ctypes.c_int32(-7)
    _lib.check(_lib.load().ocrvi_document_contour_bits(bits.ctypes.data, mask.shape[0], mask.shape[1], quad.ctypes.data, ctypes.byref(found)))
    want, kind = _lib_contour(mask)
    assert (None, "polygon", "rectangle")[found.value] == kind
    assert np.array_equal(quad, want if want is not None else np.zeros((4, 2), np.int32))


def test_bad_arguments_are_refused():
    from ocr_vi_invoice_amd import pipeline
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 3), np.uint8), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError, match="find_document_contour"):
            pipeline.find_document_contour(bad)
    assert pipeline.doc_working_size(1280, 960) == (375, 2.56) == DR.working_size(1280, 960, 500)
    for h, w, work_h in ((296, 41, 37), (64, 8200 * 8, 64), (100, 100, 7), (100, 100, 513), (16385, 9000, 500)):
        with pytest.raises(ValueError):
            pipeline.doc_working_size(h, w, work_h)
        with pytest.raises(ValueError):
            DR.working_size(h, w, work_h)


# Measured on the CPU with tests/docfind_ref.py (profiles/r22_docfind.md): the largest corner error of the three scenes, in working pixels.
MEASURED_WORKING_PIXELS = 1.90    # 1.54 bright_on_dark, 1.90 dark_on_bright, 1.20 touching_edge
BOUND_WORKING_PIXELS = 4          # twice the measured value, rounded up to a whole working pixel


@pytest.mark.parametrize("name", list(DR.PHOTOS))
def test_the_restatement_finds_the_corners_of_the_synthetic_photos(name):
    img, truth = DR.photo(name)
    ratio = DR.working_size(img.shape[0], img.shape[1], 500)[1]
    st = DR.stages(img)
    assert st["inverted"] == (name == "dark_on_bright")
    quad, kind = DR.document_contour(st["mask"])
    assert kind == "polygon"
    err = DR.corner_error(quad.astype(np.float64) * ratio, truth)
    print(f"{name}: Otsu {st['t']}, corner error {err:.2f} source pixels = {err / ratio:.2f} working pixels")
    assert err <= BOUND_WORKING_PIXELS * ratio
    assert np.array_equal(DR.find_quad(img), quad.astype(np.float64) * ratio)
    got, got_kind = _lib_contour(st["mask"].astype(np.uint8) * 255)          # the library's host half on the same mask
    assert got_kind == "polygon" and np.array_equal(got, quad)


def test_otsu_agrees_with_a_brute_force_between_class_variance():
    rng = np.random.default_rng(22)
    checked = 0
    for k in range(60):
        lo, hi = sorted(rng.integers(0, 256, 2).tolist())
        hist = np.zeros(256, np.int64)
        hist[lo:hi + 1] = rng.integers(0, 4000, hi - lo + 1)
        if k % 3 == 0:                                # two humps
            hist += (3000 * np.exp(-0.5 * ((np.arange(256) - rng.integers(20, 236)) / 9.0) ** 2)).astype(np.int64)
        if (hist > 0).sum() < 2:
            continue
        t, var = DR.otsu_brute(hist)
        top = np.sort(var)[::-1]
        if top[1] >= top[0] * (1 - 1e-9):             # near-tied maxima: rounding decides, not the definition
            continue
        assert DR.otsu(hist) == t
        checked += 1
    assert checked >= 40
    assert DR.otsu(np.bincount([77] * 9, minlength=256)) == -1                  # a single bin: no threshold
    assert DR.otsu(np.bincount([10] * 5 + [200] * 5, minlength=256)) == 10      # every t in 10 .. 199 ties: the smallest
