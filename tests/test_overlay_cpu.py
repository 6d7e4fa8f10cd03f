"""The result overlay's host half: tests/overlay_ref.py against its own second statement (fractions) and the hand case, then
ocrvi_overlay_segments (include/ocrvi.h) against the reference entry for entry, the label rule, the zip truncation, every OCRVI_EINVAL,
and a table of deliberately wrong references, each of which must change the output of an input tests/test_gpu_overlay.py paints.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_cases as cases  # noqa: E402
import overlay_ref as R  # noqa: E402


def _seg(ax, ay, bx, by, T=2, colour=0x0000ff):
    return (ax, ay, bx, by, colour, T, 0, 0)


def test_hand_case_23_pixels():
    page = np.zeros((12, 12, 3), np.uint8)
    out = R.paint(page, [_seg(2, 5, 8, 5, 2, R.rgb((9, 8, 7)))])
    want = {(x, y) for x in range(2, 9) for y in range(4, 7)} | {(1, 5), (9, 5)}
    got = {(int(x), int(y)) for y, x in zip(*np.nonzero(out.any(-1)))}
    assert len(want) == 23 and got == want
    assert all(tuple(out[y, x]) == (9, 8, 7) for x, y in want)


@pytest.mark.parametrize("T", [1, 2, 3, 15])
def test_integer_rule_equals_the_fraction_statement(T):
    rng = np.random.default_rng(T)
    y, x = np.mgrid[0:24, 0:24].astype(np.int64)
    ends = rng.integers(-6, 30, (40, 4))
    ends[0] = (5, 5, 5, 5)                       # a point
    ends[1] = (3, 20, 20, 20)                    # axis-parallel
    ends[2] = (-6, -6, 29, 29)                   # a diagonal through the window
    for e in ends:
        seg = _seg(*(int(v) for v in e), T=T)
        got = R.covered(x, y, seg)
        want = np.array([[R.covered_fraction(i, j, seg) for i in range(24)] for j in range(24)])
        assert np.array_equal(got, want), (seg, np.argwhere(got != want)[:4])


def _lib_tables(boxes, texts, sizes, T, **kw):
    from ocr_vi_invoice_amd import pipeline
    return pipeline.overlay_segments(boxes, texts, sizes, thickness=T, **kw)


@pytest.mark.parametrize("name", sorted(cases.BOX_CASES))
def test_overlay_segments_equals_the_reference(name):
    pages, boxes, texts, pairs, T = cases.box_case(name)
    segs, prims, offs = _lib_tables(boxes, texts, [p.shape[:2] for p in pages], T)
    rs, rp, ro = R.tables(boxes, pairs, thickness=T)
    assert segs.dtype == np.int32 and prims.dtype == np.int32 and offs.dtype == np.int32
    assert np.array_equal(segs, rs) and np.array_equal(prims, rp) and np.array_equal(offs, ro)
    assert len(segs) > 0


def test_colours_and_upper_bound():
    boxes = [[[(10, 40), (50, 40), (30, 70)]] * 12]
    segs, prims, _ = _lib_tables(boxes, None, [(100, 100)], 4, color=(1, 2, 3), label_color=(250, 251, 252))
    rs, rp, _ = R.tables(boxes, None, thickness=4, color=(1, 2, 3), label_color=(250, 251, 252))
    assert np.array_equal(segs, rs) and np.array_equal(prims, rp)
    assert set(segs[:, 4]) == {1 | 2 << 8 | 3 << 16, 250 | 251 << 8 | 252 << 16}
    assert len(segs) <= sum(3 + 7 * len(str(i + 1)) for i in range(12)) and len(prims) == 24
    assert np.array_equal(prims[0, 2:6], (10 - 2, 40 - 2, 50 + 2, 70 + 2))       # dilated by ceil(4 / 2)
    assert np.array_equal(_lib_tables(boxes, None, [(100, 100)], 3)[1][0, 2:6], (10 - 2, 40 - 2, 50 + 2, 70 + 2))   # ceil(3 / 2) = 2


def _label_origin(segs, prims, k):
    """The text_pos of label primitive k, read back from its strokes (every digit has stroke B or C at x + 6, and reaches y - 10 .. y)."""
    s = segs[prims[k, 0]:prims[k, 1]]
    assert prims[k, 6] == 1
    return int(s[:, [0, 2]].max()) - 6 - 10 * (len(str(int(prims[k, 7]) + 1)) - 1), int(s[:, [1, 3]].max())


def test_label_rule():
    # top vertex at y = 30: text_pos.y = 20, the label stays above; at y = 29: 19 < 20, it goes below max_y + 20
    above = [(40, 30), (80, 32), (80, 60), (40, 58)]
    below = [(40, 29), (80, 32), (80, 60), (40, 58)]
    tie = [(70, 50), (20, 45), (60, 45), (30, 90)]      # two vertices of minimum y: the first, (20, 45), wins
    segs, prims, _ = _lib_tables([[above, below, tie]], None, [(100, 100)], 2)
    assert _label_origin(segs, prims, 1) == (40, 20) == R.text_pos(np.array(above))
    assert _label_origin(segs, prims, 3) == (40, 80) == R.text_pos(np.array(below))
    assert _label_origin(segs, prims, 5) == (20, 35) == R.text_pos(np.array(tie))


def test_label_digits_and_advance():
    box = [(100, 200), (300, 200), (300, 260), (100, 260)]
    n = 1000
    segs, prims, _ = _lib_tables([[box] * n], None, [(400, 400)], 2)
    rs, rp, _ = R.tables([[box] * n], None)
    assert np.array_equal(segs, rs) and np.array_equal(prims, rp)
    for idx in (9, 10, 100, 1000):               # the label of box idx (0-based idx - 1) shows the number idx
        k = 2 * (idx - 1) + 1
        s = segs[prims[k, 0]:prims[k, 1]]
        digits = len(str(idx))
        assert len(s) == sum(len(R.DIGITS[int(c)]) for c in str(idx))
        assert int(s[:, [0, 2]].min()) >= 100 and int(s[:, [0, 2]].max()) == 100 + 10 * (digits - 1) + 6
        want = [(100 + 10 * d + R.STROKES[c][0], 190 + R.STROKES[c][1]) for d, ch in enumerate(str(idx)) for c in R.DIGITS[int(ch)]]
        assert [tuple(v) for v in s[:, :2]] == want


def test_zip_truncation():
    box = [(10, 40), (50, 40), (30, 70)]
    full = _lib_tables([[box] * 5], None, [(100, 100)], 2)
    cut = _lib_tables([[box] * 5], [["a", "b"]], [(100, 100)], 2)
    assert len(full[1]) == 10 and len(cut[1]) == 4 and np.array_equal(cut[1], full[1][:4]) and np.array_equal(cut[0], full[0][:cut[1][-1, 1]])
    assert len(_lib_tables([[box] * 5], [[]], [(100, 100)], 2)[0]) == 0
    assert np.array_equal(_lib_tables([[box] * 2], [["a"] * 7], [(100, 100)], 2)[1], full[1][:4])     # more texts than boxes
    # a box past the last pair is never looked at, as under zip: a vertex out of range or a malformed box there changes nothing
    junk = _lib_tables([[box, box, [(99999, 0), (1, 1)], "not a box"]], [["a", "b"]], [(100, 100)], 2)
    assert np.array_equal(junk[0], cut[0]) and np.array_equal(junk[1], cut[1])
    with pytest.raises(ValueError):
        _lib_tables([[box, [(99999, 0), (1, 1)]]], [["a", "b"]], [(100, 100)], 2)


def _raw_call(points, offs, page_boxes, page_hw, T=2, box_rgb=0x00ff00, label_rgb=0x0000ff, query=True, null=()):
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    pts, offs = np.asarray(points, np.int32).reshape(-1, 2), np.asarray(offs, np.int32)
    pb, hw = np.asarray(page_boxes, np.int32), np.asarray(page_hw, np.int32).reshape(-1, 2)
    ns, npr = ctypes.c_int64(-1), ctypes.c_int64(-1)
    segs, prims, po = np.zeros((64, 8), np.int32), np.zeros((64, 8), np.int32), np.zeros(len(pb), np.int32)
    out = (None, 0, None, 0, None) if query else (segs.ctypes.data, 64, prims.ctypes.data, 64, po.ctypes.data)
    arg = lambda name, v: None if name in null else v   # noqa: E731
    rc = lib.ocrvi_overlay_segments(arg("points", pts.ctypes.data), arg("offs", offs.ctypes.data), arg("page_boxes", pb.ctypes.data), None,
                                    arg("page_hw", hw.ctypes.data), len(hw), box_rgb, label_rgb, T, *out,
                                    arg("n_segs", ctypes.byref(ns)), arg("n_prims", ctypes.byref(npr)))
    return rc, ns.value, npr.value, _lib.last_error()


def test_every_einval():
    from ocr_vi_invoice_amd import pipeline
    tri, offs = [(10, 40), (50, 40), (30, 70)], [0, 3]
    assert _raw_call(tri, offs, [0, 1], [(100, 100)])[:3] == (0, 3 + 2, 2)
    assert _raw_call(tri, offs, [0, 1], [(100, 100)], query=False)[:3] == (0, 5, 2)
    assert _raw_call([(-16384, 40), (16384, 16384), (30, 70)], offs, [0, 1], [(16384, 16384)])[0] == 0      # the ends of the range are legal
    for bad in ([(16385, 40), (50, 40), (30, 70)], [(10, 40), (50, -16385), (30, 70)]):
        rc, _, _, msg = _raw_call(bad, offs, [0, 1], [(100, 100)])
        assert rc == -1 and "16384" in msg
    # a label endpoint past the range: text_pos.y = max_y + 20
    assert _raw_call([(10, 5), (50, 16380)], [0, 2], [0, 1], [(100, 100)])[0] == -1
    for hw in ((0, 100), (100, 0), (16385, 100), (100, 16385)):
        assert _raw_call(tri, offs, [0, 1], [hw])[0] == -1
    for T in (0, 16, -1):
        assert _raw_call(tri, offs, [0, 1], [(100, 100)], T=T)[0] == -1
    assert _raw_call(tri, offs, [0, 1], [(100, 100)], box_rgb=0x1000000)[0] == -1
    for name in ("offs", "page_boxes", "page_hw", "n_segs", "n_prims", "points"):
        assert _raw_call(tri, offs, [0, 1], [(100, 100)], null=(name,))[0] == -1, name
    assert _raw_call(tri, [3, 0], [0, 1], [(100, 100)])[0] == -1                      # offsets that run backwards
    assert _raw_call(tri, offs, [1, 0], [(100, 100)])[0] == -1
    # the facade turns each into ValueError, before any device work (no GPU here)
    for kw in (dict(thickness=0), dict(thickness=16), dict(thickness=2.0), dict(color=(0, 256, 0)), dict(label_color=(1, 2))):
        with pytest.raises(ValueError):
            pipeline.overlay_segments([[tri]], None, [(100, 100)], **kw)
    for boxes, size in (([[(16385, 0), (1, 1)]], (100, 100)), ([[(float("nan"), 0), (1, 1)]], (100, 100)), ([tri], (0, 5)), ([tri], (5, 16385)),
                        ([[1, 2, 3]], (100, 100))):
        with pytest.raises(ValueError):
            pipeline.overlay_segments([boxes], None, [size])
    page = np.zeros((20, 20, 3), np.uint8)
    for bad in (np.zeros((20, 20), np.uint8), np.zeros((20, 20, 4), np.uint8), np.zeros((20, 20, 3), np.float32), "page"):
        with pytest.raises(ValueError):
            pipeline.draw_boxes_with_text(bad, [tri])
    with pytest.raises(ValueError):
        pipeline.draw_boxes_pages([page, page], [[tri]])
    with pytest.raises(ValueError):
        pipeline.draw_boxes_with_text(page, [[(16385, 0), (1, 1)]])


def test_tables_too_small_are_refused():
    from ocr_vi_invoice_amd import _lib
    lib = _lib.load()
    pts, offs = np.asarray([(10, 40), (50, 40), (30, 70)], np.int32), np.asarray([0, 3], np.int32)
    pb, hw = np.asarray([0, 1], np.int32), np.asarray([(100, 100)], np.int32)
    ns, npr = ctypes.c_int64(), ctypes.c_int64()
    segs, prims, po = np.zeros((8, 8), np.int32), np.zeros((8, 8), np.int32), np.zeros(2, np.int32)
    for sc, pc in ((4, 2), (5, 1)):
        rc = lib.ocrvi_overlay_segments(pts.ctypes.data, offs.ctypes.data, pb.ctypes.data, None, hw.ctypes.data, 1, 1, 2, 2, segs.ctypes.data, sc,
                                        prims.ctypes.data, pc, po.ctypes.data, ctypes.byref(ns), ctypes.byref(npr))
        assert rc == -1
    rc = lib.ocrvi_overlay_segments(pts.ctypes.data, offs.ctypes.data, pb.ctypes.data, None, hw.ctypes.data, 1, 1, 2, 2, segs.ctypes.data, 5,
                                    None, 2, po.ctypes.data, ctypes.byref(ns), ctypes.byref(npr))
    assert rc == -1                                  # the three tables come together


def test_every_mutant_changes_a_gpu_case():
    """Each wrong variant of the reference against the right one on the inputs of tests/test_gpu_overlay.py: the first case whose painted
    page differs is printed; a variant no case tells apart would pass the GPU test unnoticed."""
    right = {}
    table = {}
    order = ["borders_t1", "degenerate_t3", "overlapping_labels", "tile_edges", "borders", "degenerate", "thick"]
    for m in R.MUTANTS:
        for name in order:
            pages, boxes, _, pairs, T = cases.box_case(name)
            if name not in right:
                right[name] = [R.draw(p, b, n, thickness=T) for p, b, n in zip(pages, boxes, pairs)]
            wrong = [R.draw(p, b, n, thickness=T, mutant=m) for p, b, n in zip(pages, boxes, pairs)]
            diff = sum(int((w != r).any(-1).sum()) for w, r in zip(wrong, right[name]))
            if diff:
                table[m] = (name, diff)
                break
    print("\n[overlay mutants] first GPU case that tells the variant from the reference, pixels that differ")
    for m in R.MUTANTS:
        print(f"  {m:24s} {table.get(m)}")
    assert set(table) == set(R.MUTANTS)
