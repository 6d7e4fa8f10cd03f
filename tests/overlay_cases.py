"""The inputs of tests/test_gpu_overlay.py, shared with the mutant table of tests/test_overlay_cpu.py.  The kernel works on 64 x 16 pixel
tiles, tests 256 primitives per round and stages 256 segments per pass; the cases are laid out against those numbers.

BOX_CASES: name -> (page sizes [(h, w)], boxes per page, texts per page or None, thickness).
RAW_CASES: name -> ((h, w), segments [(ax, ay, bx, by, T)]): segment lists no box produces (a label would leave the legal range)."""
import numpy as np

import overlay_ref as R


def page(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _many_boxes():
    # 300 two-vertex boxes inside the tile x 64..127, y 16..31: 600 primitives (three rounds), far more than 256 segments in that tile
    rng = np.random.default_rng(5)
    a = np.stack([rng.integers(64, 128, 300), rng.integers(16, 32, 300)], 1)
    d = rng.integers(-4, 5, (300, 2))
    b = np.clip(a + d, (64, 16), (127, 31))
    return [np.stack([p, q]) for p, q in zip(a, b)]


def _zigzag():
    # one box of 400 vertices inside the tile x 64..127, y 32..47: one primitive whose segments need two passes
    rng = np.random.default_rng(6)
    return [np.stack([rng.integers(64, 128, 400), rng.integers(32, 48, 400)], 1)]


_BORDERS = [[(-10, -5), (30, 10), (20, 40), (-8, 30)], [(60, 50), (120, 55), (100, 90), (70, 80)], [(-20, 20), (110, 25), (110, 60), (-20, 62)],
            [(40.9, -30.2), (55.5, -30.9), (50.1, 100.7)]]                    # floats truncate towards zero (astype(np.int32))
_TILE_EDGES = [[(64, 16), (128, 16), (128, 32), (64, 32)], [(63, 15), (127, 15), (127, 47), (63, 47)], [(0, 48), (199, 48)], [(192, 0), (192, 129)]]
_DEGENERATE = [[(20, 30), (20, 30), (50, 35), (45, 50)], [(70, 40)], [], [(10, 50), (40, 55)], [(90, 5), (90, 5)]]
# label 1 lies on box 2's top edge, label 2 (below its box: 25 - 10 < 20) on box 3's top edge, label 3 on box 2's left edge; label 4 runs off the page
_OVERLAP = [[(20, 40), (80, 40), (80, 70), (20, 70)], [(10, 25), (60, 25), (60, 60), (10, 60)], [(5, 75), (50, 75), (50, 95), (5, 95)],
            [(85, 40), (89, 40), (89, 60), (85, 60)]]

BOX_CASES = {
    "borders": ([(70, 90)], [_BORDERS], None, 2),
    "borders_t1": ([(70, 90)], [_BORDERS], None, 1),
    "borders_t3": ([(70, 90)], [_BORDERS], None, 3),
    "tile_edges": ([(130, 200)], [_TILE_EDGES], None, 2),
    "tile_edges_t3": ([(130, 200)], [_TILE_EDGES], None, 3),
    "degenerate": ([(60, 100)], [_DEGENERATE], None, 2),
    "degenerate_t1": ([(60, 100)], [_DEGENERATE], None, 1),
    "degenerate_t3": ([(60, 100)], [_DEGENERATE], None, 3),
    "overlapping_labels": ([(100, 90)], [_OVERLAP], [["a", "b", "c", "d"]], 2),
    "many_boxes": ([(56, 192)], [_many_boxes()], None, 2),
    "zigzag": ([(64, 192)], [_zigzag()], None, 2),
    "inside": ([(200, 300)], [[[(10, 10), (290, 10), (290, 190), (10, 190)]]], None, 2),
    "five_pages": ([(70, 90), (33, 200), (128, 64), (16, 64), (100, 100)],
                   [_BORDERS, [[(5, 5), (190, 8), (180, 30), (3, 25)], [(100, -5), (150, 40)]], [[(0, 0), (63, 0), (63, 127), (0, 127)]], [],
                    [[(50, 50)], [(20, 60), (80, 20), (90, 90)]]],
                   [None, ["x"], None, None, ["x", "y", "z"]], 2),
    "thick": ([(90, 140)], [[[(30, 40), (100, 45), (90, 80)], [(70, 70)]]], None, 15),
}
RAW_CASES = {
    # the largest products: a diagonal between the corners of the legal range, and a shallow line through every tile column
    "huge": ((64, 16384), [(-16384, -16384, 16384, 16384, 15), (0, 40, 16384, 20, 15), (16383, 0, 16383, 63, 1)]),
    "mixed_thickness": ((40, 70), [(5, 5, 60, 30, 15), (5, 30, 60, 5, 4), (30, 20, 30, 20, 9), (0, 39, 69, 39, 1)]),
}


def box_case(name):
    """(pages, boxes per page, pairs per page, thickness) of a box case; the pages are random bytes."""
    sizes, boxes, texts, T = BOX_CASES[name]
    pages = [page(h, w, 100 + k) for k, (h, w) in enumerate(sizes)]
    pairs = [len(b) if texts is None or texts[k] is None else min(len(b), len(texts[k])) for k, b in enumerate(boxes)]
    return pages, boxes, texts, pairs, T


def raw_case(name):
    """(page, segs [n, 8], prims [n, 8]) of a raw case: one primitive per segment, colours by ordinal."""
    (h, w), lines = RAW_CASES[name]
    segs = [(ax, ay, bx, by, R.rgb(((37 * k + 11) % 256, (91 * k + 200) % 256, (53 * k) % 256)), T, k, 0) for k, (ax, ay, bx, by, T) in enumerate(lines)]
    prims = [R.primitive(segs, k, k + 1, 0, k) for k in range(len(segs))]
    return page(h, w, 7), np.asarray(segs, np.int64), np.asarray(prims, np.int64)
