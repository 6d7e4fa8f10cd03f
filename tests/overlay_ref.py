"""The result overlay (include/ocrvi.h, "Result overlay"; draw_boxes_with_text, src/pipeline/pipeline2.py:173-190) restated in numpy int64:
``segments`` builds the segment and primitive tables of one page, ``paint`` tests every pixel against every segment, the largest ordinal
wins.  ``covered_fraction`` states the coverage of one pixel a second time, through the exact distance to the segment in
``fractions.Fraction``.  ``mutant`` selects one deliberately wrong variant (MUTANTS); tests/test_overlay_cpu.py shows that each changes
the output of an input the GPU test uses."""
from fractions import Fraction

import numpy as np

# stroke s = (from.x, from.y, to.x, to.y) relative to the digit's origin (bottom-left), A..G; digit -> its strokes
STROKES = {"A": (0, -10, 6, -10), "B": (6, -10, 6, -5), "C": (6, -5, 6, 0), "D": (0, 0, 6, 0), "E": (0, -5, 0, 0), "F": (0, -10, 0, -5),
           "G": (0, -5, 6, -5)}
DIGITS = {0: "ABCDEF", 1: "BC", 2: "ABDEG", 3: "ABCDG", 4: "BCFG", 5: "ACDFG", 6: "ACDEFG", 7: "ABC", 8: "ABCDEFG", 9: "ABCDFG"}
ADVANCE = 10
SEG, PRIM = 8, 8
MUTANTS = ("< for <=", "end caps dropped", "smallest ordinal wins", "closing edge missing", "label before outline", "floor before multiply")


def rgb(c):
    return int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16


def text_pos(v):
    """pipeline2.py:182-187 on the int32 vertices v [n, 2]."""
    top = int(np.argmin(v[:, 1]))                # the first vertex of minimum y
    x, y = int(v[top, 0]), int(v[top, 1]) - 10
    if y < 20:
        y = int(v[:, 1].max()) + 20
    return x, y


def label_strokes(number, pos):
    out = []
    for k, ch in enumerate(str(number)):
        ox = pos[0] + ADVANCE * k
        for s in DIGITS[int(ch)]:                # the strings are in the order A..G
            x0, y0, x1, y1 = STROKES[s]
            out.append((ox + x0, pos[1] + y0, ox + x1, pos[1] + y1))
    return out


def primitive(segs, first, last, kind, pair):
    """The primitive of segs[first:last]: its range and the bounding box of its endpoints dilated by ceil(T / 2)."""
    s = np.asarray(segs[first:last], np.int64)
    dil = (int(s[0, 5]) + 1) // 2
    xs, ys = s[:, [0, 2]], s[:, [1, 3]]
    return (first, last, int(xs.min()) - dil, int(ys.min()) - dil, int(xs.max()) + dil, int(ys.max()) + dil, kind, pair)


def segments(boxes, n_pairs=None, color=(0, 255, 0), label_color=(255, 0, 0), thickness=2, mutant=None, first=0):
    """One page: (segs int64 [n, 8], prims int64 [m, 8]); segment numbers start at ``first``."""
    segs, prims = [], []
    n_pairs = len(boxes) if n_pairs is None else min(len(boxes), n_pairs)
    for i in range(n_pairs):
        v = np.asarray(boxes[i]).reshape(-1, 2).astype(np.int32)
        n = len(v)
        if n == 0:
            continue
        edges = [(int(v[k, 0]), int(v[k, 1]), int(v[(k + 1) % n, 0]), int(v[(k + 1) % n, 1])) for k in range(n)]
        if mutant == "closing edge missing" and n > 1:
            edges = edges[:-1]
        parts = [(0, edges, rgb(color)), (1, label_strokes(i + 1, text_pos(v)), rgb(label_color))]
        if mutant == "label before outline":
            parts.reverse()
        for kind, lines, colour in parts:
            a = len(segs)
            segs.extend((x0, y0, x1, y1, colour, thickness, i, 0) for x0, y0, x1, y1 in lines)
            prims.append(primitive(segs, a, len(segs), kind, i))
    segs = np.asarray(segs, np.int64).reshape(-1, SEG)
    prims = np.asarray(prims, np.int64).reshape(-1, PRIM)
    prims[:, :2] += first
    return segs, prims


def tables(boxes_per_page, pairs_per_page=None, **kw):
    """Several pages: (segs, prims, prim_offs) as ocrvi_overlay_segments lists them."""
    segs, prims, offs = [], [], [0]
    for p, boxes in enumerate(boxes_per_page):
        s, q = segments(boxes, None if pairs_per_page is None else pairs_per_page[p], first=sum(len(x) for x in segs), **kw)
        segs.append(s)
        prims.append(q)
        offs.append(offs[-1] + len(q))
    return np.concatenate(segs or [np.zeros((0, SEG), np.int64)]), np.concatenate(prims or [np.zeros((0, PRIM), np.int64)]), np.asarray(offs)


def covered(x, y, seg, mutant=None):
    """The painting rule for pixel centres (x, y) (int64 arrays) and one segment."""
    ax, ay, bx, by, T = (int(v) for v in (seg[0], seg[1], seg[2], seg[3], seg[5]))
    le = (lambda a, b: a < b) if mutant == "< for <=" else (lambda a, b: a <= b)
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    qx, qy = x - ax, y - ay
    t = qx * dx + qy * dy
    cap_a = le(4 * (qx * qx + qy * qy), T * T)
    cap_b = le(4 * ((x - bx) ** 2 + (y - by) ** 2), T * T)
    if mutant == "end caps dropped":
        cap_a = cap_b = np.zeros_like(cap_a)
    c = dx * qy - dy * qx
    K = (T * T // 4) * L2 if mutant == "floor before multiply" else (T * T * L2) // 4
    return np.where(t <= 0, cap_a, np.where(t >= L2, cap_b, le(c * c, K)))


def paint(page, segs, mutant=None):
    """A new page: every pixel against every segment, the colour of the largest covering ordinal; other pixels unchanged."""
    h, w = page.shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    smallest = mutant == "smallest ordinal wins"
    best = np.full((h, w), len(segs) if smallest else -1, np.int64)
    for s, seg in enumerate(segs):
        cov = covered(x, y, seg, mutant)
        best = np.where(cov, np.minimum(best, s) if smallest else np.maximum(best, s), best)
    out = page.copy()
    hit = (best >= 0) & (best < len(segs))
    colour = np.asarray(segs, np.int64).reshape(-1, SEG)[best[hit], 4]
    out[hit] = np.stack([colour & 255, (colour >> 8) & 255, (colour >> 16) & 255], -1).astype(np.uint8)
    return out


def draw(page, boxes, n_pairs=None, mutant=None, **kw):
    return paint(page, segments(boxes, n_pairs, mutant=mutant, **kw)[0], mutant)


def covered_fraction(x, y, seg):
    """The same pixel test through the exact distance: 4 dist(p, segment)^2 <= T^2."""
    ax, ay, bx, by, T = (int(v) for v in (seg[0], seg[1], seg[2], seg[3], seg[5]))
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    u = Fraction(0) if L2 == 0 else min(Fraction(1), max(Fraction(0), Fraction((x - ax) * dx + (y - ay) * dy, L2)))
    cx, cy = ax + u * dx, ay + u * dy
    return 4 * ((x - cx) ** 2 + (y - cy) ** 2) <= T * T
