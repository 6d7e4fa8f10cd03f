"""Reference for the document finder (include/ocrvi.h, "Document finder"), independent of the library's C++ and kernels.

Part B, the library's own mask, is restated stage by stage in numpy integers (``grey``, ``smooth``, ``histogram``, ``otsu``, ``inverted``,
``opening``, ``pack_bits``; ``stages`` runs them all); Otsu's score is the one place with floating point, Python floats in the header's
order.  Part A, mask -> corners (src/preprocess/scanner.py:104-132), builds on ``oracle.dbpost_cpu`` for border following, ``arcLength``,
``approxPolyDP`` and ``contourArea`` and on ``quad_ref`` for the minimum-area rectangle.  Which borders are external is decided here
without the tracer: components by ``scipy.ndimage.label``, the background that reaches the frame by a second labelling.

``photo`` builds the three seeded synthetic scenes of the tests, with the true corners."""
import math

import numpy as np
from scipy import ndimage

import quad_ref
from oracle import dbpost_cpu

MIN_WW, MAX_WW, MIN_WORK_H, MAX_WORK_H, MAX_SIDE = 8, 8192, 8, 512, 16384
POLARITIES = ("auto", "bright", "dark")


# ---------------------------------------------------------------------------------------------------- B: the mask
def working_size(h, w, work_h):
    """-> (ww, ratio); ValueError outside the header's bounds."""
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and MIN_WORK_H <= work_h <= MAX_WORK_H):
        raise ValueError(f"{h} x {w} at {work_h} rows")
    ratio = h / float(work_h)
    ww = int(w / ratio)
    if not MIN_WW <= ww <= MAX_WW:
        raise ValueError(f"working width {ww}")
    return ww, ratio


def _edges(n_src, n_dst):
    lo = [(i * n_src) // n_dst for i in range(n_dst)]
    hi = [max(lo[i] + 1, ((i + 1) * n_src) // n_dst) for i in range(n_dst)]
    return np.asarray(lo), np.asarray(hi)


def grey(img, work_h):
    h, w = img.shape[:2]
    ww, _ = working_size(h, w, work_h)
    p = img.astype(np.int64)
    luma = (77 * p[:, :, 0] + 150 * p[:, :, 1] + 29 * p[:, :, 2] + 128) >> 8
    integral = np.zeros((h + 1, w + 1), np.int64)
    integral[1:, 1:] = luma.cumsum(0).cumsum(1)
    r0, r1 = _edges(h, work_h)
    c0, c1 = _edges(w, ww)
    s = integral[r1][:, c1] - integral[r0][:, c1] - integral[r1][:, c0] + integral[r0][:, c0]
    n = (r1 - r0)[:, None] * (c1 - c0)[None, :]
    return ((s + n // 2) // n).astype(np.uint8)


def smooth(g):
    k = (1, 4, 6, 4, 1)
    p = np.pad(g.astype(np.int64), 2, mode="edge")
    hs = sum(k[d] * p[:, d:d + g.shape[1]] for d in range(5))
    vs = sum(k[d] * hs[d:d + g.shape[0], :] for d in range(5))
    return ((vs + 128) >> 8).astype(np.uint8)


def histogram(s):
    return np.bincount(s.reshape(-1), minlength=256).astype(np.int32)


def otsu(hist):
    """The smallest t of maximal score, -1 when every t is skipped (a single non-empty bin)."""
    h = [int(v) for v in hist]
    n, m_t = sum(h), sum(v * c for v, c in enumerate(h))
    best, best_t, w0, m0 = -1.0, -1, 0, 0
    for t in range(255):
        w0 += h[t]
        m0 += t * h[t]
        w1 = n - w0
        if w0 == 0 or w1 == 0:
            continue
        d = m_t * w0 - m0 * n
        assert abs(d) < 2 ** 53
        score = (float(d) * float(d)) / (float(w0) * float(w1))
        if score > best:
            best, best_t = score, t
    return best_t


def otsu_brute(hist):
    """Between-class variance w0 w1 (mu0 - mu1)^2 / N^2 per threshold in float64, straight from the definition: (argmax, the variances)."""
    h = np.asarray(hist, np.float64)
    v = np.arange(256, dtype=np.float64)
    var = np.full(255, -1.0)
    for t in range(255):
        w0, w1 = h[:t + 1].sum(), h[t + 1:].sum()
        if w0 == 0 or w1 == 0:
            continue
        mu0, mu1 = (v[:t + 1] * h[:t + 1]).sum() / w0, (v[t + 1:] * h[t + 1:]).sum() / w1
        var[t] = w0 * w1 * (mu0 - mu1) ** 2 / h.sum() ** 2
    return int(np.argmax(var)), var


def inverted(s, t, polarity="auto"):
    if polarity != "auto":
        return polarity == "dark"
    b = s > t
    ring = np.ones(s.shape, bool)
    ring[1:-1, 1:-1] = False
    return 2 * int(b[ring].sum()) > int(ring.sum())


def opening(b):
    h, w = b.shape
    p = np.pad(b.astype(bool), 2, constant_values=False)
    e = np.ones((h, w), bool)
    for dy in range(5):
        for dx in range(5):
            e &= p[dy:dy + h, dx:dx + w]
    p = np.pad(e, 2, constant_values=False)
    d = np.zeros((h, w), bool)
    for dy in range(5):
        for dx in range(5):
            d |= p[dy:dy + h, dx:dx + w]
    return d


def pack_bits(m):
    h, w = m.shape
    wpr = (w + 31) // 32
    p = np.zeros((h, wpr * 32), np.uint64)
    p[:, :w] = m != 0
    return (p.reshape(h, wpr, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)


def unpack_bits(bits, h, w):
    b = np.asarray(bits, np.uint32).reshape(h, (w + 31) // 32)
    return ((b[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(h, -1)[:, :w].astype(np.uint8) * 255


def stages(img, work_h=500, polarity="auto"):
    """Every intermediate of part B: grey, smooth, hist, t, inverted, mask (bool), bits."""
    g = grey(img, work_h)
    s = smooth(g)
    hist = histogram(s)
    t = otsu(hist)
    if t < 0:
        inv, m = False, np.zeros(s.shape, bool)
    else:
        inv = inverted(s, t, polarity)
        m = opening((s > t) != inv)
    return dict(grey=g, smooth=s, hist=hist, t=t, inverted=inv, mask=m, bits=pack_bits(m))


# ---------------------------------------------------------------------------------------------------- A: mask -> corners
def external_contours(mask):
    """cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE): the outer border of every 8-connected component that touches the background
    reaching the frame, last-found (largest raster index of its first pixel) first."""
    fg = np.asarray(mask) != 0
    h, w = fg.shape
    labels, n = ndimage.label(fg, structure=np.ones((3, 3), int))
    if n == 0:
        return []
    bg, _ = ndimage.label(np.pad(~fg, 1, constant_values=True))          # 4-connected background; the frame is one region
    outside = bg == bg[0, 0]
    near = (outside[1:-1, :-2] | outside[1:-1, 2:] | outside[:-2, 1:-1] | outside[2:, 1:-1])
    external = set(np.unique(labels[near & fg]).tolist())
    ids, first = np.unique(labels.reshape(-1), return_index=True)
    boxes = ndimage.find_objects(labels)
    out = []
    for k, _ in sorted(((int(k), int(f)) for k, f in zip(ids, first) if k in external), key=lambda kf: -kf[1]):
        sl = boxes[k - 1]
        outer = dbpost_cpu.find_contours(labels[sl] == k)[-1]              # the first border the scan meets is the component's outer one
        out.append(outer + np.array([sl[1].start, sl[0].start], np.int32))
    return out


def document_contour(mask):
    """-> (int32 [4, 2] or None, "polygon" / "rectangle" / None)"""
    cnts = sorted(external_contours(mask), key=dbpost_cpu.contour_area, reverse=True)[:5]
    if not cnts:
        return None, None
    for c in cnts:
        approx = dbpost_cpu.approx_poly_dp_closed(c, 0.02 * dbpost_cpu.arc_length_closed(c))
        if len(approx) == 4:
            return approx.astype(np.int32), "polygon"
    quad, _ = quad_ref.min_area_quad(cnts[0])
    return np.array([[math.trunc(v) for v in p] for p in quad.tolist()], np.int32), "rectangle"


def find_quad(img, work_h=500, polarity="auto"):
    """-> float64 [4, 2] in the page's coordinates (screen_cnt.reshape(4, 2) * ratio, scanner.py:187) or None"""
    _, ratio = working_size(img.shape[0], img.shape[1], work_h)
    q, _ = document_contour(stages(img, work_h, polarity)["mask"])
    return None if q is None else q.astype(np.float64) * ratio


# ---------------------------------------------------------------------------------------------------- scenes
def _inside(h, w, quad):
    """Pixels whose centre lies inside the convex quad (corners in order, either orientation)."""
    ys, xs = np.mgrid[0:h, 0:w]
    q = np.asarray(quad, np.float64)
    side = [(q[(i + 1) % 4][0] - q[i][0]) * (ys - q[i][1]) - (q[(i + 1) % 4][1] - q[i][1]) * (xs - q[i][0]) for i in range(4)]
    return np.logical_and.reduce([s >= 0 for s in side]) | np.logical_and.reduce([s <= 0 for s in side])


PHOTOS = {
    # name: (rows, columns, true corners (x, y), paper level, frame level, text level)
    "bright_on_dark": (1280, 960, ((140, 110), (820, 170), (860, 1150), (90, 1090)), 225, 45, 60),
    "dark_on_bright": (1100, 1000, ((200, 150), (840, 120), (900, 960), (150, 1000)), 50, 215, 140),
    "touching_edge": (1200, 900, ((0, 200), (700, 150), (760, 1080), (0, 1130)), 225, 45, 60),
}


def photo(name):
    """-> (uint8 [h, w, 3] RGB, true corners float64 [4, 2]): a noisy striped frame, a quadrilateral sheet of paper, lines of text on it."""
    h, w, quad, paper, frame, text = PHOTOS[name]
    rng = np.random.default_rng(sorted(PHOTOS).index(name) + 2200)
    ys, xs = np.mgrid[0:h, 0:w]
    img = frame + 12 * (((xs + 2 * ys) // 24) % 2) + rng.integers(-10, 11, (h, w))
    doc = _inside(h, w, quad)
    sheet = paper + rng.integers(-8, 9, (h, w))
    q = np.asarray(quad, np.float64)
    inner = q.mean(0) + (q - q.mean(0)) * 0.8
    lines = _inside(h, w, inner) & ((ys // 14) % 3 == 0) & (((xs + 5 * (ys // 42)) // 90) % 4 != 3)
    sheet = np.where(lines, text + rng.integers(-8, 9, (h, w)), sheet)
    img = np.clip(np.where(doc, sheet, img), 0, 255)
    rgb = np.stack([np.clip(img + 6, 0, 255), img, np.clip(img - 9, 0, 255)], 2).astype(np.uint8)
    return np.ascontiguousarray(rgb), q


def corner_error(found, truth):
    """The largest distance from a true corner to the nearest found corner."""
    f, t = np.asarray(found, np.float64), np.asarray(truth, np.float64)
    return float(max(np.sqrt(((f - c) ** 2).sum(1)).min() for c in t))
