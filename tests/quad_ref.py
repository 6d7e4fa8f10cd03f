"""Reference for the oriented text crops (include/ocrvi.h, "Oriented text crops"), independent of the library's C++ and kernels.

``min_area_quad`` states the minimum-area rectangle of a polygon in Python integers and ``fractions``; ``quad_crop_descriptor`` takes a quad
through ``warp_ref``'s corner order, output size and 8 x 8 system and applies the refusal rules; ``warp_replicate`` is
``warp_ref.warp_perspective`` with clamped taps; ``crop_quad_preprocess`` is ``warp_replicate`` followed by
``oracle.preproc_cpu.preprocess_for_recognition``.

The 8 x 8 system is solved here by the elimination the header names (partial pivoting, back substitution, adjugate over determinant) in
Python floats -- IEEE doubles, one rounding per operation, the order the header's description implies -- so the matrices can be compared bit for
bit.  That bit-equality holds by construction: ``solve_inverse`` follows the library's elimination step for step, so it checks the
transcription, not the matrices' correctness.  The independent check of correctness is ``numpy.linalg.solve`` on the same system
(``warp_ref.four_point_geometry``): the tests project the crop's corners through the library's matrix and compare with the ordered corners."""
import math
from fractions import Fraction

import numpy as np

import warp_ref as WR
from oracle import preproc_cpu

COORD_MIN, COORD_MAX = -32768, 32767


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(points):
    """Strictly convex hull of integer points by the monotone chain (lower chain, then upper chain), starting at the smallest (x, y)."""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) < 3:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def min_area_quad(points):
    """-> (quad float64 [4, 2], flag).  flag = 1: fewer than three hull vertices, the quad is the inclusive bounding box."""
    pts = [(int(x), int(y)) for x, y in np.asarray(points).reshape(-1, 2).tolist()]
    for x, y in pts:
        if not (COORD_MIN <= x <= COORD_MAX and COORD_MIN <= y <= COORD_MAX):
            raise ValueError(f"point ({x}, {y}) outside the coordinate range")
    hull = convex_hull(pts)
    if len(hull) < 3:
        if not pts:
            return np.zeros((4, 2)), 1
        x0, x1 = min(p[0] for p in pts), max(p[0] for p in pts)
        y0, y1 = min(p[1] for p in pts), max(p[1] for p in pts)
        return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64), 1
    best = None
    for k in range(len(hull)):
        a, b = hull[k], hull[(k + 1) % len(hull)]
        dx, dy = b[0] - a[0], b[1] - a[1]
        s = [p[0] * dx + p[1] * dy for p in hull]
        t = [p[1] * dx - p[0] * dy for p in hull]
        den = dx * dx + dy * dy
        area = Fraction((max(s) - min(s)) * (max(t) - min(t)), den)
        if best is None or area < best[0]:            # strict: the smallest k wins a tie
            best = (area, min(s), max(s), min(t), max(t), dx, dy, den)
    _, s0, s1, t0, t1, dx, dy, den = best
    quad = []
    for s, t in ((s0, t0), (s1, t0), (s1, t1), (s0, t1)):
        nx, ny = s * dx - t * dy, s * dy + t * dx
        assert abs(nx) < 2 ** 53 and abs(ny) < 2 ** 53
        quad.append([float(nx) / float(den), float(ny) / float(den)])
    return np.array(quad, np.float64), 0


def _three_collinear(p):
    for a in range(4):
        q = [p[i] for i in range(4) if i != a]
        ux, uy, vx, vy = q[1][0] - q[0][0], q[1][1] - q[0][1], q[2][0] - q[0][0], q[2][1] - q[0][1]
        cross = ux * vy - uy * vx
        if not abs(cross) > 1e-12 * math.sqrt((ux * ux + uy * uy) * (vx * vx + vy * vy)):
            return True
    return False


def solve_inverse(rect, dst):
    """m_inv [9] of the homography rect[i] -> dst[i], or None when the system is refused: Gaussian elimination with partial pivoting (the
    first largest pivot), back substitution, then the adjugate over the determinant, every step one Python float operation."""
    sp = [[float(v) for v in r] for r in np.asarray(rect, np.float64)]
    dp = [[float(v) for v in r] for r in np.asarray(dst, np.float64)]
    if _three_collinear(sp) or _three_collinear(dp):
        return None
    A, b = WR.homography_system(rect, dst)
    A = [[float(v) for v in row] + [float(bb)] for row, bb in zip(A, b)]
    for c in range(8):
        piv = c
        for r in range(c + 1, 8):
            if abs(A[r][c]) > abs(A[piv][c]):
                piv = r
        if A[piv][c] == 0.0 or not math.isfinite(A[piv][c]):
            return None
        A[c], A[piv] = A[piv], A[c]
        for r in range(c + 1, 8):
            f = A[r][c] / A[c][c]
            if f == 0.0:
                continue
            for j in range(c, 9):
                A[r][j] -= f * A[c][j]
    h = [0.0] * 9
    for r in range(7, -1, -1):
        acc = A[r][8]
        for j in range(r + 1, 8):
            acc -= A[r][j] * h[j]
        h[r] = acc / A[r][r]
        if not math.isfinite(h[r]):
            return None
    h[8] = 1.0
    m = h
    c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    det = m[0] * c00 + m[1] * c01 + m[2] * c02
    if det == 0.0 or not math.isfinite(det):
        return None
    adj = [c00, m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
           c01, m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
           c02, m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]]
    out = [v / det for v in adj]
    return np.array(out, np.float64) if all(math.isfinite(v) for v in out) else None


def fallback_descriptor(quad, page_hw, page_id=0):
    """The reference's crop as a descriptor: the bounding rectangle of the corners clamped as crop_image clamps, a pure translation."""
    q = np.asarray(quad, np.float64).reshape(4, 2)
    ph, pw = page_hw
    x0, y0 = int(math.floor(q[:, 0].min())), int(math.floor(q[:, 1].min()))
    bw, bh = int(math.ceil(q[:, 0].max())) - x0 + 1, int(math.ceil(q[:, 1].max())) - y0 + 1
    x, y = max(0, x0), max(0, y0)
    w, h = max(min(bw, pw - x), 0), max(min(bh, ph - y), 0)
    if w == 0 or h == 0:
        w = h = 0
    return (page_id, w, h, 0), np.array([1, 0, x, 0, 1, y, 0, 0, 1], np.float64)


def quad_crop_descriptor(quad, flag, page_hw, page_id=0):
    """-> ((page_id, w, h, 0), m_inv float64 [9], refused).  The four-point geometry of warp_ref on the quad, or the fallback."""
    if not flag:
        rect = WR.order_points(quad)
        w, h = WR.output_size(rect)
        if w >= 1 and h >= 1:
            m = solve_inverse(rect, WR.dst_corners(w, h))
            if m is not None:
                return (page_id, w, h, 0), m, False
    return fallback_descriptor(quad, page_hw, page_id) + (True,)


def warp_replicate(src, m_inv, dst_h, dst_w):
    """``warp_ref.warp_perspective`` with a replicate border: every tap's row and column is clamped to the page."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3
    sh, sw = src.shape[:2]
    X, Y = WR.warp_coords(m_inv, dst_h, dst_w)
    sx, sy = (X >> 5).astype(np.int64), (Y >> 5).astype(np.int64)
    ax, ay = (X & 31).astype(np.int64), (Y & 31).astype(np.int64)
    acc = np.full((dst_h, dst_w, src.shape[2]), 16384, np.int64)
    for dy, dx, wgt in ((0, 0, (32 - ax) * (32 - ay) * 32), (0, 1, ax * (32 - ay) * 32), (1, 0, (32 - ax) * ay * 32), (1, 1, ax * ay * 32)):
        ty, tx = np.clip(sy + dy, 0, sh - 1), np.clip(sx + dx, 0, sw - 1)
        acc += wgt[:, :, None] * src[ty, tx].astype(np.int64)
    return (acc >> 15).astype(np.uint8)


def crop_quad_preprocess(page, desc, m_inv, img_size=(32, 256)):
    """One output of ocrvi_crop_quad_resize_normalize: float32 [3, out_h, out_w].  ``page`` None stands for an invalid page."""
    _, w, h, _ = desc
    if page is None or w <= 0 or h <= 0:
        return np.zeros((3,) + tuple(img_size), np.float32)
    return preproc_cpu.preprocess_for_recognition(warp_replicate(page, m_inv, h, w), img_size)
