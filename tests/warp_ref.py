"""Reference for the four-point rectification (include/ocrvi.h, "Four-point page rectification"), in numpy float64 / integers.

``four_point_geometry`` restates what scanner.py:13-50 computes (corner order, output size from float32 side lengths, destination corners,
the 8 x 8 system of ``cv2.getPerspectiveTransform``) with ``numpy.linalg.solve`` / ``numpy.linalg.inv`` as the solver.
``warp_perspective`` states the library's fixed-point bilinear warp independently of the kernel: it is the definition the header gives,
vectorised over the destination grid.  numpy evaluates ``a * b + c`` as two correctly rounded operations, never as a fused multiply-add,
which is what the header asks of the kernel."""
import numpy as np


def order_points(pts):
    """Top-left, top-right, bottom-right, bottom-left as float32 [4, 2]; sums / differences in float64, first index wins ties."""
    pts = np.asarray(pts, np.float64).reshape(4, 2)
    s = pts[:, 0] + pts[:, 1]
    d = pts[:, 1] - pts[:, 0]
    idx = [int(np.argmin(s)), int(np.argmin(d)), int(np.argmax(s)), int(np.argmax(d))]
    return pts[idx].astype(np.float32)


def output_size(rect):
    """(out_w, out_h) from the float32 corners: every step of a side length stays float32, each length is truncated."""
    rect = np.asarray(rect, np.float32)
    tl, tr, br, bl = rect

    def side(a, b):
        dx, dy = np.float32(a[0] - b[0]), np.float32(a[1] - b[1])
        return int(np.sqrt(np.float32(np.float32(dx * dx) + np.float32(dy * dy))))

    return max(side(tr, tl), side(br, bl)), max(side(tl, bl), side(tr, br))


def dst_corners(w, h):
    return np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float32)


def homography_system(src, dst):
    """The 8 x 8 matrix and right-hand side of the four correspondences src[i] -> dst[i] with h22 = 1 (unknowns h00 .. h21)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        x, y = src[i]
        u, v = dst[i]
        A[i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[i + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[i], b[i + 4] = u, v
    return A, b


def four_point_geometry(pts):
    """-> (rect float32 [4,2], dst float32 [4,2], out_w, out_h, m_fwd [3,3], m_inv [3,3]) with numpy's solver."""
    rect = order_points(pts)
    w, h = output_size(rect)
    dst = dst_corners(w, h)
    A, b = homography_system(rect, dst)
    m_fwd = np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)
    return rect, dst, w, h, m_fwd, np.linalg.inv(m_fwd)


def project(m, pts):
    """The 3 x 3 map m applied to points [n, 2] -> [n, 2] (float64)."""
    m = np.asarray(m, np.float64).reshape(3, 3)
    p = np.concatenate([np.asarray(pts, np.float64), np.ones((len(pts), 1))], 1) @ m.T
    return p[:, :2] / p[:, 2:3]


def warp_coords(m_inv, dst_h, dst_w):
    """(X, Y) int32 [dst_h, dst_w]: the source coordinates in 1/32 pixel."""
    m = np.asarray(m_inv, np.float64).reshape(9)
    x = np.arange(dst_w, dtype=np.float64)[None, :]
    y = np.arange(dst_h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X0 = (m[0] * x + m[1] * y) + m[2]
        Y0 = (m[3] * x + m[4] * y) + m[5]
        W0 = (m[6] * x + m[7] * y) + m[8]
        s = np.where(W0 != 0, 32.0 / np.where(W0 != 0, W0, 1.0), 0.0)

        def fix(v0):
            v = v0 * s
            v = np.where(np.isnan(v), -2147483648.0, v)          # a NaN product counts as the lower bound
            return np.rint(np.clip(v, -2147483648.0, 2147483647.0)).astype(np.int64).astype(np.int32)

        return fix(X0), fix(Y0)


def warp_perspective(src, m_inv, dst_h, dst_w):
    """uint8 [src_h, src_w, 3] -> uint8 [dst_h, dst_w, 3]; 1/32-pixel coordinates, 15-bit weights, constant border 0."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 3
    sh, sw = src.shape[:2]
    X, Y = warp_coords(m_inv, dst_h, dst_w)
    sx, sy = (X >> 5).astype(np.int64), (Y >> 5).astype(np.int64)      # arithmetic shifts
    ax, ay = (X & 31).astype(np.int64), (Y & 31).astype(np.int64)
    acc = np.full((dst_h, dst_w, src.shape[2]), 16384, np.int64)
    for dy, dx, wgt in ((0, 0, (32 - ax) * (32 - ay) * 32), (0, 1, ax * (32 - ay) * 32), (1, 0, (32 - ax) * ay * 32), (1, 1, ax * ay * 32)):
        ty, tx = sy + dy, sx + dx
        inside = (ty >= 0) & (ty < sh) & (tx >= 0) & (tx < sw)
        tap = src[np.where(inside, ty, 0), np.where(inside, tx, 0)].astype(np.int64)
        acc += np.where(inside, wgt, 0)[:, :, None] * tap
    return (acc >> 15).astype(np.uint8)
