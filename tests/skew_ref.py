"""Reference for the skew estimate (include/ocrvi.h, "Skew estimate"), independent of the library's C++ and kernels: every stage in numpy
integers (``edges``, ``offsets``, ``profile``, ``scores``), the host half (``pick``, ``quad``) in Python floats in the header's order, and
``estimate`` from a page.  The grey stage is ``docfind_ref.grey``.

``profile`` uses that o(j, k) is monotone in j: the columns of equal offset are summed first (``np.add.reduceat``), then every such sum is
binned once.  ``profile_brute`` is the definition pixel by pixel, for small images.  ``MUTANTS`` are wrong readings of the definition;
``scores(..., mutant=name)`` / ``edges(..., mutant=name)`` compute them, and tests/test_skew_cpu.py checks that each one shows on the inputs
the GPU tests use (``score_cases``, ``grey_cases``).

``rotated`` turns a page by an angle with tests/warp_ref.py's fixed-point warp."""
import math
from typing import NamedTuple

import numpy as np

import docfind_ref as DR
import warp_ref

K, SHIFT, FLOOR, ANGLES = 128, 9, 8, 257
MUTANTS = ("shift_toward_zero", "centre_ww_minus_1", "floor_dropped", "border_wrapped", "offset_sign", "square_in_32_bits")


class Skew(NamedTuple):
    k: int
    angle: float
    gain: float


# ---------------------------------------------------------------------------------------------------- stages
def edges(g, mutant=None):
    g = np.asarray(g).astype(np.int64)
    if mutant == "border_wrapped":
        d = np.abs(np.roll(g, -1, 1) - np.roll(g, 1, 1))
    else:
        p = np.pad(g, ((0, 0), (1, 1)), mode="edge")
        d = np.abs(p[:, 2:] - p[:, :-2])
    return (d if mutant == "floor_dropped" else np.where(d >= FLOOR, d, 0)).astype(np.uint8)


def offsets(ww, k, mutant=None):
    cj = (ww - 1) >> 1 if mutant == "centre_ww_minus_1" else ww >> 1
    v = (np.arange(ww, dtype=np.int64) - cj) * k + (1 << (SHIFT - 1))
    o = np.sign(v) * (np.abs(v) >> SHIFT) if mutant == "shift_toward_zero" else v >> SHIFT
    return -o if mutant == "offset_sign" else o


def profile(E, k, mutant=None):
    """(r_min, P int64): P[r - r_min] = the sum of E[i][j] over i - o(j, k) == r."""
    E = np.asarray(E)
    h, ww = E.shape
    o = offsets(ww, k, mutant)
    starts = np.concatenate([[0], np.nonzero(np.diff(o))[0] + 1])
    seg = np.add.reduceat(E.astype(np.int64), starts, axis=1)                # [h, segments]: the columns of one offset
    r = np.arange(h, dtype=np.int64)[:, None] - o[starts][None, :]
    r_min = int(r.min())
    P = np.bincount((r - r_min).reshape(-1), weights=seg.reshape(-1).astype(np.float64))     # sums below 2^53: exact
    return r_min, P.astype(np.int64)


def profile_brute(E, k):
    """The definition, pixel by pixel: {r: P[r]}."""
    E = np.asarray(E)
    h, ww = E.shape
    P = {}
    for j in range(ww):
        o = ((j - (ww >> 1)) * k + 256) >> 9                              # Python's >> floors
        for i in range(h):
            P[i - o] = P.get(i - o, 0) + int(E[i, j])
    return P


def scores(E, mutant=None):
    """uint64 [257]: scores[k + K] = S_k, exact."""
    out = np.zeros(ANGLES, np.uint64)
    for k in range(-K, K + 1):
        _, P = profile(E, k, mutant)
        sq = P.astype(np.uint64) * P.astype(np.uint64)                       # < 2^43 each, the sum < 2^54: no wrap
        if mutant == "square_in_32_bits":
            sq &= np.uint64(0xFFFFFFFF)
        out[k + K] = sq.sum(dtype=np.uint64)
    return out


def scores_constant(h, ww, v):
    """``scores`` of an h x ww image of the constant v in closed form: P_k[r] = v * #{j : 0 <= r + o(j, k) < h}."""
    out = np.zeros(ANGLES, np.uint64)
    for k in range(-K, K + 1):
        o = offsets(ww, k)
        P = np.convolve(np.bincount(o - o.min()), np.ones(h, np.int64)) * int(v)
        out[k + K] = sum(int(p) * int(p) for p in P)
    return out


# ---------------------------------------------------------------------------------------------------- host half
def pick(sc):
    s = [int(v) for v in sc]
    assert len(s) == ANGLES
    best = max(s)
    k = min((k for k in range(-K, K + 1) if s[k + K] == best), key=lambda k: (abs(k), -k))
    gain = float(best) / float(s[K]) if s[K] else (math.inf if best else 1.0)
    return Skew(k, math.atan(k / 512.0) * 180 / math.pi, gain)


def quad(h, w, k):
    """float64 [4, 2]; Python evaluates every product and sum as its own rounded operation."""
    t = k / 512.0
    c = 1 / math.sqrt(1 + t * t)
    s = t * c
    cx, cy = (w - 1) / 2, (h - 1) / 2
    ab = []
    for x, y in ((0, 0), (w, 0), (w, h), (0, h)):
        dx, dy = x - cx, y - cy
        ab.append((dx * c + dy * s, dy * c - dx * s))
    a0, a1 = min(a for a, _ in ab), max(a for a, _ in ab)
    b0, b1 = min(b for _, b in ab), max(b for _, b in ab)
    return np.array([[cx + a * c - b * s, cy + a * s + b * c] for a, b in ((a0, b0), (a1, b0), (a1, b1), (a0, b1))], np.float64)


def estimate(img, work_h=500):
    """Skew of a page (uint8 [h, w, 3]), or None outside the bounds of the working size."""
    try:
        g = DR.grey(img, work_h)
    except ValueError:
        return None
    return pick(scores(edges(g)))


# ---------------------------------------------------------------------------------------------------- pages and inputs
def rotated(img, degrees, enclose=True):
    """The page turned about its centre so that its text lines get the image slope tan(degrees), y pointing down: on the enclosing canvas
    (0 outside the page) or cropped to the page's own size.  The three channels of the synthetic pages are equal: one is warped."""
    h, w = img.shape[:2]
    th = math.radians(degrees)
    c, s = math.cos(th), math.sin(th)
    oh, ow = (int(math.ceil(w * abs(s) + h * abs(c))), int(math.ceil(w * abs(c) + h * abs(s)))) if enclose else (h, w)
    sx, sy, dx, dy = (w - 1) / 2, (h - 1) / 2, (ow - 1) / 2, (oh - 1) / 2
    m_inv = [c, s, sx - c * dx - s * dy, -s, c, sy + s * dx - c * dy, 0.0, 0.0, 1.0]      # destination -> source
    assert np.array_equal(img[:, :, 0], img[:, :, 1]) and np.array_equal(img[:, :, 0], img[:, :, 2])
    return np.ascontiguousarray(warp_ref.warp_perspective(img[:, :, :1], m_inv, oh, ow).repeat(3, axis=2))


def grey_cases():
    """The grey images of the GPU edge test, 8 x 8, 37 x 101 and 64 x 257: even rows step by 7, 8 or 9 every two columns, so that every
    interior difference sits at the floor or one beside it; odd rows are noise; the outermost columns differ from their neighbours."""
    out = []
    for seed, (h, ww) in enumerate(((8, 8), (37, 101), (64, 257))):
        rng = np.random.default_rng(3000 + seed)
        g = rng.integers(0, 256, (h, ww))
        step = np.array([7, 8, 9])[np.arange(h) % 3][:, None] * ((np.arange(ww) // 2) % 2)[None, :]
        g[0::2] = (rng.integers(20, 200, (h, 1)) + step)[0::2]
        g[:, 0] = rng.integers(0, 256, h)
        g[:, -1] = rng.integers(0, 256, h)
        out.append(g.astype(np.uint8))
    return out


def score_cases():
    """name -> edge image (any bytes) of the GPU score test, small ones first."""
    rng = np.random.default_rng(3100)
    return {
        "random_8x8": rng.integers(0, 256, (8, 8), dtype=np.uint8),
        "random_512x8": rng.integers(0, 256, (512, 8), dtype=np.uint8),
        "random_37x101": rng.integers(0, 256, (37, 101), dtype=np.uint8),
        "random_64x8192": rng.integers(0, 256, (64, 8192), dtype=np.uint8),      # 4160 bins: several per thread, many column tiles
        "all_255_512x8192": np.full((512, 8192), 255, np.uint8),                   # P^2 needs 64 bits
    }
