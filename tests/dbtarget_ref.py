"""Test infrastructure: an independent Python statement of the reference's detection dataloader without augmentation
(src/det/dataloader.py:27-362) -- what ``ocrvi_db_target_jobs``, ``ocrvi_db_target_maps``, ``ocrvi_resize_normalize_pad_pages`` and
``ocr_vi_invoice_amd.data.DetectionDataset`` must equal exactly.

shapely, pyclipper and cv2 are absent here, so each of their calls is restated as include/ocrvi.h ("DB ground truth") states it:
``is_valid`` / ``area`` / ``length`` on the float ring in double; ``Execute(-d)`` as the raw round-join offset path followed by EVERY outer
loop of its positive-winding region (the multi-loop union is restated below from the arrangement helpers of ``oracle.dbpost_cpu``);
``cv2.fillPoly`` as ``oracle.dbpost_cpu.polygon_mask``; ``cv2.resize(INTER_NEAREST)`` as ``sx = min(floor(X * (1 / (new_w / w))), w - 1)``;
``cv2.resize`` of the image as ``oracle.preproc_cpu.resize_linear_u8``.  Unlike the library, the maps are filled at full resolution and
then sampled, as the reference does."""
from __future__ import annotations

import functools
import math
from fractions import Fraction as Fr
from typing import List, Optional, Tuple

import numpy as np

from oracle import dbpost_cpu as O
from oracle.preproc_cpu import resize_linear_u8

GT, MASK, THRESH = 0, 1, 2
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ the union with every loop
def union_boundary_loops(path) -> List[List[Tuple[int, int]]]:
    """Every boundary loop (interior on the left, crossings rounded as Clipper rounds them, before FixupOutPolygon) of the region of one
    closed integer path whose winding number is positive.  The arrangement is ``oracle.dbpost_cpu.clipper_union_outline``'s; that one
    keeps the loop through the left-most vertex only."""
    P = O._addpath_cleanup(path)
    n = len(P)
    if n < 3:
        return []
    seg = [(P[i], P[(i + 1) % n]) for i in range(n)]
    cuts = [[Fr(0), Fr(1)] for _ in range(n)]
    for i in range(n):
        (ax, ay), (bx, by) = seg[i]
        rx, ry = bx - ax, by - ay
        for j in range(i + 1, n):
            (cx, cy), (ex, ey) = seg[j]
            if max(ax, bx) < min(cx, ex) or max(cx, ex) < min(ax, bx) or max(ay, by) < min(cy, ey) or max(cy, ey) < min(ay, by):
                continue
            sx, sy = ex - cx, ey - cy
            wx, wy = cx - ax, cy - ay
            d = rx * sy - ry * sx
            if d != 0:
                t, u = wx * sy - wy * sx, wx * ry - wy * rx
                if d < 0:
                    d, t, u = -d, -t, -u
                if 0 <= t <= d and 0 <= u <= d:
                    cuts[i].append(Fr(t, d))
                    cuts[j].append(Fr(u, d))
            elif wx * ry - wy * rx == 0:
                rr, ss = rx * rx + ry * ry, sx * sx + sy * sy
                for (qx, qy) in seg[j]:
                    t = (qx - ax) * rx + (qy - ay) * ry
                    if 0 <= t <= rr:
                        cuts[i].append(Fr(t, rr))
                for (qx, qy) in seg[i]:
                    u = (qx - cx) * sx + (qy - cy) * sy
                    if 0 <= u <= ss:
                        cuts[j].append(Fr(u, ss))
    vid, vpt = {}, []

    def vertex(x, y):
        if (x, y) not in vid:
            vid[(x, y)] = len(vpt)
            vpt.append((x, y))
        return vid[(x, y)]

    mult, edir, eseg = {}, {}, {}
    for i in range(n):
        (ax, ay), (bx, by) = seg[i]
        rx, ry = bx - ax, by - ay
        ids = [vertex(ax + t * rx, ay + t * ry) for t in sorted(set(cuts[i]))]
        for u, v in zip(ids[:-1], ids[1:]):
            if u == v:
                continue
            mult[(u, v)] = mult.get((u, v), 0) + 1
            mult.setdefault((v, u), 0)
            edir[(u, v)], edir[(v, u)] = (rx, ry), (-rx, -ry)
            eseg.setdefault((u, v), i)
            eseg.setdefault((v, u), i)
    out_edges = {}
    for (u, v) in mult:
        out_edges.setdefault(u, []).append(v)

    def angle_key(u):
        def cmp(v1, v2):                                     # counter-clockwise from the +x axis, exact
            (x1, y1), (x2, y2) = edir[(u, v1)], edir[(u, v2)]
            h1 = 0 if (y1 > 0 or (y1 == 0 and x1 > 0)) else 1
            h2 = 0 if (y2 > 0 or (y2 == 0 and x2 > 0)) else 1
            if h1 != h2:
                return h1 - h2
            c = x1 * y2 - y1 * x2
            return -1 if c > 0 else (1 if c < 0 else 0)
        return functools.cmp_to_key(cmp)

    pos = {}
    for u, vs in out_edges.items():
        vs.sort(key=angle_key(u))
        for k, v in enumerate(vs):
            pos[(u, v)] = k
    face_of, faces = {}, []
    for h in mult:
        if h in face_of:
            continue
        cyc, g = [], h
        while g not in face_of:
            face_of[g] = len(faces)
            cyc.append(g)
            u, v = g
            vs = out_edges[v]
            g = (v, vs[(pos[(v, u)] - 1) % len(vs)])
        faces.append(cyc)
    u0 = min(range(len(vpt)), key=lambda i: vpt[i])
    v0 = out_edges[u0][0]
    for v in out_edges[u0][1:]:
        (x1, y1), (x2, y2) = edir[(u0, v0)], edir[(u0, v)]
        if x1 * y2 - y1 * x2 > 0:
            v0 = v
    outer = face_of[(u0, v0)]
    wind, stack = {outer: 0}, [outer]
    while stack:
        f = stack.pop()
        for (u, v) in faces[f]:
            g = face_of[(v, u)]
            if g not in wind:
                wind[g] = wind[f] - (mult[(u, v)] - mult[(v, u)])
                stack.append(g)
    is_b = {h: (wind[face_of[h]] >= 1 and wind[face_of[(h[1], h[0])]] <= 0) for h in mult}
    loops, seen = [], set()
    for h0 in mult:
        if not is_b[h0] or h0 in seen:
            continue
        loop, g = [], h0
        while g not in seen:
            seen.add(g)
            loop.append(g)
            u, v = g
            vs = out_edges[v]
            k = pos[(v, u)]
            for s in range(1, len(vs) + 1):
                cand = (v, vs[(k + s) % len(vs)])
                if is_b[cand]:
                    g = cand
                    break
        outline = []
        for k, (u, v) in enumerate(loop):
            x, y = vpt[u]
            if x.denominator == 1 and y.denominator == 1:
                outline.append((int(x), int(y)))
            else:
                outline.append(O._clipper_intersect_point(seg[eseg[loop[k - 1]]], seg[eseg[(u, v)]]))
        loops.append(outline)
    return loops


def area2(poly) -> int:
    n = len(poly)
    return sum(poly[i][0] * poly[(i + 1) % n][1] - poly[(i + 1) % n][0] * poly[i][1] for i in range(n))


def union_outer_loops(path) -> List[List[Tuple[int, int]]]:
    """What Execute(-d)'s closing union leaves of the raw path: every outer loop (positive area after FixupOutPolygon)."""
    out = []
    for outline in union_boundary_loops(path):
        poly = O._fixup_and_emit(outline)
        if len(poly) >= 3 and area2(poly) > 0:
            out.append(poly)
    return out


def pick_largest(loops) -> Optional[int]:
    """max(paths, key=pyclipper.Area) with the tie rule of include/ocrvi.h: the largest signed area; among equals the loop whose smallest
    vertex (by x, then y) is smallest; among those the first found."""
    best = None
    for k, lp in enumerate(loops):
        key = (-area2(lp), min(lp))
        if best is None or key < best[0]:
            best = (key, k)
    return None if best is None else best[1]


def shrink_loops(poly_int, d: float):
    raw = O.clipper_offset_round(np.asarray(poly_int, dtype=np.int64).reshape(-1, 2), -d)
    return union_outer_loops([tuple(p) for p in raw.tolist()])


def dilate(poly_int, d: float):
    raw = O.clipper_offset_round(np.asarray(poly_int, dtype=np.int64).reshape(-1, 2), d)
    return O.clipper_union_outline([tuple(p) for p in raw.tolist()])


# ------------------------------------------------------------------------------------------------ shapely's three numbers
def _orient(a, b, c) -> int:
    l, r = (b[0] - a[0]) * (c[1] - a[1]), (b[1] - a[1]) * (c[0] - a[0])
    v = l - r
    return 1 if v > 0 else (-1 if v < 0 else 0)


def _in_box(a, b, p) -> bool:
    return min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def _segments_meet(a, b, c, e) -> bool:
    o1, o2, o3, o4 = _orient(a, b, c), _orient(a, b, e), _orient(c, e, a), _orient(c, e, b)
    if o1 * o2 < 0 and o3 * o4 < 0:
        return True
    return (o1 == 0 and _in_box(a, b, c)) or (o2 == 0 and _in_box(a, b, e)) or (o3 == 0 and _in_box(c, e, a)) or (o4 == 0 and _in_box(c, e, b))


def ring_is_simple(ring) -> bool:
    q = []
    for p in ring:
        if not q or p != q[-1]:
            q.append(p)
    if len(q) > 1 and q[-1] == q[0]:
        q.pop()
    m = len(q)
    if m < 3:
        return False
    for i in range(m):
        a, b = q[i], q[(i + 1) % m]
        for j in range(i + 1, m):
            c, e = q[j], q[(j + 1) % m]
            nxt, wrap = j == i + 1, (i == 0 and j == m - 1)
            if nxt or wrap:
                s, p, r = (b, a, e) if nxt else (a, b, c)
                if _orient(p, s, r) == 0 and (p[0] - s[0]) * (r[0] - s[0]) + (p[1] - s[1]) * (r[1] - s[1]) > 0:
                    return False
            elif _segments_meet(a, b, c, e):
                return False
    return True


def ring_area_length(ring) -> Tuple[float, float]:
    n = len(ring)
    a2, length = 0.0, 0.0
    for i in range(n):
        (ax, ay), (bx, by) = ring[i], ring[(i + 1) % n]
        a2 += ax * by - bx * ay
        dx, dy = bx - ax, by - ay
        length += math.sqrt(dx * dx + dy * dy)
    return abs(a2) * 0.5, length


# ------------------------------------------------------------------------------------------------ the polygon loop
def polygon_jobs(h: int, w: int, polygons, shrink_ratio: float = 0.4, want_thresh: bool = False):
    """dataloader.py:334-350 -> [(kind, [(x, y), ...]), ...] in the reference's order."""
    jobs = []
    for poly in polygons:
        poly = np.array(poly, dtype=np.float32).reshape(-1, 2)
        if len(poly) < 3:
            continue
        poly[:, 0] = np.clip(poly[:, 0], 0, w - 1)
        poly[:, 1] = np.clip(poly[:, 1], 0, h - 1)
        ring = [(float(x), float(y)) for x, y in poly]
        trunc = [(int(x), int(y)) for x, y in poly.astype(int)]
        ok = ring_is_simple(ring)
        d = 0.0
        if ok:
            area, length = ring_area_length(ring)
            ok = not (area < 1) and not (length < 1)
        if ok:
            d = area * (1 - shrink_ratio ** 2) / length
        pick = None
        if ok:
            loops = shrink_loops(trunc, d)
            pick = pick_largest(loops)
        jobs.append((GT, loops[pick]) if pick is not None else (MASK, trunc))
        if want_thresh and ok and d >= 1:
            dil = dilate(trunc, d)
            if dil:
                jobs.append((THRESH, dil))
    return jobs


# ------------------------------------------------------------------------------------------------ the maps and the image
def resize_sizes(h: int, w: int, S: int):
    scale = S / max(h, w)
    return scale, int(h * scale), int(w * scale)


def nearest_resize(m: np.ndarray, new_w: int, new_h: int) -> np.ndarray:
    h, w = m.shape
    ifx, ify = 1.0 / (new_w / w), 1.0 / (new_h / h)
    xs = [min(int(math.floor(X * ifx)), w - 1) for X in range(new_w)]
    ys = [min(int(math.floor(Y * ify)), h - 1) for Y in range(new_h)]
    return m[np.ix_(ys, xs)]


def blank_sample(S: int):
    return {"image": np.zeros((3, S, S), np.float32), **{k: np.zeros((1, S, S), np.float32) for k in ("gt", "mask", "thresh_map", "thresh_mask")}}


def load_sample(image: np.ndarray, polygons, S: int, shrink_ratio: float = 0.4, thresh_max: float = 0.7, want_thresh: bool = False):
    """_load_sample + _resize_pad for a uint8 HxWx3 image -> dict of float32 arrays ([3,S,S] and four [1,S,S])."""
    h, w = image.shape[:2]
    scale, new_h, new_w = resize_sizes(h, w, S)
    if new_h <= 0 or new_w <= 0:          # cv2.resize raises -> __getitem__ returns _blank_sample()
        return blank_sample(S)
    gt, mask = np.zeros((h, w), np.float32), np.ones((h, w), np.float32)
    tmap, tmask = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    for kind, pts in polygon_jobs(h, w, polygons, shrink_ratio, want_thresh):
        fill = O.polygon_mask(np.asarray(pts, dtype=np.int64), h, w).astype(bool)
        if kind == GT:
            gt[fill] = 1.0
        elif kind == MASK:
            mask[fill] = 0.0
        else:
            tmask[fill] = 1.0
            tmap[fill] = np.float32(thresh_max)
    img = image if scale == 1.0 else resize_linear_u8(image, (new_w, new_h))
    f = img.astype(np.float32) / np.float32(255.0)
    f = ((f - MEAN) / STD).astype(np.float32).transpose(2, 0, 1)
    out = {"image": np.zeros((3, S, S), np.float32)}
    out["image"][:, :new_h, :new_w] = f
    for name, m in (("gt", gt), ("mask", mask), ("thresh_map", tmap), ("thresh_mask", tmask)):
        if scale != 1.0:
            m = nearest_resize(m, new_w, new_h)
        full = np.zeros((1, S, S), np.float32)
        full[0, :new_h, :new_w] = m
        out[name] = full
    return out


def same_cycle(a, b) -> bool:
    """Equal as cyclic vertex sequences (same orientation)."""
    a, b = [tuple(p) for p in a], [tuple(p) for p in b]
    if len(a) != len(b):
        return False
    if not a:
        return True
    return any(a == b[k:] + b[:k] for k in range(len(b)) if b[k] == a[0])
