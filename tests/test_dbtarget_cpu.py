"""Host geometry of the DB ground-truth maps (csrc/db_target_geom.h, ``ocrvi_db_target_jobs``) against the Python statement in
tests/dbtarget_ref.py: hand-derived cases, then job-for-job equality on seeded polygon families, the overflow report, the header and
the exports.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import dbtarget_ref as R
from oracle.dbpost_cpu import polygon_mask
from ocr_vi_invoice_amd import _lib, data

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SQUARE = [(0, 0), (100, 0), (100, 100), (0, 100)]
STRIP = [(0, 0), (100, 0), (100, 6), (0, 6)]
# two 40 x 40 squares joined by a neck 20 long and 4 wide
DUMBBELL = [(0, 0), (40, 0), (40, 18), (60, 18), (60, 0), (100, 0), (100, 40), (60, 40), (60, 22), (40, 22), (40, 40), (0, 40)]


def c_jobs(h, w, polys, r=0.4, thresh=True, **kw):
    jobs, pts = data.target_jobs([(h, w)], [[np.asarray(p, np.float32) for p in polys]], r, thresh, **kw)
    return [(int(j[1]), [tuple(p) for p in pts[j[2]:j[3]].tolist()]) for j in jobs]


def both(h, w, polys, r=0.4, thresh=True):
    """The C entry's jobs, after checking them against the Python statement job for job (each cycle up to rotation)."""
    ref, got = R.polygon_jobs(h, w, polys, r, thresh), c_jobs(h, w, polys, r, thresh)
    assert [k for k, _ in got] == [k for k, _ in ref]
    for (_, a), (_, b) in zip(ref, got):
        assert R.same_cycle(a, b), (a, b)
    return got


# ------------------------------------------------------------------------------------------------ hand-derived cases
def test_square_shrinks_to_the_inner_square():
    # area 10000, perimeter 400, r = 0.4: d = 10000 * 0.84 / 400 = 21; a convex corner shrinks to the crossing of its two offset edges
    loops = R.shrink_loops(SQUARE, 21.0)
    assert len(loops) == 1 and R.same_cycle(loops[0], [(21, 21), (79, 21), (79, 79), (21, 79)])
    assert int(polygon_mask(np.array(loops[0]), 120, 120).sum()) == 59 * 59 == 3481
    got = both(200, 200, [SQUARE], thresh=False)
    assert got[0][0] == R.GT and R.same_cycle(got[0][1], [(21, 21), (79, 21), (79, 79), (21, 79)]) and len(got) == 1


def test_strip_thinner_than_twice_the_offset_vanishes():
    assert R.shrink_loops(STRIP, 5.0) == []            # 6 wide, 5 taken off either side: the offset path winds negatively everywhere
    # a 100 x 2 strip through the entry: area 200, perimeter 204, d = 0.82 rounds to 1 off either side -> nothing left -> ignored region
    thin = [(10, 10), (110, 10), (110, 12), (10, 12)]
    assert both(200, 200, [thin], thresh=False) == [(R.MASK, thin)]


def test_dumbbell_falls_apart_into_both_lobes():
    loops = R.shrink_loops(DUMBBELL, 5.0)              # the neck (4 wide) goes, each 40 x 40 lobe keeps its inner 30 x 30
    assert len(loops) == 2
    fills = [polygon_mask(np.array(lp), 50, 110).astype(bool) for lp in loops]
    left, right = (fills[0], fills[1]) if fills[0][20, 20] else (fills[1], fills[0])
    assert left[5:36, 5:36].all() and not left[:, 37:].any() and not left[:4].any() and not left[:, :4].any()
    assert right[5:36, 65:96].all() and not right[:, :64].any() and not right[36:].any()
    assert R.area2(loops[0]) == R.area2(loops[1])      # mirror images: a tie on the area
    pick = loops[R.pick_largest(loops)]
    assert min(pick) == (5, 5)                         # the rule: the loop whose smallest vertex (x, then y) is smallest -- the left lobe
    assert R.pick_largest(loops[::-1]) == 1            # ... whatever the order they were found in


def test_dumbbell_through_the_entry_keeps_the_left_lobe():
    # r = 0.4: area 3280, perimeter 352, d = 7.83: both lobes survive (40 - 2 * 7.83 > 0), the neck does not
    assert len(R.shrink_loops(DUMBBELL, 3280 * 0.84 / 352)) == 2
    got = both(120, 120, [DUMBBELL])
    assert [k for k, _ in got] == [R.GT, R.THRESH]
    xs = [x for x, _ in got[0][1]]
    assert min(xs) == 8 and max(xs) <= 40              # the left lobe, 8 = round(7.83) in from the edge


def test_bow_tie_is_invalid_and_becomes_an_ignore_region():
    bow = [(0, 0), (10, 10), (10, 0), (0, 10)]
    assert not R.ring_is_simple([(float(x), float(y)) for x, y in bow])
    assert both(50, 50, [bow]) == [(R.MASK, bow)]      # no THRESH job either: _draw_border_map returns on `not poly.is_valid`


def test_sliver_below_one_pixel_of_area_is_ignored():
    sliver = [(0, 0), (50, 0), (50, 0.01)]             # area 0.25
    assert R.ring_area_length([(0.0, 0.0), (50.0, 0.0), (50.0, float(np.float32(0.01)))])[0] < 1
    assert both(60, 60, [sliver]) == [(R.MASK, [(0, 0), (50, 0), (50, 0)])]


def test_polygon_half_outside_the_image_is_clipped_first():
    # x clipped to 59, y to 0: the 30 x 41 rectangle (30,0)-(59,40) is what is shrunk: area 1160, perimeter 138, d = 7.06
    got = both(60, 60, [[(30, -20), (90, -20), (90, 40), (30, 40)]])
    assert got[0][0] == R.GT and R.same_cycle(got[0][1], [(37, 7), (52, 7), (52, 33), (37, 33)])
    assert got[1][0] == R.THRESH and min(y for _, y in got[1][1]) == -7 and max(x for x, _ in got[1][1]) == 66   # dilated past the border


def test_offset_below_one_pixel_gives_no_threshold_job():
    # 30 x 2: area 60, perimeter 64, d = 0.79 < 1 (dataloader.py:160); the same box 30 x 6 has d = 2.1
    assert [k for k, _ in both(80, 80, [[(10, 10), (40, 10), (40, 12), (10, 12)]])] == [R.MASK]
    assert [k for k, _ in both(80, 80, [[(10, 10), (40, 10), (40, 16), (10, 16)]])] == [R.GT, R.THRESH]
    assert [k for k, _ in both(80, 80, [[(10, 10), (40, 10), (40, 16), (10, 16)]], thresh=False)] == [R.GT]


def test_neighbouring_edges_that_fold_back_are_invalid():
    spike = [(0.0, 0.0), (20.0, 0.0), (10.0, 0.0), (10.0, 10.0)]      # the second edge runs back along the first
    assert not R.ring_is_simple(spike)
    assert [k for k, _ in both(40, 40, [spike])] == [R.MASK]
    assert R.ring_is_simple([(0.0, 0.0), (20.0, 0.0), (20.0, 0.0), (10.0, 10.0)])   # a repeated vertex is dropped, not a fault


# ------------------------------------------------------------------------------------------------ seeded families
H, W = 160, 200


def _rot(pts, ang, cx, cy):
    c, s = math.cos(ang), math.sin(ang)
    return [(cx + x * c - y * s, cy + x * s + y * c) for x, y in pts]


def families(seed, count):
    """`count` polygons of each family, as float32 (k, 2) arrays"""
    rng = np.random.default_rng(seed)
    out = {k: [] for k in ("convex", "star", "fractional_duplicates", "strip", "dumbbell", "bow_tie", "out_of_range")}
    for _ in range(count):
        n = int(rng.integers(3, 13))
        cx, cy = rng.uniform(30, W - 30), rng.uniform(30, H - 30)
        ang = np.sort(rng.uniform(0, 2 * math.pi, n))
        rx, ry = rng.uniform(4, 40, 2)
        out["convex"].append([(cx + rx * math.cos(a), cy + ry * math.sin(a)) for a in ang])
        rad = rng.uniform(3, 40, n)
        out["star"].append([(round(cx + r * math.cos(a)), round(cy + r * math.sin(a))) for a, r in zip(ang, rad)])
        base = [(round(4 * (cx + r * math.cos(a))) / 4, round(4 * (cy + r * math.sin(a))) / 4) for a, r in zip(ang, rad)]
        k = int(rng.integers(0, n))
        out["fractional_duplicates"].append(base[:k + 1] + [base[k]] * int(rng.integers(1, 3)) + base[k + 1:] + ([base[0]] if rng.random() < 0.5 else []))
        ln, wd = rng.uniform(20, 150), rng.uniform(0.5, 7)
        out["strip"].append(_rot([(-ln / 2, -wd / 2), (ln / 2, -wd / 2), (ln / 2, wd / 2), (-ln / 2, wd / 2)], rng.uniform(0, math.pi), cx, cy))
        a, nk, nw = int(rng.integers(10, 40)), int(rng.integers(4, 30)), int(rng.integers(1, 8))
        y0, y1 = (a - nw) // 2, (a - nw) // 2 + nw
        db = [(0, 0), (a, 0), (a, y0), (a + nk, y0), (a + nk, 0), (2 * a + nk, 0), (2 * a + nk, a), (a + nk, a), (a + nk, y1), (a, y1), (a, a), (0, a)]
        ox, oy = rng.uniform(0, W - (2 * a + nk)), rng.uniform(0, H - a)
        out["dumbbell"].append([(x + ox, y + oy) for x, y in db] if rng.random() < 0.5 else _rot([(x - a, y - a / 2) for x, y in db], rng.uniform(0, math.pi), cx, cy))
        bw, bh = rng.uniform(2, 60, 2)
        out["bow_tie"].append(_rot([(-bw, -bh), (bw, bh), (bw, -bh), (-bw, bh)], rng.uniform(0, math.pi), cx, cy))
        ex, ey = rng.choice([-40.0, 0.0, 60.0]), rng.choice([-50.0, 0.0, 70.0])
        out["out_of_range"].append([(cx + ex + 3 * r * math.cos(a), cy + ey + 3 * r * math.sin(a)) for a, r in zip(ang, rad)])
    return {k: [np.asarray(p, np.float32) for p in v] for k, v in out.items()}


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_entry_equals_the_python_statement_on_seeded_families(seed):
    """4 seeds x 7 families x 75 polygons = 2100; each family is one image of a batch, so the entry's thread pool and its concatenation
    of per-image results are exercised too.  Every polygon yields a GT or a MASK job in both, so none can drop out unnoticed."""
    fam = families(seed, 75)
    names = sorted(fam)
    thresh = seed % 2 == 1
    jobs, pts = data.target_jobs([(H, W)] * len(names), [fam[k] for k in names], 0.4, thresh, threads=4)
    kinds_seen = set()
    for i, name in enumerate(names):
        ref = R.polygon_jobs(H, W, fam[name], 0.4, thresh)
        got = [(int(j[1]), [tuple(p) for p in pts[j[2]:j[3]].tolist()], tuple(int(v) for v in j[4:])) for j in jobs if j[0] == i]
        assert sum(k != R.THRESH for k, _ in ref) == len(fam[name]) == 75, name
        assert [g[0] for g in got] == [k for k, _ in ref], name
        for (kind, a), (_, b, box) in zip(ref, got):
            assert R.same_cycle(a, b), (name, a, b)
            assert box == (min(x for x, _ in a), min(y for _, y in a), max(x for x, _ in a), max(y for _, y in a)), name
            kinds_seen.add((name, kind))
    assert ("bow_tie", R.GT) not in kinds_seen and ("convex", R.GT) in kinds_seen and ("dumbbell", R.GT) in kinds_seen
    assert ("strip", R.MASK) in kinds_seen and ("strip", R.GT) in kinds_seen
    assert jobs[:, 0].tolist() == sorted(jobs[:, 0].tolist())                      # image after image


def test_families_hold_what_they_claim():
    fam = families(11, 75)
    simple = lambda p: R.ring_is_simple([(float(x), float(y)) for x, y in p])
    assert not any(simple(p) for p in fam["bow_tie"]) and all(simple(p) for p in fam["convex"] if len({tuple(q) for q in p.tolist()}) == len(p))
    assert any((p < 0).any() or (p[:, 0] > W - 1).any() or (p[:, 1] > H - 1).any() for p in fam["out_of_range"])
    assert any((p != np.round(p)).any() for p in fam["fractional_duplicates"])
    assert all(any((p[i] == p[(i + 1) % len(p)]).all() for i in range(len(p))) for p in fam["fractional_duplicates"])
    two = [len(R.shrink_loops([tuple(int(v) for v in q) for q in np.clip(p, 0, [W - 1, H - 1])], 3.0)) for p in fam["dumbbell"]]
    assert max(two) >= 2                                                            # some dumbbells do fall apart


# ------------------------------------------------------------------------------------------------ the ABI
def test_overflow_reports_the_room_and_writes_nothing():
    lib = _lib.load()
    sizes = np.array([[200, 200]], np.int32)
    xy = np.asarray(SQUARE + DUMBBELL, np.float32)
    poly_offs, img_offs = np.array([0, 4, 16], np.int32), np.array([0, 2], np.int32)
    want_jobs, want_pts = data.target_jobs([(200, 200)], [[xy[:4], xy[4:]]], 0.4, True)
    nj, npts, over = C.c_int32(), C.c_int32(), C.c_int32()
    for cap_j, cap_p in ((0, 0), (len(want_jobs), len(want_pts) - 1), (len(want_jobs) - 1, len(want_pts))):
        jobs, pts = np.full((8, 8), -7, np.int32), np.full((len(want_pts) + 4, 2), -7, np.int32)
        _lib.check(lib.ocrvi_db_target_jobs(sizes.ctypes.data, xy.ctypes.data, poly_offs.ctypes.data, img_offs.ctypes.data, 1, 0.4, 1, jobs.ctypes.data,
                                            cap_j, pts.ctypes.data, cap_p, C.byref(nj), C.byref(npts), C.byref(over), 2))
        assert (over.value, nj.value, npts.value) == (1, len(want_jobs), len(want_pts))
        assert (jobs == -7).all() and (pts == -7).all()
    _lib.check(lib.ocrvi_db_target_jobs(sizes.ctypes.data, xy.ctypes.data, poly_offs.ctypes.data, img_offs.ctypes.data, 1, 0.4, 1, jobs.ctypes.data,
                                        nj.value, pts.ctypes.data, npts.value, C.byref(nj), C.byref(npts), C.byref(over), 2))
    assert over.value == 0 and (jobs[:nj.value] == want_jobs).all() and (pts[:npts.value] == want_pts).all() and (pts[npts.value:] == -7).all()
    # the Python wrapper repeats the call with the room it was told
    j2, p2 = data.target_jobs([(200, 200)], [[xy[:4], xy[4:]]], 0.4, True, cap_jobs=1, cap_points=3)
    assert (j2 == want_jobs).all() and (p2 == want_pts).all()


def test_bad_arguments_are_refused():
    with pytest.raises(ValueError):
        data.target_jobs([(0, 10)], [[]])
    with pytest.raises(ValueError):
        data.target_jobs([(10, _lib.DB_TARGET_MAX_SIDE + 1)], [[]])
    with pytest.raises(ValueError):
        data.target_jobs([(10, 10)], [[np.array([[0, 0], [5, 0], [np.nan, 5]], np.float32)]])
    with pytest.raises(ValueError):
        data.target_jobs([(10, 10)], [[np.array(SQUARE, np.float32)]], shrink_ratio=1.0)
    jobs, pts = data.target_jobs([(10, 10), (10, 10)], [[], [np.array([[0, 0], [5, 5]], np.float32)]])   # no polygon; one too short (:320)
    assert len(jobs) == 0 and len(pts) == 0


def test_header_and_exports():
    hdr = open(os.path.join(REPO, "include", "ocrvi.h")).read()
    for name in ("ocrvi_db_target_jobs", "ocrvi_db_target_maps", "ocrvi_resize_normalize_pad_pages"):
        assert f"int {name}(" in hdr and name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert f"#define OCRVI_DB_TARGET_JOB {_lib.DB_TARGET_JOB}" in hdr and f"#define OCRVI_DB_TARGET_MAX_SIDE {_lib.DB_TARGET_MAX_SIDE}" in hdr
    assert (_lib.DB_TARGET_GT, _lib.DB_TARGET_MASK, _lib.DB_TARGET_THRESH) == (R.GT, R.MASK, R.THRESH) == (0, 1, 2)
    for k, v in (("GT", 0), ("MASK", 1), ("THRESH", 2)):
        assert f"#define OCRVI_DB_TARGET_{k} {v}" in hdr
    assert "dataloader.py" in hdr and "np.minimum(dist_inside, dist_outside)" in hdr
    assert _lib.load().ocrvi_abi_version() == _lib.ABI_VERSION == 5             # exports were added, nothing changed
