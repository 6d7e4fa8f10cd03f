// Host geometry of the DB ground-truth maps (DetectionDataset._load_sample's polygon loop, src/det/dataloader.py:334-350, with
// _shrink_polygon :71-102, _dilate_polygon :104-133 and the gates of _draw_border_map :139-161): every annotation polygon of an image becomes
// one or two fill jobs for the rasteriser (db_targets.hip).  The reference does this with shapely (validity, area, length), pyclipper
// (Execute(-d), Execute(+d)) and cv2.fillPoly; here the Clipper half is clip_union.h and the shapely half is stated below.  Parity with
// GEOS and Clipper themselves is unpinned, as for the rest of the host geometry; tests/dbtarget_ref.py is the independent Python statement
// this file must agree with job for job and point for point.  Host-only code without a HIP dependency.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "clip_union.h"

namespace dbtarget {

enum Kind { KIND_GT = 0, KIND_MASK = 1, KIND_THRESH = 2 };   // OCRVI_DB_TARGET_GT / _MASK / _THRESH
constexpr int kJobInts = 8;                                  // OCRVI_DB_TARGET_JOB: (image, kind, p0, p1, x0, y0, x1, y1)

struct F2 { double x, y; };   // a float32 coordinate pair, widened (exact)

inline int sign_of(double v) { return v > 0 ? 1 : (v < 0 ? -1 : 0); }
inline int orient(F2 a, F2 b, F2 c) {
#pragma clang fp contract(off)
    const double l = (b.x - a.x) * (c.y - a.y), r = (b.y - a.y) * (c.x - a.x);
    return sign_of(l - r);
}
inline bool in_box(F2 a, F2 b, F2 p) {
    return std::min(a.x, b.x) <= p.x && p.x <= std::max(a.x, b.x) && std::min(a.y, b.y) <= p.y && p.y <= std::max(a.y, b.y);
}
// closed segments a-b and c-e share a point
inline bool segments_meet(F2 a, F2 b, F2 c, F2 e) {
    const int o1 = orient(a, b, c), o2 = orient(a, b, e), o3 = orient(c, e, a), o4 = orient(c, e, b);
    if (o1 * o2 < 0 && o3 * o4 < 0) return true;
    if (o1 == 0 && in_box(a, b, c)) return true;
    if (o2 == 0 && in_box(a, b, e)) return true;
    if (o3 == 0 && in_box(c, e, a)) return true;
    if (o4 == 0 && in_box(c, e, b)) return true;
    return false;
}

// shapely Polygon(ring).is_valid as this library states it (include/ocrvi.h): consecutive duplicate vertices are dropped; at least three
// must remain; two edges that are not neighbours may not share a point; two neighbours may share only their common vertex (they may not
// fold back onto each other).  All predicates are the sign of a double cross product of double differences, without fused multiply-adds.
inline bool ring_is_simple(const std::vector<F2>& ring) {
#pragma clang fp contract(off)
    std::vector<F2> q;
    for (const F2& p : ring)
        if (q.empty() || p.x != q.back().x || p.y != q.back().y) q.push_back(p);
    if (q.size() > 1 && q.back().x == q[0].x && q.back().y == q[0].y) q.pop_back();
    const int m = (int)q.size();
    if (m < 3) return false;
    for (int i = 0; i < m; ++i) {
        const F2 a = q[i], b = q[(i + 1) % m];
        for (int j = i + 1; j < m; ++j) {
            const F2 c = q[j], e = q[(j + 1) % m];
            const bool next = j == i + 1, wrap = i == 0 && j == m - 1;
            if (next || wrap) {
                const F2 s = next ? b : a, p = next ? a : b, r = next ? e : c;   // common vertex, the two far ends
                if (orient(p, s, r) == 0 && (p.x - s.x) * (r.x - s.x) + (p.y - s.y) * (r.y - s.y) > 0) return false;
            } else if (segments_meet(a, b, c, e)) {
                return false;
            }
        }
    }
    return true;
}

// shapely .area (shoelace) and .length (perimeter) of the ring as given: sequential double sums
inline void ring_area_length(const std::vector<F2>& ring, double* area, double* length) {
#pragma clang fp contract(off)
    const size_t n = ring.size();
    double a2 = 0, len = 0;
    for (size_t i = 0; i < n; ++i) {
        const F2 a = ring[i], b = ring[(i + 1) % n];
        const double l = a.x * b.y, r = b.x * a.y;
        a2 += l - r;
        const double dx = b.x - a.x, dy = b.y - a.y;
        const double xx = dx * dx, yy = dy * dy;
        len += sqrt(xx + yy);
    }
    *area = fabs(a2) * 0.5;
    *length = len;
}

// max(paths, key=pyclipper.Area) over loops that may tie: the largest signed area; among equals the loop whose smallest vertex (by x, then
// y) is smallest; among those the first found.  The same rule, word for word, is in tests/dbtarget_ref.py.
inline int pick_largest(const std::vector<std::vector<clipu::P2>>& loops) {
    int best = -1;
    clipu::i64 best_a = 0;
    clipu::P2 best_v{0, 0};
    for (int k = 0; k < (int)loops.size(); ++k) {
        const clipu::i64 a2 = clipu::signed_area2(loops[k]);
        clipu::P2 v = loops[k][0];
        for (const clipu::P2& p : loops[k])
            if (p.x < v.x || (p.x == v.x && p.y < v.y)) v = p;
        if (best < 0 || a2 > best_a || (a2 == best_a && (v.x < best_v.x || (v.x == best_v.x && v.y < best_v.y)))) {
            best = k; best_a = a2; best_v = v;
        }
    }
    return best;
}

struct ImageJobs {
    std::vector<int32_t> jobs;     // kJobInts per job, p0 / p1 relative to this image's points
    std::vector<int32_t> points;   // (x, y) pairs
    void emit(int image, int kind, const std::vector<clipu::P2>& poly) {
        const int p0 = (int)(points.size() / 2);
        int x0 = poly[0].x, x1 = x0, y0 = poly[0].y, y1 = y0;
        for (const clipu::P2& p : poly) {
            points.push_back(p.x); points.push_back(p.y);
            x0 = std::min(x0, p.x); x1 = std::max(x1, p.x); y0 = std::min(y0, p.y); y1 = std::max(y1, p.y);
        }
        const int32_t row[kJobInts] = {image, kind, p0, p0 + (int)poly.size(), x0, y0, x1, y1};
        jobs.insert(jobs.end(), row, row + kJobInts);
    }
};

// One image: xy = float32 (x, y) pairs of all its polygons, polygon k owning vertices offs[k] .. offs[k+1].  A polygon of fewer than three
// vertices is skipped (the reference drops it when it reads the annotation, dataloader.py:320).  Coordinates must be finite.
inline void image_jobs(int image, int h, int w, const float* xy, const int32_t* offs, int n_poly, double shrink_ratio, bool want_thresh,
                       ImageJobs& out) {
#pragma clang fp contract(off)
    std::vector<F2> ring;
    std::vector<clipu::P2> poly, raw, dil;
    std::vector<std::vector<clipu::P2>> loops;
    const float xmax = (float)(w - 1), ymax = (float)(h - 1);
    for (int k = 0; k < n_poly; ++k) {
        const int v0 = offs[k], nv = offs[k + 1] - v0;
        if (nv < 3) continue;
        ring.resize(nv);
        poly.resize(nv);
        for (int i = 0; i < nv; ++i) {   // np.clip in float32 (:336-337), then astype(int) (:87)
            const float x = std::min(std::max(xy[2 * (size_t)(v0 + i)], 0.f), xmax), y = std::min(std::max(xy[2 * (size_t)(v0 + i) + 1], 0.f), ymax);
            ring[i] = {(double)x, (double)y};
            poly[i] = {(int)x, (int)y};
        }
        double area = 0, length = 0, d = 0;
        bool ok = ring_is_simple(ring);
        if (ok) {
            ring_area_length(ring, &area, &length);
            ok = !(area < 1) && !(length < 1);
        }
        if (ok) d = area * (1 - shrink_ratio * shrink_ratio) / length;
        int pick = -1;
        if (ok) {
            clipu::offset_round(poly, -d, raw);
            clipu::union_outer_loops(raw, loops);
            pick = pick_largest(loops);
        }
        if (pick >= 0) out.emit(image, KIND_GT, loops[pick]);
        else out.emit(image, KIND_MASK, poly);
        if (want_thresh && ok && d >= 1) {
            clipu::offset_round(poly, d, raw);
            clipu::union_outline(raw, dil);
            if (!dil.empty()) out.emit(image, KIND_THRESH, dil);
        }
    }
}

}  // namespace dbtarget
