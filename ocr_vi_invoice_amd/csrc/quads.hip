// Oriented text crops, host half (include/ocrvi.h, "Oriented text crops"): the minimum-area rectangle of each DB polygon in exact
// integer arithmetic, and the crop descriptors (size + destination -> source matrix) ocrvi_crop_quad_resize_normalize_pages consumes.
// No GPU is touched here.  tests/quad_ref.py restates both entries in Python integers / fractions; the two agree to the last bit.
#include <math.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "common.h"

namespace {

typedef std::pair<int64_t, int64_t> Pt;

inline int64_t cross3(const Pt& o, const Pt& a, const Pt& b) {
    return (a.first - o.first) * (b.second - o.second) - (a.second - o.second) * (b.first - o.first);
}

// strictly convex hull by the monotone chain: lower chain, then upper chain; collinear points dropped; hull[0] = the smallest (x, y)
void convex_hull(std::vector<Pt>& pts, std::vector<Pt>& hull) {
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    hull.clear();
    const size_t n = pts.size();
    if (n < 3) { hull = pts; return; }
    for (size_t i = 0; i < n; ++i) {
        while (hull.size() >= 2 && cross3(hull[hull.size() - 2], hull.back(), pts[i]) <= 0) hull.pop_back();
        hull.push_back(pts[i]);
    }
    const size_t lower = hull.size() + 1;
    for (size_t i = n - 1; i-- > 0;) {
        while (hull.size() >= lower && cross3(hull[hull.size() - 2], hull.back(), pts[i]) <= 0) hull.pop_back();
        hull.push_back(pts[i]);
    }
    hull.pop_back();   // the first point again
}

}  // namespace

extern "C" int ocrvi_min_area_quads(const int32_t* points, const int32_t* offs, int n, double* quads, int32_t* flags) {
    OCRVI_CHECK(offs && quads && flags && n >= 0, OCRVI_EINVAL, "min_area_quads: null argument or negative count");
    std::vector<Pt> pts, hull;
    for (int i = 0; i < n; ++i) {
        const int b = offs[i], e = offs[i + 1];
        OCRVI_CHECK(b >= 0 && e >= b && (e == b || points), OCRVI_EINVAL, "min_area_quads: polygon %d has offsets %d .. %d", i, b, e);
        double* q = quads + (size_t)i * 8;
        pts.clear();
        int64_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        for (int k = b; k < e; ++k) {
            const int64_t x = points[2 * (size_t)k], y = points[2 * (size_t)k + 1];
            OCRVI_CHECK(x >= -32768 && x <= 32767 && y >= -32768 && y <= 32767, OCRVI_EINVAL,
                        "min_area_quads: polygon %d point %d = (%lld, %lld) lies outside [-32768, 32767]", i, k - b, (long long)x, (long long)y);
            if (k == b) { x0 = x1 = x; y0 = y1 = y; }
            x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
            pts.emplace_back(x, y);
        }
        convex_hull(pts, hull);
        const size_t m = hull.size();
        if (m < 3) {   // degenerate (no point, one point, collinear points): the corners of the inclusive bounding box
            flags[i] = 1;
            const double c[8] = {(double)x0, (double)y0, (double)x1, (double)y0, (double)x1, (double)y1, (double)x0, (double)y1};
            for (int j = 0; j < 8; ++j) q[j] = c[j];
            continue;
        }
        flags[i] = 0;
        // per hull edge: extents along d and along n = (-dy, dx); area = (s1 - s0)(t1 - t0) / |d|^2, compared as exact rationals
        unsigned __int128 best_num = 0;
        int64_t best_den = 0, bs0 = 0, bs1 = 0, bt0 = 0, bt1 = 0, bdx = 0, bdy = 0;
        for (size_t k = 0; k < m; ++k) {
            const Pt &a = hull[k], &c = hull[(k + 1) % m];
            const int64_t dx = c.first - a.first, dy = c.second - a.second;
            int64_t s0 = 0, s1 = 0, t0 = 0, t1 = 0;
            for (size_t j = 0; j < m; ++j) {
                const int64_t s = hull[j].first * dx + hull[j].second * dy, t = hull[j].second * dx - hull[j].first * dy;
                if (j == 0) { s0 = s1 = s; t0 = t1 = t; }
                s0 = std::min(s0, s); s1 = std::max(s1, s); t0 = std::min(t0, t); t1 = std::max(t1, t);
            }
            const unsigned __int128 num = (unsigned __int128)(uint64_t)(s1 - s0) * (unsigned __int128)(uint64_t)(t1 - t0);   // < 2^66
            const int64_t den = dx * dx + dy * dy;                                                                           // < 2^34
            if (k == 0 || num * (unsigned __int128)(uint64_t)best_den < best_num * (unsigned __int128)(uint64_t)den) {
                best_num = num; best_den = den; bs0 = s0; bs1 = s1; bt0 = t0; bt1 = t1; bdx = dx; bdy = dy;
            }
        }
        const int64_t cs[4] = {bs0, bs1, bs1, bs0}, ct[4] = {bt0, bt0, bt1, bt1};
        const double den = (double)best_den;
        for (int j = 0; j < 4; ++j) {   // the numerators are exact integers below 2^53: one conversion, one division
            q[2 * j] = (double)(cs[j] * bdx - ct[j] * bdy) / den;
            q[2 * j + 1] = (double)(cs[j] * bdy + ct[j] * bdx) / den;
        }
    }
    return OCRVI_OK;
}

extern "C" int ocrvi_quad_crops(const double* quads, const int32_t* flags, int n, const int32_t* page_ids, const int32_t* page_hw, int32_t* crops,
                                double* m_inv) {
    OCRVI_CHECK(quads && flags && page_ids && page_hw && crops && m_inv && n >= 0, OCRVI_EINVAL, "quad_crops: null argument or negative count");
    for (int i = 0; i < 8 * n; ++i) OCRVI_CHECK(std::isfinite(quads[i]) && fabs(quads[i]) <= 1048576.0, OCRVI_EINVAL,
                                                "quad_crops: quad %d has a corner that is not finite or beyond 2^20", i / 8);
    for (int i = 0; i < n; ++i) {
        const double* q = quads + (size_t)i * 8;
        int32_t* c = crops + (size_t)i * 4;
        double* m = m_inv + (size_t)i * 9;
        c[0] = page_ids[i];
        c[3] = 0;
        int32_t w = 0, h = 0;
        if (!flags[i] && ocrvi_four_point_transform(q, nullptr, m, &w, &h) == OCRVI_OK) {
            c[1] = w;
            c[2] = h;
            continue;
        }
        if (!flags[i]) ::ocrvi::set_error("%s", "");   // the geometry's refusal is control flow here, not this call's error
        // the reference's crop (crop_image, src/det/test.py:123-130) as a descriptor: the bounding rectangle of the corners, clamped to the
        // page, under a pure translation
        double fx0 = q[0], fx1 = q[0], fy0 = q[1], fy1 = q[1];
        for (int j = 1; j < 4; ++j) {
            fx0 = std::min(fx0, q[2 * j]); fx1 = std::max(fx1, q[2 * j]);
            fy0 = std::min(fy0, q[2 * j + 1]); fy1 = std::max(fy1, q[2 * j + 1]);
        }
        const int64_t x0 = (int64_t)floor(fx0), y0 = (int64_t)floor(fy0);
        const int64_t bw = (int64_t)ceil(fx1) - x0 + 1, bh = (int64_t)ceil(fy1) - y0 + 1;
        const int64_t x = std::max<int64_t>(0, x0), y = std::max<int64_t>(0, y0);
        int64_t cw = std::max<int64_t>(std::min<int64_t>(bw, (int64_t)page_hw[2 * i + 1] - x), 0);
        int64_t ch = std::max<int64_t>(std::min<int64_t>(bh, (int64_t)page_hw[2 * i] - y), 0);
        if (cw == 0 || ch == 0) cw = ch = 0;
        c[1] = (int32_t)cw;
        c[2] = (int32_t)ch;
        const double t[9] = {1.0, 0.0, (double)x, 0.0, 1.0, (double)y, 0.0, 0.0, 1.0};
        for (int j = 0; j < 9; ++j) m[j] = t[j];
    }
    return OCRVI_OK;
}
