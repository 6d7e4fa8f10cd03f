// Result overlay (include/ocrvi.h, "Result overlay"): draw_boxes_with_text (src/pipeline/pipeline2.py:173-190) as a segment list built on the
// host and one kernel that paints every page of a call in place.  The painting rule, the segment order and the label font are stated in
// the header; tests/overlay_ref.py restates them in numpy int64 and in fractions, and the kernel equals that reference bit for bit.
#include <algorithm>

#include "common.h"
#include "overlay_font.h"

using namespace ocrvi;

namespace {

constexpr int COORD = OCRVI_OVERLAY_MAX_COORD;
constexpr int SEG = OCRVI_OVERLAY_SEG, PRIM = OCRVI_OVERLAY_PRIM;

// ---------------------------------------------------------------- host: boxes -> segments and primitives
struct Builder {
    int32_t *segs, *prims;
    int64_t seg_cap, prim_cap, ns = 0, np = 0;
    int T, dil;
    // the open primitive
    int64_t first = 0;
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;

    void open() { first = ns; }
    int emit(int ax, int ay, int bx, int by, uint32_t colour, int pair, int page) {
        OCRVI_CHECK(ax >= -COORD && ax <= COORD && ay >= -COORD && ay <= COORD && bx >= -COORD && bx <= COORD && by >= -COORD && by <= COORD,
                    OCRVI_EINVAL, "overlay_segments: page %d pair %d: segment (%d, %d) -> (%d, %d) leaves [-%d, %d]", page, pair, ax, ay, bx, by,
                    COORD, COORD);
        if (segs) {
            OCRVI_CHECK(ns < seg_cap, OCRVI_EINVAL, "overlay_segments: the segment table holds %lld entries, more are needed", (long long)seg_cap);
            int32_t* s = segs + ns * SEG;
            s[0] = ax; s[1] = ay; s[2] = bx; s[3] = by; s[4] = (int32_t)colour; s[5] = T; s[6] = pair; s[7] = 0;
        }
        const int lx = std::min(ax, bx), hx = std::max(ax, bx), ly = std::min(ay, by), hy = std::max(ay, by);
        if (ns == first) { x0 = lx; x1 = hx; y0 = ly; y1 = hy; }
        x0 = std::min(x0, lx); x1 = std::max(x1, hx); y0 = std::min(y0, ly); y1 = std::max(y1, hy);
        ++ns;
        return OCRVI_OK;
    }
    int close(int kind, int pair) {
        if (ns == first) return OCRVI_OK;
        if (prims) {
            OCRVI_CHECK(np < prim_cap, OCRVI_EINVAL, "overlay_segments: the primitive table holds %lld entries, more are needed", (long long)prim_cap);
            int32_t* p = prims + np * PRIM;
            p[0] = (int32_t)first; p[1] = (int32_t)ns; p[2] = x0 - dil; p[3] = y0 - dil; p[4] = x1 + dil; p[5] = y1 + dil; p[6] = kind; p[7] = pair;
        }
        ++np;
        return OCRVI_OK;
    }
};

}  // namespace

extern "C" int ocrvi_overlay_segments(const int32_t* points, const int32_t* offs, const int32_t* page_boxes, const int32_t* page_pairs,
                                      const int32_t* page_hw, int n_pages, uint32_t box_rgb, uint32_t label_rgb, int thickness, int32_t* segs,
                                      int64_t seg_cap, int32_t* prims, int64_t prim_cap, int32_t* prim_offs, int64_t* n_segs, int64_t* n_prims) {
    OCRVI_CHECK(offs && page_boxes && page_hw && n_segs && n_prims && n_pages >= 0, OCRVI_EINVAL,
                "overlay_segments: null argument or negative page count");
    const bool query = !segs && !prims && !prim_offs;
    OCRVI_CHECK(query || (segs && prims && prim_offs && seg_cap >= 0 && prim_cap >= 0), OCRVI_EINVAL,
                "overlay_segments: segs, prims and prim_offs are given together, or all null for the size query");
    OCRVI_CHECK(thickness >= 1 && thickness <= 15, OCRVI_EINVAL, "overlay_segments: thickness %d outside 1..15", thickness);
    OCRVI_CHECK(box_rgb <= 0xffffffu && label_rgb <= 0xffffffu, OCRVI_EINVAL, "overlay_segments: a colour is r | g << 8 | b << 16, at most 0xffffff");
    for (int p = 0; p < n_pages; ++p) {
        const int h = page_hw[2 * p], w = page_hw[2 * p + 1];
        OCRVI_CHECK(h >= 1 && h <= COORD && w >= 1 && w <= COORD, OCRVI_EINVAL, "overlay_segments: page %d is %d x %d, sides must lie in 1..%d", p, h, w,
                    COORD);
        OCRVI_CHECK(page_boxes[p] >= 0 && page_boxes[p + 1] >= page_boxes[p], OCRVI_EINVAL, "overlay_segments: page %d owns boxes %d .. %d", p,
                    page_boxes[p], page_boxes[p + 1]);
        OCRVI_CHECK(!page_pairs || page_pairs[p] >= 0, OCRVI_EINVAL, "overlay_segments: page %d has %d texts", p, page_pairs ? page_pairs[p] : 0);
    }
    Builder b{segs, prims, seg_cap, prim_cap};
    b.T = thickness;
    b.dil = (thickness + 1) / 2;
    for (int p = 0; p < n_pages; ++p) {
        if (prim_offs) prim_offs[p] = (int32_t)b.np;
        const int j0 = page_boxes[p];
        int pairs = page_boxes[p + 1] - j0;
        if (page_pairs) pairs = std::min(pairs, (int)page_pairs[p]);
        for (int i = 0; i < pairs; ++i) {
            const int vb = offs[j0 + i], ve = offs[j0 + i + 1], n = ve - vb;
            OCRVI_CHECK(vb >= 0 && n >= 0 && (n == 0 || points), OCRVI_EINVAL, "overlay_segments: page %d box %d has offsets %d .. %d", p, i, vb, ve);
            if (n == 0) continue;   // nothing to outline and no vertex to hang the label on
            const int32_t* v = points + 2 * (size_t)vb;
            // validated first: the label arithmetic below then stays far from int32's ends
            for (int k = 0; k < n; ++k)
                OCRVI_CHECK(v[2 * k] >= -COORD && v[2 * k] <= COORD && v[2 * k + 1] >= -COORD && v[2 * k + 1] <= COORD, OCRVI_EINVAL,
                            "overlay_segments: page %d box %d vertex %d = (%d, %d) lies outside [-%d, %d]", p, i, k, v[2 * k], v[2 * k + 1], COORD, COORD);
            b.open();
            int top = 0, max_y = v[1];
            for (int k = 0; k < n; ++k) {
                const int m = (k + 1) % n;
                OCRVI_TRY(b.emit(v[2 * k], v[2 * k + 1], v[2 * m], v[2 * m + 1], box_rgb, i, p));
                if (v[2 * k + 1] < v[2 * top + 1]) top = k;   // the first vertex of minimum y (np.argmin)
                max_y = std::max(max_y, (int)v[2 * k + 1]);
            }
            OCRVI_TRY(b.close(0, i));
            // the label (pipeline2.py:182-188)
            const int tx = v[2 * top];
            int ty = v[2 * top + 1] - 10;
            if (ty < 20) ty = max_y + 20;
            int digits[10], nd = 0;
            for (int q = i + 1; q > 0; q /= 10) digits[nd++] = q % 10;
            b.open();
            for (int k = 0; k < nd; ++k) {
                const int dgt = digits[nd - 1 - k], ox = tx + OVERLAY_DIGIT_ADVANCE * k;
                for (int s = 0; s < OVERLAY_STROKES; ++s)
                    if (OVERLAY_DIGIT[dgt] >> s & 1)
                        OCRVI_TRY(b.emit(ox + OVERLAY_STROKE[s][0], ty + OVERLAY_STROKE[s][1], ox + OVERLAY_STROKE[s][2], ty + OVERLAY_STROKE[s][3],
                                         label_rgb, i, p));
            }
            OCRVI_TRY(b.close(1, i));
        }
    }
    if (prim_offs) prim_offs[n_pages] = (int32_t)b.np;
    OCRVI_CHECK(b.ns <= INT32_MAX, OCRVI_EINVAL, "overlay_segments: %lld segments, more than a 32-bit index addresses", (long long)b.ns);
    *n_segs = b.ns;
    *n_prims = b.np;
    return OCRVI_OK;
}

// ---------------------------------------------------------------- device: one launch paints every page
namespace {

constexpr int TILE_W = 64, TILE_H = 16, NT = 256, PPT = TILE_W * TILE_H / NT;   // 4 pixels per thread: column tid & 63, rows (tid >> 6) + 4 j
constexpr int CHUNK = NT;                                                       // segments staged per pass

// a segment as the pixel loop wants it (48 bytes; every lane reads the same entry: an LDS broadcast)
struct Staged {
    int ax, ay, dx, dy;
    long long L2, K;      // d.d and floor(T^2 L2 / 4)
    int T2, ord, colour, pad;
};

__global__ __launch_bounds__(NT) void overlay_pages_kernel(const int64_t* __restrict__ pages, const int32_t* __restrict__ prims,
                                                           const int32_t* __restrict__ segs, const int32_t* __restrict__ prim_offs) {
    const int page = blockIdx.z;
    const int64_t* e = pages + (size_t)page * OCRVI_PAGE_ENTRY;
    uint8_t* img = (uint8_t*)e[0];
    const long long h = e[1], w = e[2];
    const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    if (!img || h <= 0 || w <= 0 || tx0 >= w || ty0 >= h) return;   // block-uniform
    const int tx1 = tx0 + TILE_W - 1, ty1 = ty0 + TILE_H - 1;
    const int p0 = prim_offs[page], p1 = prim_offs[page + 1];

    __shared__ Staged s_seg[CHUNK];
    __shared__ int s_beg[NT];          // first segment of each hit primitive of the round
    __shared__ int s_pre[2][NT];       // inclusive prefix sums of the hits' segment counts
    // the counters of the two compactions.  Every reset of one lies a barrier behind its last reader and a barrier ahead of its next
    // writer: s_nhit is reset at the top of a round, behind the barrier that ends the previous one; s_nseg alternates between two
    // slots, pass p counts in slot p & 1 and resets the other one between its two barriers
    __shared__ int s_nhit, s_nseg[2];

    const int tid = threadIdx.x;
    const int px = tx0 + (tid & (TILE_W - 1)), py = ty0 + (tid >> 6);
    int best[PPT], col[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) { best[j] = -1; col[j] = 0; }

    for (int r = p0; r < p1; r += NT) {
        // ---- level 1: this round's primitives against the tile, the hits compacted (their order does not matter: the largest ordinal wins)
        if (tid == 0) { s_nhit = 0; s_nseg[0] = 0; }
        s_pre[0][tid] = 0;
        __syncthreads();
        if (r + tid < p1) {
            const int4 a = *(const int4*)(prims + (size_t)(r + tid) * PRIM);       // first, last, x0, y0
            const int2 b = *(const int2*)(prims + (size_t)(r + tid) * PRIM + 4);   // x1, y1
            if (a.y > a.x && a.z <= tx1 && b.x >= tx0 && a.w <= ty1 && b.y >= ty0) {
                const int k = atomicAdd(&s_nhit, 1);   // LDS
                s_beg[k] = a.x;
                s_pre[0][k] = a.y - a.x;
            }
        }
        __syncthreads();
        const int nhit = s_nhit;
        if (nhit == 0) { __syncthreads(); continue; }   // block-uniform (the barrier keeps the next round's reset behind this read)
        int cur = 0;
        for (int off = 1; off < NT; off <<= 1, cur ^= 1) {
            const int v = s_pre[cur][tid] + (tid >= off ? s_pre[cur][tid - off] : 0);
            s_pre[cur ^ 1][tid] = v;
            __syncthreads();
        }                                               // 8 steps: the result is back in s_pre[0]
        const int* pre = s_pre[0];
        const int total = pre[NT - 1];
        // ---- level 2: the hits' segments, CHUNK at a time: staged (a conservative box test drops most), then every pixel against every staged one
        for (int c = 0, slot = 0; c < total; c += CHUNK, slot ^= 1) {
            __syncthreads();                            // the previous pass has finished reading s_seg and its own counter
            if (tid == 0) s_nseg[slot ^ 1] = 0;         // the next pass's counter: read last in the previous pass, ahead of the barrier above
            const int q = c + tid;
            if (q < total) {
                int lo = 0, hi = nhit - 1;              // the smallest k with pre[k] > q
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (pre[mid] > q) hi = mid; else lo = mid + 1;
                }
                const int si = s_beg[lo] + (q - (lo ? pre[lo - 1] : 0));
                const int4 a = *(const int4*)(segs + (size_t)si * SEG);       // a.x, a.y, b.x, b.y
                const int2 b = *(const int2*)(segs + (size_t)si * SEG + 4);   // colour, T
                const int T = b.y, dil = (T + 1) >> 1;
                if (min(a.x, a.z) - dil <= tx1 && max(a.x, a.z) + dil >= tx0 && min(a.y, a.w) - dil <= ty1 && max(a.y, a.w) + dil >= ty0) {
                    const int k = atomicAdd(&s_nseg[slot], 1);   // LDS
                    Staged g;
                    g.ax = a.x; g.ay = a.y; g.dx = a.z - a.x; g.dy = a.w - a.y;
                    g.L2 = (long long)g.dx * g.dx + (long long)g.dy * g.dy;
                    g.T2 = T * T;
                    g.K = ((long long)g.T2 * g.L2) >> 2;
                    g.ord = si; g.colour = b.x; g.pad = 0;
                    s_seg[k] = g;
                }
            }
            __syncthreads();
            const int nseg = s_nseg[slot];
            for (int k = 0; k < nseg; ++k) {
                const Staged g = s_seg[k];
                const int qx = px - g.ax;
#pragma unroll
                for (int j = 0; j < PPT; ++j) {
                    const int qy = py + 4 * j - g.ay;
                    const long long t = (long long)qx * g.dx + (long long)qy * g.dy;
                    bool cov;
                    if (t <= 0) {
                        cov = 4 * ((long long)qx * qx + (long long)qy * qy) <= g.T2;
                    } else if (t >= g.L2) {
                        const int rx = qx - g.dx, ry = qy - g.dy;
                        cov = 4 * ((long long)rx * rx + (long long)ry * ry) <= g.T2;
                    } else {
                        const long long cr = (long long)g.dx * qy - (long long)g.dy * qx;
                        const unsigned long long ac = (unsigned long long)(cr < 0 ? -cr : cr);
                        // K < 2^37: a cross product of 2^31 or more is never inside, and below that its square is a 32 x 32 -> 64 bit product
                        cov = ac < 0x80000000ull && (unsigned long long)(unsigned)ac * (unsigned)ac <= (unsigned long long)g.K;
                    }
                    if (cov && g.ord > best[j]) { best[j] = g.ord; col[j] = g.colour; }
                }
            }
        }
        __syncthreads();                                // the next round rewrites the hit lists
    }
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int y = py + 4 * j;
        if (best[j] >= 0 && px < w && y < h) {          // only painted pixels inside the page are stored
            uint8_t* o = img + ((size_t)y * (size_t)w + (size_t)px) * 3;
            o[0] = (uint8_t)(col[j] & 255);
            o[1] = (uint8_t)((col[j] >> 8) & 255);
            o[2] = (uint8_t)((col[j] >> 16) & 255);
        }
    }
}

}  // namespace

extern "C" int ocrvi_overlay_pages(int device, const int64_t* pages, int n_pages, const int32_t* prims, const int32_t* segs, const int32_t* prim_offs,
                                   int max_h, int max_w, void* stream) {
    OCRVI_CHECK(pages && prims && segs && prim_offs, OCRVI_EINVAL, "overlay_pages: null argument");
    OCRVI_CHECK(n_pages >= 1 && n_pages <= 65535, OCRVI_EINVAL, "overlay_pages: %d pages (1..65535)", n_pages);
    OCRVI_CHECK(max_h >= 1 && max_h <= COORD && max_w >= 1 && max_w <= COORD, OCRVI_EINVAL, "overlay_pages: max_h %d, max_w %d outside 1..%d", max_h,
                max_w, COORD);
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    hipLaunchKernelGGL(overlay_pages_kernel, dim3(cdiv(max_w, TILE_W), cdiv(max_h, TILE_H), n_pages), dim3(NT), 0, (hipStream_t)stream, pages, prims,
                       segs, prim_offs);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
