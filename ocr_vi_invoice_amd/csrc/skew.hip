// Skew estimate (include/ocrvi.h, "Skew estimate"): the document finder's grey image -> horizontal edge strength -> for each of 257 slopes the
// projection profile along that slope and the sum of its squares.  Integer arithmetic throughout, no atomics: every (page, slope) score is
// accumulated in registers by one workgroup and stored once, so it does not depend on the grid.  tests/skew_ref.py restates every stage in
// numpy integers and must agree exactly.  The device entries only enqueue on their stream; pick and quad run on the host.
#include <math.h>

#include "docfind.h"

namespace ocrvi {
namespace {

constexpr int K = OCRVI_SKEW_K, SHIFT = OCRVI_SKEW_SHIFT, FLOOR = OCRVI_SKEW_FLOOR, ANGLES = OCRVI_SKEW_ANGLES;
static_assert(ANGLES == 2 * K + 1, "one slope per k in -K .. K");

__host__ __device__ inline int col_stride(int work_h) { return (work_h + 3) & ~3; }      // bytes of one column of the transposed edge image

// ---------------------------------------------------------------- edges
// E = |G[i][j+1] - G[i][j-1]| with a replicated border, 0 below FLOOR.  TRANSPOSED: a 64 x 64 tile goes through LDS so that both the reads
// (along j) and the writes (along i, into column j's col_stride(work_h) bytes) are contiguous; otherwise the output is row-major like G.
constexpr int ED_T = 64;
template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void edges_kernel(Pages pages, int work_h, int ww_cap, const uint8_t* g_base, size_t g_stride, uint8_t* e_base,
                                                    size_t e_stride) {
    Geom g;
    if (!page_geom(pages, blockIdx.z, work_h, ww_cap, g)) return;
    const int ww = g.ww, j0 = blockIdx.x * ED_T, i0 = blockIdx.y * ED_T, tid = threadIdx.x;
    if (j0 >= ww) return;
    const uint8_t* G = g_base + (size_t)blockIdx.z * g_stride;
    uint8_t* E = e_base + (size_t)blockIdx.z * e_stride;
    __shared__ uint8_t t[ED_T][ED_T + 4];
    for (int k = tid; k < ED_T * ED_T; k += 256) {
        const int ii = k / ED_T, jj = k - ii * ED_T, i = i0 + ii, j = j0 + jj;
        if (i >= work_h || j >= ww) continue;
        const uint8_t* row = G + (size_t)i * ww;
        const int a = row[min(j + 1, ww - 1)], b = row[max(j - 1, 0)], d = a > b ? a - b : b - a;
        const uint8_t e = (uint8_t)(d >= FLOOR ? d : 0);
        if (TRANSPOSED) t[jj][ii] = e;
        else E[(size_t)i * ww + j] = e;
    }
    if (!TRANSPOSED) return;
    __syncthreads();
    const int hs = col_stride(work_h);
    for (int k = tid; k < ED_T * ED_T; k += 256) {
        const int jj = k / ED_T, ii = k - jj * ED_T, i = i0 + ii, j = j0 + jj;
        if (i < work_h && j < ww) E[(size_t)j * hs + i] = t[jj][ii];
    }
}

// ---------------------------------------------------------------- profiles and scores
// A workgroup owns SC_SLOPES neighbouring slopes of one page.  Bin r of slope k collects E[r + o(j, k)][j] over the columns j; thread t owns
// the bins r0 + pass * SC_BINS + b * 256 + t, b < SC_BPT, in int32 registers (a profile is at most 255 * 8192).  The columns go through LDS
// in tiles of whole columns, SC_TILE bytes, each column col_stride(work_h) bytes apart as in the transposed edge image: for a column and a
// slope the offset is uniform, so a wave reads consecutive bytes, and all slopes of the workgroup reuse the tile.  Pages with more than
// SC_BINS bins (ww above about 1060 at 500 rows) take several passes over their tiles.  After a pass every thread squares its bins in 64
// bits; at the end the block adds the partial sums up and stores one uint64 per slope.  The workgroups of a page that is not processed
// store zeros, so every score of the call is written by this one launch (no memset node in a captured graph).
constexpr int SC_SLOPES = 8, SC_BPT = 3, SC_THREADS = 256, SC_BINS = SC_BPT * SC_THREADS, SC_TILE = 32768;
constexpr int SC_GROUPS = (ANGLES + SC_SLOPES - 1) / SC_SLOPES;
template <bool COLMAJOR>
__global__ __launch_bounds__(SC_THREADS) void scores_kernel(Pages pages, int work_h, int ww_cap, const uint8_t* e_base, size_t e_stride,
                                                            unsigned long long* scores) {
    Geom g;
    const int kidx0 = blockIdx.x * SC_SLOPES;                     // slope index k + K of the group's first slope
    if (!page_geom(pages, blockIdx.y, work_h, ww_cap, g)) {       // a page that is not processed: its scores are zero
        if (threadIdx.x < SC_SLOPES && kidx0 + threadIdx.x < ANGLES) scores[(size_t)blockIdx.y * ANGLES + kidx0 + threadIdx.x] = 0;
        return;
    }
    __shared__ uint32_t tile32[SC_TILE / 4];
    __shared__ unsigned long long part[SC_THREADS / 64][SC_SLOPES];
    uint8_t* tile = (uint8_t*)tile32;
    const uint8_t* E = e_base + (size_t)blockIdx.y * e_stride;
    const int ww = g.ww, tid = threadIdx.x, hs = col_stride(work_h), cj = ww >> 1, tj_max = SC_TILE / hs;
    const int obound = ((cj * K + (1 << (SHIFT - 1))) >> SHIFT) + 1, r0 = -obound, nbins = work_h + 2 * obound;
    unsigned long long total[SC_SLOPES];
#pragma unroll
    for (int s = 0; s < SC_SLOPES; ++s) total[s] = 0;
    for (int rbase = r0; rbase < r0 + nbins; rbase += SC_BINS) {
        int acc[SC_SLOPES][SC_BPT];
#pragma unroll
        for (int s = 0; s < SC_SLOPES; ++s)
#pragma unroll
            for (int b = 0; b < SC_BPT; ++b) acc[s][b] = 0;
        for (int j0 = 0; j0 < ww; j0 += tj_max) {
            const int tj = min(tj_max, ww - j0);
            __syncthreads();                                       // the previous tile has been read
            if (COLMAJOR) {
                const uint32_t* src = (const uint32_t*)(E + (size_t)j0 * hs);
                for (int q = tid; q < tj * (hs >> 2); q += SC_THREADS) tile32[q] = src[q];
            } else {
                for (int q = tid; q < tj * work_h; q += SC_THREADS) {
                    const int i = q / tj, jj = q - i * tj;
                    tile[jj * hs + i] = E[(size_t)i * ww + j0 + jj];
                }
            }
            __syncthreads();
            for (int jj = 0; jj < tj; ++jj) {
                const int c = j0 + jj - cj;
                const uint8_t* col = tile + jj * hs;
#pragma unroll
                for (int s = 0; s < SC_SLOPES; ++s) {
                    const int k = min(kidx0 + s, ANGLES - 1) - K;
                    const int i0 = rbase + tid + ((c * k + (1 << (SHIFT - 1))) >> SHIFT);      // an arithmetic shift: the floor
#pragma unroll
                    for (int b = 0; b < SC_BPT; ++b) {
                        const int i = i0 + b * SC_THREADS;
                        if ((unsigned)i < (unsigned)work_h) acc[s][b] += col[i];
                    }
                }
            }
        }
#pragma unroll
        for (int s = 0; s < SC_SLOPES; ++s)
#pragma unroll
            for (int b = 0; b < SC_BPT; ++b) total[s] += (unsigned long long)acc[s][b] * (unsigned long long)acc[s][b];
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 0; s < SC_SLOPES; ++s) {
        unsigned long long v = total[s];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) part[wave][s] = v;
    }
    __syncthreads();
    if (tid < SC_SLOPES && kidx0 + tid < ANGLES) {
        unsigned long long v = 0;
        for (int w = 0; w < SC_THREADS / 64; ++w) v += part[w][tid];
        scores[(size_t)blockIdx.y * ANGLES + kidx0 + tid] = v;
    }
}

// ---------------------------------------------------------------- host side
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Layout {
    size_t g_plane, e_plane, g, e, total;
};
inline Layout layout(int n, int work_h, int ww_cap) {
    Layout l;
    l.g_plane = align256((size_t)work_h * ww_cap);
    l.e_plane = align256((size_t)col_stride(work_h) * ww_cap);
    l.g = 0;
    l.e = l.g + l.g_plane * n;
    l.total = l.e + l.e_plane * n;
    return l;
}

template <bool TRANSPOSED>
int launch_edges(const Pages& p, int n, int work_h, int ww_cap, const uint8_t* G, size_t g_stride, uint8_t* E, size_t e_stride, hipStream_t st) {
    ProfScope ps("skew_edges", 0.0, 0.0, st);
    hipLaunchKernelGGL(edges_kernel<TRANSPOSED>, dim3((ww_cap + ED_T - 1) / ED_T, (work_h + ED_T - 1) / ED_T, n), dim3(256), 0, st, p, work_h, ww_cap, G,
                       g_stride, E, e_stride);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
template <bool COLMAJOR>
int launch_scores(const Pages& p, int n, int work_h, int ww_cap, const uint8_t* E, size_t e_stride, uint64_t* scores, hipStream_t st) {
    ProfScope ps("skew_scores", 0.0, 0.0, st);
    hipLaunchKernelGGL(scores_kernel<COLMAJOR>, dim3(SC_GROUPS, n), dim3(SC_THREADS), 0, st, p, work_h, ww_cap, E, e_stride,
                       (unsigned long long*)scores);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

}  // namespace
}  // namespace ocrvi

using namespace ocrvi;

extern "C" int ocrvi_skew_sizes(int n, int work_h, int ww_cap, size_t* workspace_bytes) {
    OCRVI_CHECK(workspace_bytes, OCRVI_EINVAL, "skew_sizes: null pointer");
    OCRVI_CHECK(n >= 1 && n <= 65535, OCRVI_EINVAL, "skew_sizes: %d pages (1 .. 65535)", n);
    OCRVI_TRY(check_work("skew_sizes", 0, work_h, ww_cap));
    *workspace_bytes = layout(n, work_h, ww_cap).total;
    return OCRVI_OK;
}

extern "C" int ocrvi_skew_scores_pages(int device, const int64_t* pages, int n, int work_h, int ww_cap, uint64_t* scores, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    OCRVI_CHECK(pages && scores && workspace, OCRVI_EINVAL, "skew_scores_pages: null pointer");
    OCRVI_CHECK(n >= 1 && n <= 65535, OCRVI_EINVAL, "skew_scores_pages: %d pages (1 .. 65535)", n);
    OCRVI_TRY(check_work("skew_scores_pages", device, work_h, ww_cap));
    const Layout l = layout(n, work_h, ww_cap);
    OCRVI_CHECK(workspace_bytes >= l.total, OCRVI_ENOMEM, "skew_scores_pages: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    OCRVI_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)scores & 7) == 0, OCRVI_EINVAL, "skew_scores_pages: workspace or scores misaligned");
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *G = (uint8_t*)workspace + l.g, *E = (uint8_t*)workspace + l.e;
    const Pages p{pages, nullptr, 0, 0, 0};
    OCRVI_TRY(launch_grey(p, n, work_h, ww_cap, G, l.g_plane, st));
    OCRVI_TRY(launch_edges<true>(p, n, work_h, ww_cap, G, l.g_plane, E, l.e_plane, st));
    return launch_scores<true>(p, n, work_h, ww_cap, E, l.e_plane, scores, st);
}

extern "C" int ocrvi_skew_edges_u8(int device, const uint8_t* grey, int work_h, int ww, uint8_t* edges, void* stream) {
    OCRVI_CHECK(grey && edges && grey != edges, OCRVI_EINVAL, "skew_edges_u8: null pointer or edges == grey");
    OCRVI_TRY(check_work("skew_edges_u8", device, work_h, ww));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_edges<false>(Pages{nullptr, nullptr, work_h, ww, ww}, 1, work_h, ww, grey, 0, edges, 0, (hipStream_t)stream);
}

extern "C" int ocrvi_skew_scores(int device, const uint8_t* edges, int work_h, int ww, uint64_t* scores, void* stream) {
    OCRVI_CHECK(edges && scores && ((uintptr_t)scores & 7) == 0, OCRVI_EINVAL, "skew_scores: null pointer or scores misaligned");
    OCRVI_TRY(check_work("skew_scores", device, work_h, ww));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_scores<false>(Pages{nullptr, nullptr, work_h, ww, ww}, 1, work_h, ww, edges, 0, scores, (hipStream_t)stream);
}

extern "C" int ocrvi_skew_pick(const uint64_t* scores, int32_t* k, double* angle_deg, double* gain) {
    OCRVI_CHECK(scores && k && angle_deg && gain, OCRVI_EINVAL, "skew_pick: null pointer");
    int best = 0;                                                  // k = 0 first, then |k| = 1, 2, ..: +k ahead of -k, strict comparisons
    for (int a = 1; a <= K; ++a) {
        if (scores[K + a] > scores[K + best]) best = a;
        if (scores[K - a] > scores[K + best]) best = -a;
    }
    const uint64_t sb = scores[K + best], s0 = scores[K];
    *k = best;
    *angle_deg = atan((double)best / 512.0) * 180.0 / 3.14159265358979323846;
    *gain = s0 ? (double)sb / (double)s0 : (sb ? (double)INFINITY : 1.0);
    return OCRVI_OK;
}

extern "C" int ocrvi_skew_quad(int h, int w, int k, double* quad) {
#pragma clang fp contract(off)
    OCRVI_CHECK(quad, OCRVI_EINVAL, "skew_quad: null pointer");
    OCRVI_CHECK(h >= 1 && w >= 1 && h <= DOC_MAX_SIDE && w <= DOC_MAX_SIDE, OCRVI_EINVAL, "skew_quad: a %d x %d page (sides 1 .. %d)", h, w, DOC_MAX_SIDE);
    OCRVI_CHECK(k >= -K && k <= K, OCRVI_EINVAL, "skew_quad: k = %d (%d .. %d)", k, -K, K);
    const double t = (double)k / 512.0, c = 1.0 / sqrt(1.0 + t * t), s = t * c;
    const double cx = (double)(w - 1) / 2.0, cy = (double)(h - 1) / 2.0;
    const double px[4] = {0.0, (double)w, (double)w, 0.0}, py[4] = {0.0, 0.0, (double)h, (double)h};
    double amin = 0, amax = 0, bmin = 0, bmax = 0;
    for (int i = 0; i < 4; ++i) {
        const double dx = px[i] - cx, dy = py[i] - cy;
        const double a = dx * c + dy * s, b = dy * c - dx * s;
        if (i == 0 || a < amin) amin = a;
        if (i == 0 || a > amax) amax = a;
        if (i == 0 || b < bmin) bmin = b;
        if (i == 0 || b > bmax) bmax = b;
    }
    const double qa[4] = {amin, amax, amax, amin}, qb[4] = {bmin, bmin, bmax, bmax};
    for (int i = 0; i < 4; ++i) {
        quad[2 * i] = cx + qa[i] * c - qb[i] * s;
        quad[2 * i + 1] = cy + qa[i] * s + qb[i] * c;
    }
    return OCRVI_OK;
}
