// The DB ground-truth maps on the device (include/ocrvi.h, "DB ground truth"): what DetectionDataset._load_sample's four cv2.fillPoly
// targets look like after _resize_pad (src/det/dataloader.py:328-350, 240-273), from the fill jobs of ocrvi_db_target_jobs.
//
// The reference fills h x w maps and then samples them with cv2.INTER_NEAREST.  Here the full-resolution maps never exist: an output
// pixel (X, Y) reads source pixel (sx, sy) = (min(floor(X / (new_w / w)), w - 1), likewise y), so the fill is evaluated at (sx, sy) only.
// A pixel is filled when it lies on the Bresenham line of an edge (cv::LineIterator, 8-connected, drawn from vertex i to vertex i + 1) or
// inside the even-odd interior at pixel centres with the half-open vertex rule -- oracle/dbpost_cpu.polygon_mask's statement of
// cv2.fillPoly, the one box_score in dbpost.hip uses.  Both tests are closed forms in integers:
//   * x-major line, step i = |px - ax| in 0 .. dx: its row offset k is the integer with 0 <= dx - 2 dy i + 2 dx k < 2 dx (the error term of
//     the walk after its conditional step); y-major likewise with the axes exchanged.
//   * row py crosses edge a-b (ay <= py < by or by <= py < ay) at c = ax + (py - ay)(bx - ax) / (by - ay).  With the crossings sorted and
//     paired, px is inside when the number of crossings < px is odd or a crossing equals px: compared as integers, N = (py - ay)(bx - ax)
//     against (px - ax)(by - ay).  The double arithmetic of polygon_mask decides the same way while |coordinates| < 2^20: 1 / |by - ay|
//     is then far above the rounding error of the quotient and of the sum.
// One block per job walks the job's bounding box in OUTPUT pixels, 256 at a time, with the vertices staged in LDS (DBT_STAGE per pass; a
// longer polygon takes several passes per tile, the parity and the hit flag stay in registers).  Every store to a map writes that map's one
// constant, so overlapping jobs need neither an order nor atomics.
#include "common.h"

namespace ocrvi {

constexpr int DBT_STAGE = 1024;       // vertices per LDS pass (one more is staged: the end of the last edge)
constexpr int DBT_TILE_BLOCKS = 4;    // blocks that share one job's tiles

// gt = 0, mask = 1 inside new_h x new_w, thresh_map = thresh_mask = 0: V consecutive pixels of a row per thread (V = 4: 16-byte stores)
template <int V>
__global__ __launch_bounds__(256) void db_target_init_kernel(const int32_t* __restrict__ rows, int n, int S, float* __restrict__ gt,
                                                             float* __restrict__ mask, float* __restrict__ tmap, float* __restrict__ tmask) {
    const int SV = S / V;
    const size_t per = (size_t)S * SV, total = (size_t)n * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int img = (int)(i / per);
        const size_t r = i - (size_t)img * per;
        const int y = (int)(r / SV), x = (int)(r - (size_t)y * SV) * V;
        const int nh = min(rows[4 * img + 2], S), nw = min(rows[4 * img + 3], S);
        const size_t o = ((size_t)img * S + y) * S + x;
        if constexpr (V == 4) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const bool in = y < nh;
            *(float4*)(gt + o) = z;
            *(float4*)(tmap + o) = z;
            *(float4*)(tmask + o) = z;
            *(float4*)(mask + o) = make_float4(in && x < nw ? 1.f : 0.f, in && x + 1 < nw ? 1.f : 0.f, in && x + 2 < nw ? 1.f : 0.f,
                                               in && x + 3 < nw ? 1.f : 0.f);
        } else {
            gt[o] = 0.f; tmap[o] = 0.f; tmask[o] = 0.f;
            mask[o] = (y < nh && x < nw) ? 1.f : 0.f;
        }
    }
}

// is (px, py) a pixel of the line walked from a to b?
__device__ __forceinline__ bool on_line(int ax, int ay, int bx, int by, int px, int py) {
    const int dx = abs(bx - ax), dy = abs(by - ay);
    const int ix = bx >= ax ? px - ax : ax - px, iy = by >= ay ? py - ay : ay - py;   // steps along each axis, in the walking direction
    const bool xmajor = dx >= dy;
    const int dm = xmajor ? dx : dy, dn = xmajor ? dy : dx, i = xmajor ? ix : iy, k = xmajor ? iy : ix;
    if (dm == 0) return ix == 0 && iy == 0;
    if (i < 0 || i > dm) return false;
    const long long t = (long long)dm - 2ll * dn * i + 2ll * dm * k;
    return t >= 0 && t < 2ll * dm;
}

__global__ __launch_bounds__(256) void db_target_fill_kernel(const int32_t* __restrict__ jobs, int n_jobs, const int32_t* __restrict__ points,
                                                             int n_points, const int32_t* __restrict__ rows, int n, int S, float thresh_max,
                                                             float* __restrict__ gt, float* __restrict__ mask, float* __restrict__ tmap,
                                                             float* __restrict__ tmask) {
#pragma clang fp contract(off)
    __shared__ int2 pts[DBT_STAGE + 1];
    const int tid = threadIdx.x;
    for (int job = blockIdx.y; job < n_jobs; job += gridDim.y) {   // everything up to the tile loop is uniform over the block
        const int32_t* J = jobs + (size_t)job * OCRVI_DB_TARGET_JOB;
        const int img = J[0], kind = J[1], p0 = J[2], p1 = J[3];
        if (img < 0 || img >= n || kind < 0 || kind > OCRVI_DB_TARGET_THRESH || p0 < 0 || p1 <= p0 || p1 > n_points) continue;
        const int h = rows[4 * img], w = rows[4 * img + 1];
        const int nh = min(rows[4 * img + 2], S), nw = min(rows[4 * img + 3], S);
        if (h <= 0 || w <= 0 || nh <= 0 || nw <= 0) continue;
        const int x0 = max(J[4], 0), y0 = max(J[5], 0), x1 = min(J[6], w - 1), y1 = min(J[7], h - 1);
        if (x0 > x1 || y0 > y1) continue;
        // cv2.resize(..., INTER_NEAREST): sx = min(floor(X * (1 / (new_w / w))), w - 1) in double; it never decreases with X, so the output
        // pixels that read the box lie in a range, taken two pixels wide of the mark and tested pixel by pixel below
        const double fx = (double)nw / (double)w, fy = (double)nh / (double)h;
        const double ifx = 1.0 / fx, ify = 1.0 / fy;
        const int Xlo = max((int)floor((double)x0 * fx) - 2, 0), Xhi = min((int)ceil((double)(x1 + 1) * fx) + 2, nw - 1);
        const int Ylo = max((int)floor((double)y0 * fy) - 2, 0), Yhi = min((int)ceil((double)(y1 + 1) * fy) + 2, nh - 1);
        if (Xlo > Xhi || Ylo > Yhi) continue;
        const int bw = Xhi - Xlo + 1, npx = bw * (Yhi - Ylo + 1), tiles = (npx + 255) >> 8;
        const int n_pts = p1 - p0, passes = (n_pts + DBT_STAGE - 1) / DBT_STAGE;
        bool staged = false;
        for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const int idx = tile * 256 + tid;
            const int Y = Ylo + idx / bw, X = Xlo + idx % bw;
            const int px = min((int)floor((double)X * ifx), w - 1), py = min((int)floor((double)Y * ify), h - 1);
            const bool live = idx < npx && px >= x0 && px <= x1 && py >= y0 && py <= y1;
            bool hit = false, odd = false;
            for (int pass = 0; pass < passes; ++pass) {
                const int c0 = pass * DBT_STAGE, cnt = min(DBT_STAGE, n_pts - c0);   // edges c0 .. c0 + cnt - 1
                if (passes > 1 || !staged) {
                    __syncthreads();   // the previous pass, tile or job is done with the stage
                    for (int j = tid; j <= cnt; j += 256) {
                        const int v = (c0 + j) % n_pts;
                        pts[j] = make_int2(points[2 * (size_t)(p0 + v)], points[2 * (size_t)(p0 + v) + 1]);
                    }
                    __syncthreads();
                    staged = true;
                }
                if (live && !hit) {
                    for (int e = 0; e < cnt; ++e) {
                        const int2 a = pts[e], b = pts[e + 1];
                        if (a.y != b.y && ((a.y <= py && py < b.y) || (b.y <= py && py < a.y))) {
                            const long long D = b.y - a.y, N = (long long)(py - a.y) * (b.x - a.x), M = (long long)(px - a.x) * D;
                            const long long l = D > 0 ? N : M, r = D > 0 ? M : N;   // crossing < px  <=>  l < r
                            odd ^= l < r;
                            hit |= l == r;
                        }
                        hit |= on_line(a.x, a.y, b.x, b.y, px, py);
                    }
                }
            }
            if (live && (hit || odd)) {
                const size_t o = ((size_t)img * S + Y) * S + X;
                if (kind == OCRVI_DB_TARGET_GT) gt[o] = 1.f;
                else if (kind == OCRVI_DB_TARGET_MASK) mask[o] = 0.f;
                else { tmask[o] = 1.f; tmap[o] = thresh_max; }
            }
        }
    }
}

}  // namespace ocrvi

using namespace ocrvi;

extern "C" int ocrvi_db_target_maps(int device, const int32_t* jobs, int n_jobs, const int32_t* points, int n_points, const int32_t* rows, int n,
                                    int S, float thresh_max, float* gt, float* mask, float* thresh_map, float* thresh_mask, void* stream) {
    OCRVI_CHECK(rows && gt && mask && thresh_map && thresh_mask && n > 0 && S > 0 && S <= OCRVI_DB_TARGET_MAX_SIDE && n_jobs >= 0 && n_points >= 0 &&
                    (n_jobs == 0 || (jobs && points)),
                OCRVI_EINVAL, "db_target_maps: bad argument (1 <= S <= %d)", OCRVI_DB_TARGET_MAX_SIDE);
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const bool vec = S % 4 == 0 && ((((uintptr_t)gt) | ((uintptr_t)mask) | ((uintptr_t)thresh_map) | ((uintptr_t)thresh_mask)) & 15) == 0;
    const size_t total = (size_t)n * S * (vec ? S / 4 : S);
    const int grid = (int)std::min<size_t>((total + 255) / 256, 16384);
    {
        ProfScope ps("db_target_init", 0.0, 16.0 * n * S * S, (hipStream_t)stream);
        if (vec) hipLaunchKernelGGL(db_target_init_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, rows, n, S, gt, mask, thresh_map, thresh_mask);
        else hipLaunchKernelGGL(db_target_init_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, rows, n, S, gt, mask, thresh_map, thresh_mask);
    }
    OCRVI_HIP(hipGetLastError());
    if (n_jobs > 0) {
        ProfScope ps("db_target_fill", 0.0, 0.0, (hipStream_t)stream);
        hipLaunchKernelGGL(db_target_fill_kernel, dim3(DBT_TILE_BLOCKS, std::min(n_jobs, 65535)), dim3(256), 0, (hipStream_t)stream, jobs, n_jobs,
                           points, n_points, rows, n, S, thresh_max, gt, mask, thresh_map, thresh_mask);
        OCRVI_HIP(hipGetLastError());
    }
    return OCRVI_OK;
}
