// The document finder's own mask (include/ocrvi.h, "Document finder"): page -> area-average luminance at the working size -> binomial
// smooth -> histogram -> Otsu threshold + polarity -> 5 x 5 opening -> one bit per working pixel.  Integer arithmetic throughout, doubles
// only in Otsu's score; tests/docfind_ref.py restates every stage in Python integers and must agree to the last bit.  Every entry is
// enqueue-only on its stream: no allocation, no synchronisation.  The contour half runs on the host (dbpost.hip, ocrvi_document_contour).
#include <algorithm>

#include "docfind.h"

namespace ocrvi {
namespace {

// (the bounds, the page table and the grey stage's launch are shared with skew.hip: docfind.h)
constexpr int MAX_SIDE = DOC_MAX_SIDE;
constexpr int MIN_WW = DOC_MIN_WW, MAX_WW = DOC_MAX_WW, MIN_WORK_H = DOC_MIN_WORK_H, MAX_WORK_H = DOC_MAX_WORK_H;
constexpr int GREY_COLS = 8192;      // source columns whose sums one LDS pass of grey_kernel holds

__device__ inline uint32_t luma(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// ---------------------------------------------------------------- 1. grey downscale
// A workgroup per working row (grid-strided).  Per pass over at most GREY_COLS source columns: every thread owns four neighbouring source
// columns and walks the box's rows, so a wave reads 768 contiguous bytes of each row as aligned dwords; the column sums go to LDS, and a
// thread per working pixel adds up its box's columns from there.
__global__ __launch_bounds__(256) void grey_kernel(Pages pages, int work_h, int ww_cap, uint8_t* out_base, size_t out_stride) {
    Geom g;
    if (!page_geom(pages, blockIdx.y, work_h, ww_cap, g)) return;
    __shared__ uint32_t col[GREY_COLS];
    uint8_t* out = out_base + (size_t)blockIdx.y * out_stride;
    const int H = g.H, W = g.W, ww = g.ww, tid = threadIdx.x;
    const uintptr_t page_lo = (uintptr_t)g.ptr, page_hi = page_lo + (size_t)H * W * 3;
    const int64_t fit = ((int64_t)(GREY_COLS - 2) * ww) / W;                 // working columns whose source columns fit one pass
    const int jc = fit < 1 ? 1 : (fit > ww ? ww : (int)fit);
    for (int i = blockIdx.x; i < work_h; i += gridDim.x) {
        const int r0 = (int)((int64_t)i * H / work_h), r1 = max(r0 + 1, (int)((int64_t)(i + 1) * H / work_h));
        for (int j0 = 0; j0 < ww; j0 += jc) {
            const int j1 = min(j0 + jc, ww);
            const int xs = (int)((int64_t)j0 * W / ww);
            const int xe = min(max((int)((int64_t)(j1 - 1) * W / ww) + 1, (int)((int64_t)j1 * W / ww)), xs + GREY_COLS);
            const int groups = (xe - xs + 3) >> 2;
            for (int gi = tid; gi < groups; gi += 256) {
                const int x = xs + 4 * gi, cnt = min(4, xe - x);
                uint32_t acc[4] = {0, 0, 0, 0};
                for (int r = r0; r < r1; ++r) {
                    const uintptr_t a = page_lo + ((size_t)r * W + x) * 3, al = a & ~(uintptr_t)3;
                    if (cnt == 4 && al >= page_lo && al + 16 <= page_hi) {
                        const uint32_t* q = (const uint32_t*)al;
                        const uint32_t sh = (uint32_t)(a & 3), w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
                        const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, sh), d1 = __builtin_amdgcn_alignbyte(w2, w1, sh),
                                       d2 = __builtin_amdgcn_alignbyte(w3, w2, sh);
                        acc[0] += luma(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u);
                        acc[1] += luma(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u);
                        acc[2] += luma((d1 >> 16) & 255u, d1 >> 24, d2 & 255u);
                        acc[3] += luma((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24);
                    } else {
                        const uint8_t* q = (const uint8_t*)a;
                        for (int c = 0; c < cnt; ++c) acc[c] += luma(q[3 * c], q[3 * c + 1], q[3 * c + 2]);
                    }
                }
                for (int c = 0; c < cnt; ++c) col[4 * gi + c] = acc[c];
            }
            __syncthreads();
            for (int j = j0 + tid; j < j1; j += 256) {
                const int c0 = (int)((int64_t)j * W / ww), c1 = min(max(c0 + 1, (int)((int64_t)(j + 1) * W / ww)), xe);
                uint32_t sum = 0;
                for (int c = c0; c < c1; ++c) sum += col[c - xs];
                const uint32_t n = (uint32_t)(r1 - r0) * (uint32_t)(c1 - c0);
                out[(size_t)i * ww + j] = (uint8_t)((sum + n / 2) / n);
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- 2. smooth
// [1 4 6 4 1] x [1 4 6 4 1], replicate border, (sum + 128) >> 8.  64 x 16 outputs per workgroup from an LDS tile with a 2-pixel halo.
constexpr int SM_TW = 64, SM_TH = 16;
__global__ __launch_bounds__(256) void smooth_kernel(Pages pages, int work_h, int ww_cap, const uint8_t* in_base, uint8_t* out_base, size_t stride) {
    Geom g;
    if (!page_geom(pages, blockIdx.z, work_h, ww_cap, g)) return;
    const int ww = g.ww, x0 = blockIdx.x * SM_TW, y0 = blockIdx.y * SM_TH, tid = threadIdx.x;
    if (x0 >= ww) return;
    const uint8_t* in = in_base + (size_t)blockIdx.z * stride;
    uint8_t* out = out_base + (size_t)blockIdx.z * stride;
    __shared__ uint8_t tile[SM_TH + 4][SM_TW + 4];
    __shared__ uint16_t hs[SM_TH + 4][SM_TW];
    for (int k = tid; k < (SM_TH + 4) * (SM_TW + 4); k += 256) {
        const int ry = k / (SM_TW + 4), rx = k - ry * (SM_TW + 4);
        const int y = min(max(y0 + ry - 2, 0), work_h - 1), x = min(max(x0 + rx - 2, 0), ww - 1);
        tile[ry][rx] = in[(size_t)y * ww + x];
    }
    __syncthreads();
    for (int k = tid; k < (SM_TH + 4) * SM_TW; k += 256) {
        const int ry = k / SM_TW, rx = k - ry * SM_TW;
        const uint8_t* t = &tile[ry][rx];
        hs[ry][rx] = (uint16_t)(t[0] + 4 * t[1] + 6 * t[2] + 4 * t[3] + t[4]);
    }
    __syncthreads();
    for (int k = tid; k < SM_TH * SM_TW; k += 256) {
        const int ry = k / SM_TW, rx = k - ry * SM_TW, y = y0 + ry, x = x0 + rx;
        if (y >= work_h || x >= ww) continue;
        const uint32_t s = hs[ry][rx] + 4u * hs[ry + 1][rx] + 6u * hs[ry + 2][rx] + 4u * hs[ry + 3][rx] + hs[ry + 4][rx];
        out[(size_t)y * ww + x] = (uint8_t)((s + 128u) >> 8);
    }
}

// ---------------------------------------------------------------- 3. histogram
// Counts privatised in LDS, then one integer atomic per non-empty bin and workgroup: the result does not depend on the order.
constexpr int HIST_BLOCKS = 32;
__global__ __launch_bounds__(256) void hist_kernel(Pages pages, int work_h, int ww_cap, const uint8_t* in_base, size_t stride, int32_t* hist_base) {
    Geom g;
    if (!page_geom(pages, blockIdx.y, work_h, ww_cap, g)) return;
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const uint8_t* in = in_base + (size_t)blockIdx.y * stride;
    const int total = work_h * g.ww;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < total; k += gridDim.x * 256) atomicAdd(&bins[in[k]], 1u);
    __syncthreads();
    const uint32_t c = bins[threadIdx.x];
    if (c) atomicAdd(hist_base + (size_t)blockIdx.y * 256 + threadIdx.x, (int32_t)c);
}

// ---------------------------------------------------------------- 4 + 5. Otsu and the polarity rule
// One wave per page.  thr[page] = (t, invert, 0, 0); t = -1: no threshold (one non-empty bin), the mask is all zero.
__global__ __launch_bounds__(64) void otsu_kernel(Pages pages, int work_h, int ww_cap, const uint8_t* s_base, size_t stride, const int32_t* hist_base,
                                                  int polarity, int32_t* thr_base) {
    Geom g;
    const int lane = threadIdx.x;
    int32_t* thr = thr_base + (size_t)blockIdx.x * 4;
    if (!page_geom(pages, blockIdx.x, work_h, ww_cap, g)) {
        if (lane < 4) thr[lane] = lane == 0 ? -1 : 0;
        return;
    }
    __shared__ long long cw[256], cm[256];
    __shared__ double score[256];
    __shared__ int best_t;
    const int32_t* hist = hist_base + (size_t)blockIdx.x * 256;
    if (lane == 0) {
        long long w = 0, m = 0;
        for (int v = 0; v < 256; ++v) {
            w += hist[v];
            m += (long long)v * hist[v];
            cw[v] = w;
            cm[v] = m;
        }
    }
    __syncthreads();
    const long long N = cw[255], mT = cm[255];
    for (int t = lane; t < 255; t += 64) {
        const long long w0 = cw[t], m0 = cm[t], w1 = N - w0;
        double sc = -1.0;                                 // skipped
        if (w0 != 0 && w1 != 0) {
            const double d = (double)(mT * w0 - m0 * N);
            sc = __ddiv_rn(__dmul_rn(d, d), __dmul_rn((double)w0, (double)w1));
        }
        score[t] = sc;
    }
    __syncthreads();
    if (lane == 0) {
        int bt = -1;
        double bs = -1.0;
        for (int t = 0; t < 255; ++t)
            if (score[t] > bs) { bs = score[t]; bt = t; }   // strict: the smallest t of maximal score
        best_t = bt;
    }
    __syncthreads();
    const int t = best_t, ww = g.ww;
    int invert = polarity == 2;
    if (t >= 0 && polarity == 0) {                        // the ring: outermost rows and columns, each pixel once
        const uint8_t* S = s_base + (size_t)blockIdx.x * stride;
        int cnt = 0;
        for (int x = lane; x < ww; x += 64) cnt += (S[x] > t) + (S[(size_t)(work_h - 1) * ww + x] > t);
        for (int y = 1 + lane; y < work_h - 1; y += 64) cnt += (S[(size_t)y * ww] > t) + (S[(size_t)y * ww + ww - 1] > t);
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
        cnt = __shfl(cnt, 0, 64);
        invert = 2 * cnt > 2 * ww + 2 * (work_h - 2);
    }
    if (lane < 4) thr[lane] = lane == 0 ? t : (lane == 1 ? (t >= 0 ? invert : 0) : 0);
}

// ---------------------------------------------------------------- 6 .. 8. threshold, 5 x 5 opening, bits
// 32 rows x 8 words (256 pixels) of the mask per workgroup.  B = (S > t) ^ invert as bits in LDS with a 4-row, one-word halo (outside the
// image: 0); each morphological pass is shifts and ANDs / ORs of words.  Bit x & 31 of word y * ((ww + 31) / 32) + (x >> 5).
constexpr int MK_TR = 32, MK_TW = 8;
__device__ inline uint32_t shift_and5(uint32_t l, uint32_t c, uint32_t r) {     // bit k = AND of pixels k-2 .. k+2
    return c & ((c << 1) | (l >> 31)) & ((c << 2) | (l >> 30)) & ((c >> 1) | (r << 31)) & ((c >> 2) | (r << 30));
}
__device__ inline uint32_t shift_or5(uint32_t l, uint32_t c, uint32_t r) {
    return c | ((c << 1) | (l >> 31)) | ((c << 2) | (l >> 30)) | ((c >> 1) | (r << 31)) | ((c >> 2) | (r << 30));
}
__global__ __launch_bounds__(256) void mask_kernel(Pages pages, int work_h, int ww_cap, const uint8_t* s_base, size_t stride, const int32_t* thr_base,
                                                   uint32_t* mask_base, size_t mask_stride) {
    Geom g;
    if (!page_geom(pages, blockIdx.z, work_h, ww_cap, g)) return;
    const int ww = g.ww, wpr = (ww + 31) >> 5, wx0 = blockIdx.x * MK_TW, y0 = blockIdx.y * MK_TR, tid = threadIdx.x;
    if (wx0 >= wpr) return;
    const int32_t* thr = thr_base + (size_t)blockIdx.z * 4;
    const int t = thr[0], invert = thr[1];
    uint32_t* mask = mask_base + (size_t)blockIdx.z * mask_stride;
    constexpr int BW = MK_TW + 2, BR = MK_TR + 8, ER = MK_TR + 4;
    __shared__ uint32_t B[BR][BW], T[BR][BW], E[ER][BW];
    if (t < 0) {                                           // no threshold: all zero
        for (int k = tid; k < MK_TR * MK_TW; k += 256) {
            const int y = y0 + k / MK_TW, wx = wx0 + k % MK_TW;
            if (y < work_h && wx < wpr) mask[(size_t)y * wpr + wx] = 0;
        }
        return;
    }
    const uint8_t* S = s_base + (size_t)blockIdx.z * stride;
    const int lane = tid & 63, wave = tid >> 6;
    for (int seg = wave; seg < BR * (BW / 2); seg += 4) {  // 64 pixels per ballot = two words
        const int ry = seg / (BW / 2), sx = seg - ry * (BW / 2);
        const int y = y0 + ry - 4, x = (wx0 - 1) * 32 + sx * 64 + lane;
        bool v = false;
        if (y >= 0 && y < work_h && x >= 0 && x < ww) v = ((int)S[(size_t)y * ww + x] > t) != (invert != 0);
        const unsigned long long b = __ballot(v);
        if (lane == 0) {
            B[ry][2 * sx] = (uint32_t)b;
            B[ry][2 * sx + 1] = (uint32_t)(b >> 32);
        }
    }
    __syncthreads();
    for (int k = tid; k < BR * BW; k += 256) {             // erosion along x (the words beyond the halo are background)
        const int ry = k / BW, rx = k - ry * BW;
        T[ry][rx] = shift_and5(rx ? B[ry][rx - 1] : 0u, B[ry][rx], rx + 1 < BW ? B[ry][rx + 1] : 0u);
    }
    __syncthreads();
    for (int k = tid; k < ER * BW; k += 256) {             // erosion along y: E row r = image row y0 + r - 2
        const int ry = k / BW, rx = k - ry * BW;
        E[ry][rx] = T[ry][rx] & T[ry + 1][rx] & T[ry + 2][rx] & T[ry + 3][rx] & T[ry + 4][rx];
    }
    __syncthreads();
    for (int k = tid; k < ER * BW; k += 256) {             // dilation along x
        const int ry = k / BW, rx = k - ry * BW;
        T[ry][rx] = shift_or5(rx ? E[ry][rx - 1] : 0u, E[ry][rx], rx + 1 < BW ? E[ry][rx + 1] : 0u);
    }
    __syncthreads();
    for (int k = tid; k < MK_TR * MK_TW; k += 256) {       // dilation along y, padding bits cleared
        const int ry = k / MK_TW, rx = k - ry * MK_TW, y = y0 + ry, wx = wx0 + rx;
        if (y >= work_h || wx >= wpr) continue;
        uint32_t d = T[ry][rx + 1] | T[ry + 1][rx + 1] | T[ry + 2][rx + 1] | T[ry + 3][rx + 1] | T[ry + 4][rx + 1];
        if (wx == wpr - 1 && (ww & 31)) d &= (1u << (ww & 31)) - 1u;
        mask[(size_t)y * wpr + wx] = d;
    }
}

// ---------------------------------------------------------------- host side
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
struct Layout {
    size_t plane, g, s, hist, thr, total;
};
inline Layout layout(int n, int work_h, int ww_cap) {
    Layout l;
    l.plane = align256((size_t)work_h * ww_cap);
    l.g = 0;
    l.s = l.g + l.plane * n;
    l.hist = l.s + l.plane * n;
    l.thr = l.hist + align256((size_t)n * 256 * sizeof(int32_t));
    l.total = l.thr + align256((size_t)n * 4 * sizeof(int32_t));
    return l;
}

}  // namespace

int check_work(const char* what, int device, int work_h, int ww) {
    OCRVI_CHECK(device >= 0, OCRVI_EINVAL, "%s: device %d", what, device);
    OCRVI_CHECK(work_h >= MIN_WORK_H && work_h <= MAX_WORK_H, OCRVI_EINVAL, "%s: work_h = %d (%d .. %d)", what, work_h, MIN_WORK_H, MAX_WORK_H);
    OCRVI_CHECK(ww >= MIN_WW && ww <= MAX_WW, OCRVI_EINVAL, "%s: a working width of %d (%d .. %d)", what, ww, MIN_WW, MAX_WW);
    return OCRVI_OK;
}

int launch_grey(const Pages& p, int n, int work_h, int ww_cap, uint8_t* out, size_t stride, hipStream_t st) {
    ProfScope ps("doc_grey", 0.0, 0.0, st);   // (the byte counts stay 0: the sizes are in the table, on the device)
    hipLaunchKernelGGL(grey_kernel, dim3(work_h, n), dim3(256), 0, st, p, work_h, ww_cap, out, stride);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

namespace {
int launch_smooth(const Pages& p, int n, int work_h, int ww_cap, const uint8_t* in, uint8_t* out, size_t stride, hipStream_t st) {
    ProfScope ps("doc_smooth", 0.0, 0.0, st);
    hipLaunchKernelGGL(smooth_kernel, dim3((ww_cap + SM_TW - 1) / SM_TW, (work_h + SM_TH - 1) / SM_TH, n), dim3(256), 0, st, p, work_h, ww_cap, in, out,
                       stride);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
int launch_hist(const Pages& p, int n, int work_h, int ww_cap, const uint8_t* in, size_t stride, int32_t* hist, hipStream_t st) {
    OCRVI_HIP(hipMemsetAsync(hist, 0, (size_t)n * 256 * sizeof(int32_t), st));
    ProfScope ps("doc_hist", 0.0, 0.0, st);
    hipLaunchKernelGGL(hist_kernel, dim3(HIST_BLOCKS, n), dim3(256), 0, st, p, work_h, ww_cap, in, stride, hist);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
int launch_otsu(const Pages& p, int n, int work_h, int ww_cap, const uint8_t* s, size_t stride, const int32_t* hist, int polarity, int32_t* thr,
                hipStream_t st) {
    ProfScope ps("doc_otsu", 0.0, 0.0, st);
    hipLaunchKernelGGL(otsu_kernel, dim3(n), dim3(64), 0, st, p, work_h, ww_cap, s, stride, hist, polarity, thr);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
int launch_mask(const Pages& p, int n, int work_h, int ww_cap, const uint8_t* s, size_t stride, const int32_t* thr, uint32_t* mask, size_t mask_stride,
                hipStream_t st) {
    const int wpr = (ww_cap + 31) / 32;
    ProfScope ps("doc_mask", 0.0, 0.0, st);
    hipLaunchKernelGGL(mask_kernel, dim3((wpr + MK_TW - 1) / MK_TW, (work_h + MK_TR - 1) / MK_TR, n), dim3(256), 0, st, p, work_h, ww_cap, s, stride, thr,
                       mask, mask_stride);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

}  // namespace
}  // namespace ocrvi

using namespace ocrvi;

extern "C" int ocrvi_doc_working_size(int h, int w, int work_h, int32_t* ww, double* ratio) {
    OCRVI_CHECK(ww && ratio, OCRVI_EINVAL, "doc_working_size: null pointer");
    OCRVI_CHECK(h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE, OCRVI_EINVAL, "doc_working_size: a %d x %d page (sides 1 .. %d)", h, w, MAX_SIDE);
    OCRVI_CHECK(work_h >= MIN_WORK_H && work_h <= MAX_WORK_H, OCRVI_EINVAL, "doc_working_size: work_h = %d (%d .. %d)", work_h, MIN_WORK_H, MAX_WORK_H);
    *ratio = (double)h / (double)work_h;
    *ww = working_width(h, w, work_h);
    OCRVI_CHECK(*ww >= MIN_WW && *ww <= MAX_WW, OCRVI_EINVAL, "doc_working_size: a %d x %d page at %d working rows is %d pixels wide (%d .. %d)", h, w,
                work_h, *ww, MIN_WW, MAX_WW);
    return OCRVI_OK;
}

extern "C" int ocrvi_doc_mask_sizes(int n, int work_h, int ww_cap, size_t* workspace_bytes, size_t* mask_words) {
    OCRVI_CHECK(workspace_bytes && mask_words, OCRVI_EINVAL, "doc_mask_sizes: null pointer");
    OCRVI_CHECK(n >= 1 && n <= 65535, OCRVI_EINVAL, "doc_mask_sizes: %d pages (1 .. 65535)", n);
    OCRVI_TRY(check_work("doc_mask_sizes", 0, work_h, ww_cap));
    *workspace_bytes = layout(n, work_h, ww_cap).total;
    *mask_words = (size_t)work_h * ((ww_cap + 31) / 32);
    return OCRVI_OK;
}

extern "C" int ocrvi_doc_grey_u8(int device, const uint8_t* src, int h, int w, int work_h, uint8_t* dst, void* stream) {
    int32_t ww;
    double ratio;
    OCRVI_CHECK(src && dst, OCRVI_EINVAL, "doc_grey_u8: null pointer");
    OCRVI_TRY(ocrvi_doc_working_size(h, w, work_h, &ww, &ratio));
    OCRVI_TRY(check_work("doc_grey_u8", device, work_h, ww));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_grey(Pages{nullptr, src, h, w, ww}, 1, work_h, ww, dst, 0, (hipStream_t)stream);
}

extern "C" int ocrvi_doc_smooth_u8(int device, const uint8_t* src, int work_h, int ww, uint8_t* dst, void* stream) {
    OCRVI_CHECK(src && dst && src != dst, OCRVI_EINVAL, "doc_smooth_u8: null pointer or dst == src");
    OCRVI_TRY(check_work("doc_smooth_u8", device, work_h, ww));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_smooth(Pages{nullptr, nullptr, work_h, ww, ww}, 1, work_h, ww, src, dst, 0, (hipStream_t)stream);
}

extern "C" int ocrvi_doc_histogram(int device, const uint8_t* src, int work_h, int ww, int32_t* hist, void* stream) {
    OCRVI_CHECK(src && hist, OCRVI_EINVAL, "doc_histogram: null pointer");
    OCRVI_TRY(check_work("doc_histogram", device, work_h, ww));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_hist(Pages{nullptr, nullptr, work_h, ww, ww}, 1, work_h, ww, src, 0, hist, (hipStream_t)stream);
}

extern "C" int ocrvi_doc_otsu(int device, const uint8_t* smooth, const int32_t* hist, int work_h, int ww, int polarity, int32_t* thr, void* stream) {
    OCRVI_CHECK(smooth && hist && thr, OCRVI_EINVAL, "doc_otsu: null pointer");
    OCRVI_CHECK(polarity >= OCRVI_DOC_AUTO && polarity <= OCRVI_DOC_DARK, OCRVI_EINVAL, "doc_otsu: polarity %d", polarity);
    OCRVI_TRY(check_work("doc_otsu", device, work_h, ww));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_otsu(Pages{nullptr, nullptr, work_h, ww, ww}, 1, work_h, ww, smooth, 0, hist, polarity, thr, (hipStream_t)stream);
}

extern "C" int ocrvi_doc_mask_bits(int device, const uint8_t* smooth, int work_h, int ww, const int32_t* thr, uint32_t* bits, void* stream) {
    OCRVI_CHECK(smooth && thr && bits, OCRVI_EINVAL, "doc_mask_bits: null pointer");
    OCRVI_TRY(check_work("doc_mask_bits", device, work_h, ww));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_mask(Pages{nullptr, nullptr, work_h, ww, ww}, 1, work_h, ww, smooth, 0, thr, bits, 0, (hipStream_t)stream);
}

extern "C" int ocrvi_doc_mask_pages(int device, const int64_t* pages, int n, int work_h, int ww_cap, int polarity, uint32_t* masks, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    OCRVI_CHECK(pages && masks && workspace, OCRVI_EINVAL, "doc_mask_pages: null pointer");
    OCRVI_CHECK(n >= 1 && n <= 65535, OCRVI_EINVAL, "doc_mask_pages: %d pages (1 .. 65535)", n);
    OCRVI_CHECK(polarity >= OCRVI_DOC_AUTO && polarity <= OCRVI_DOC_DARK, OCRVI_EINVAL, "doc_mask_pages: polarity %d", polarity);
    OCRVI_TRY(check_work("doc_mask_pages", device, work_h, ww_cap));
    const Layout l = layout(n, work_h, ww_cap);
    OCRVI_CHECK(workspace_bytes >= l.total, OCRVI_ENOMEM, "doc_mask_pages: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
    OCRVI_CHECK(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)masks & 3) == 0, OCRVI_EINVAL, "doc_mask_pages: workspace or masks misaligned");
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)workspace;
    uint8_t *G = ws + l.g, *S = ws + l.s;
    int32_t *hist = (int32_t*)(ws + l.hist), *thr = (int32_t*)(ws + l.thr);
    const size_t mask_words = (size_t)work_h * ((ww_cap + 31) / 32);
    const Pages p{pages, nullptr, 0, 0, 0};
    OCRVI_HIP(hipMemsetAsync(masks, 0, (size_t)n * mask_words * sizeof(uint32_t), st));   // pages that are not processed stay all zero
    OCRVI_TRY(launch_grey(p, n, work_h, ww_cap, G, l.plane, st));
    OCRVI_TRY(launch_smooth(p, n, work_h, ww_cap, G, S, l.plane, st));
    OCRVI_TRY(launch_hist(p, n, work_h, ww_cap, S, l.plane, hist, st));
    OCRVI_TRY(launch_otsu(p, n, work_h, ww_cap, S, l.plane, hist, polarity, thr, st));
    return launch_mask(p, n, work_h, ww_cap, S, l.plane, thr, masks, mask_words, st);
}
