// Device-side pre-processing on the e2e path:
//  * detection input: uint8 HWC -> /255 (float32) -> (x - mean)/std in float64 -> float32 NCHW  (pipeline2.py:312-314)
//  * recognition input: crop (src/det/test.py:123-130) -> resize to the target height keeping aspect, squash if wider than
//    the target, right-pad with 255 -> /255, ImageNet normalise in float32 -> NCHW  (pipeline2.py:92-128)
// The resize restates OpenCV's 8-bit INTER_LINEAR (cv2.resize default): 11-bit fixed-point coefficients, horizontal pass
// in int32, vertical pass ((b0*(r0>>4))>>16 + (b1*(r1>>4))>>16 + 2) >> 2, and the exact-2x-downscale special case that
// OpenCV routes to the 2x2 box filter.  cv2 is absent from the build container: parity with cv2 itself is UNPINNED; the
// CPU oracle (oracle/preproc_cpu.py) restates the same published algorithm independently in numpy.
#include <math.h>

#include <algorithm>
#include <cmath>

#include "common.h"

namespace ocrvi {

__constant__ double c_mean[3] = {0.485, 0.456, 0.406};
__constant__ double c_std[3] = {0.229, 0.224, 0.225};

__global__ void normalize_u8_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int N, int H, int W) {
    const size_t plane = (size_t)H * W, total = (size_t)N * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t n = i / plane, p = i % plane;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = (float)img[i * 3 + c] / 255.0f;
            out[(n * 3 + c) * plane + p] = (float)(((double)v - c_mean[c]) / c_std[c]);
        }
    }
}

struct AxisCoef { int s0, s1; int a0, a1; };
// OpenCV resizeLinear coefficient for destination index d on an axis of src length `ssize`, dst length `dsize`.
__device__ __forceinline__ AxisCoef axis_coef(int d, int ssize, int dsize) {
    const double scale = (double)ssize / (double)dsize;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= ssize - 1) { s = ssize - 1; f = 0.f; }
    AxisCoef c;
    c.s0 = s;
    c.s1 = min(s + 1, ssize - 1);
    c.a0 = __float2int_rn((1.f - f) * 2048.f);
    c.a1 = __float2int_rn(f * 2048.f);
    return c;
}

__global__ void crop_resize_normalize_kernel(const uint8_t* __restrict__ images, int n_img, int H, int W, const int32_t* __restrict__ boxes,
                                             int B, int oh, int ow, float* __restrict__ out) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const size_t total = (size_t)B * oh * ow;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % ow);
        const size_t t = i / ow;
        const int y = (int)(t % oh), b = (int)(t / oh);
        const int32_t* bx = boxes + (size_t)b * 5;
        const int img = bx[0];
        // clamp the rectangle to the page exactly as crop_image does (src/det/test.py:126-129: x = max(0, x); bw = min(bw, w - x) --
        // the width is NOT reduced by the shift).  Boxes live in HBM, so the host cannot validate them; a rectangle that ends up
        // empty takes the zero-tensor path below
        const int cx = max(bx[1], 0), cy = max(bx[2], 0);
        const int cw = min(bx[3], W - cx), ch = min(bx[4], H - cy);
        float* o = out + ((size_t)b * 3 * oh + y) * ow + x;
        const size_t plane = (size_t)oh * ow;
        if (cw <= 0 || ch <= 0 || img < 0 || img >= n_img) {  // empty crop -> zeros tensor (pipeline2.py:154-156)
            o[0] = o[plane] = o[2 * plane] = 0.f;
            continue;
        }
        // new_w = int(w * (target_h / h))  (pipeline2.py:101-102), computed in double like Python floats
        int new_w = (int)((double)cw * ((double)oh / (double)ch));
        if (new_w > ow) new_w = ow;   // squash (pipeline2.py:104-105)
        if (new_w < 1) new_w = 1;
        int v[3] = {255, 255, 255};
        if (x < new_w) {
            const uint8_t* src = images + ((size_t)img * H + cy) * W * 3 + (size_t)cx * 3;
            const size_t rs = (size_t)W * 3;
            if (cw == 2 * new_w && ch == 2 * oh) {  // OpenCV: exact 2x decimation with INTER_LINEAR runs the 2x2 area filter
                const uint8_t* p0 = src + (size_t)(2 * y) * rs + (size_t)(2 * x) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = (p0[c] + p0[3 + c] + p0[rs + c] + p0[rs + 3 + c] + 2) >> 2;
            } else {
                const AxisCoef ax = axis_coef(x, cw, new_w), ay = axis_coef(y, ch, oh);
                const uint8_t *r0 = src + (size_t)ay.s0 * rs, *r1 = src + (size_t)ay.s1 * rs;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int h0 = r0[ax.s0 * 3 + c] * ax.a0 + r0[ax.s1 * 3 + c] * ax.a1;
                    const int h1 = r1[ax.s0 * 3 + c] * ax.a0 + r1[ax.s1 * 3 + c] * ax.a1;
                    v[c] = (((ay.a0 * (h0 >> 4)) >> 16) + ((ay.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane] = ((float)v[c] / 255.0f - mean[c]) / stdv[c];
    }
}

// cv2.resize(img, (dw, dh)) with the default INTER_LINEAR on uint8 HWC (resize_image_for_det, pipeline2.py:33-40)
__global__ void resize_u8_kernel(const uint8_t* __restrict__ src, int sh, int sw, uint8_t* __restrict__ dst, int dh, int dw) {
    const size_t total = (size_t)dh * dw;
    const bool area2 = (sw == 2 * dw && sh == 2 * dh);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % dw), y = (int)(i / dw);
        const size_t rs = (size_t)sw * 3;
        int v[3];
        if (area2) {
            const uint8_t* p0 = src + (size_t)(2 * y) * rs + (size_t)(2 * x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (p0[c] + p0[3 + c] + p0[rs + c] + p0[rs + 3 + c] + 2) >> 2;
        } else {
            const AxisCoef ax = axis_coef(x, sw, dw), ay = axis_coef(y, sh, dh);
            const uint8_t *r0 = src + (size_t)ay.s0 * rs, *r1 = src + (size_t)ay.s1 * rs;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int h0 = r0[ax.s0 * 3 + c] * ax.a0 + r0[ax.s1 * 3 + c] * ax.a1;
                const int h1 = r1[ax.s0 * 3 + c] * ax.a0 + r1[ax.s1 * 3 + c] * ax.a1;
                v[c] = (((ay.a0 * (h0 >> 4)) >> 16) + ((ay.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[i * 3 + c] = (uint8_t)v[c];
    }
}


// ---------------------------------------------------------------- pages of different sizes through a device page table
// Page table: int64 [n][OCRVI_PAGE_ENTRY] = (device address of the uint8 HWC page, height, width, reserved).  The addresses are read
// when the kernel runs, so a captured graph stays valid when the pages move and only the table's contents are rewritten.
struct PageRef { const uint8_t* p; int h, w; };
__device__ __forceinline__ PageRef load_page(const int64_t* __restrict__ table, int i) {
    const int64_t* e = table + (size_t)i * OCRVI_PAGE_ENTRY;
    PageRef r;
    r.p = (const uint8_t*)(uintptr_t)e[0];
    r.h = (int)e[1];
    r.w = (int)e[2];
    if (!r.p || r.h <= 0 || r.w <= 0) r.h = r.w = 0;
    return r;
}

// resize_u8_kernel's value of destination pixel (x, y) of an sh x sw page resized to dh x dw, channel by channel
__device__ __forceinline__ void resized_px(const uint8_t* __restrict__ src, int sh, int sw, int dh, int dw, int x, const AxisCoef& ay, int y,
                                           bool area2, int v[3]) {
    const size_t rs = (size_t)sw * 3;
    if (area2) {
        const uint8_t* p0 = src + (size_t)(2 * y) * rs + (size_t)(2 * x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (p0[c] + p0[3 + c] + p0[rs + c] + p0[rs + 3 + c] + 2) >> 2;
    } else {
        const AxisCoef ax = axis_coef(x, sw, dw);
        const uint8_t *r0 = src + (size_t)ay.s0 * rs, *r1 = src + (size_t)ay.s1 * rs;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int h0 = r0[ax.s0 * 3 + c] * ax.a0 + r0[ax.s1 * 3 + c] * ax.a1;
            const int h1 = r1[ax.s0 * 3 + c] * ax.a0 + r1[ax.s1 * 3 + c] * ax.a1;
            v[c] = (((ay.a0 * (h0 >> 4)) >> 16) + ((ay.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
        }
    }
}

// resize_u8_kernel then normalize_u8_kernel, fused, for n pages of their own sizes into one [n,3,H,W] batch.  One thread writes 4
// consecutive pixels of a row: a 16-byte store to each of the 3 planes (W % 4 == 0), so a wave writes 1 KiB of each plane back to back.
// An identity-size page (the resize is then exact: a0 = 2048, a1 = 0) is read as three 4-byte words per thread when it is aligned.
__global__ void resize_normalize_pages_kernel(const int64_t* __restrict__ table, int n, int H, int W, float* __restrict__ out) {
    const int W4 = W >> 2;
    const size_t plane = (size_t)H * W, quads = (size_t)H * W4, total = (size_t)n * quads;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int pg = (int)(i / quads);
        const size_t r = i - (size_t)pg * quads;
        const int y = (int)(r / W4), x0 = (int)(r - (size_t)y * W4) * 4;
        const PageRef src = load_page(table, pg);
        int v[4][3];
        if (src.h == 0) {                // an invalid table entry: zero-valued pixels, never a read
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k][0] = v[k][1] = v[k][2] = 0;
        } else if (src.h == H && src.w == W) {
            const uint8_t* p = src.p + ((size_t)y * W + x0) * 3;
            if ((((uintptr_t)p) & 3) == 0) {
                const uint32_t w0 = ((const uint32_t*)p)[0], w1 = ((const uint32_t*)p)[1], w2 = ((const uint32_t*)p)[2];
                const uint32_t b[12] = {w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, w0 >> 24, w1 & 255, (w1 >> 8) & 255,
                                        (w1 >> 16) & 255, w1 >> 24, w2 & 255, (w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24};
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k][0] = b[3 * k], v[k][1] = b[3 * k + 1], v[k][2] = b[3 * k + 2];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k][0] = p[3 * k], v[k][1] = p[3 * k + 1], v[k][2] = p[3 * k + 2];
            }
        } else {
            const bool area2 = (src.w == 2 * W && src.h == 2 * H);
            const AxisCoef ay = axis_coef(y, src.h, H);
#pragma unroll
            for (int k = 0; k < 4; ++k) resized_px(src.p, src.h, src.w, H, W, x0 + k, ay, y, area2, v[k]);
        }
        float* o = out + (size_t)pg * 3 * plane + (size_t)y * W + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float4 f;
            f.x = (float)(((double)((float)v[0][c] / 255.0f) - c_mean[c]) / c_std[c]);
            f.y = (float)(((double)((float)v[1][c] / 255.0f) - c_mean[c]) / c_std[c]);
            f.z = (float)(((double)((float)v[2][c] / 255.0f) - c_mean[c]) / c_std[c]);
            f.w = (float)(((double)((float)v[3][c] / 255.0f) - c_mean[c]) / c_std[c]);
            *(float4*)(o + (size_t)c * plane) = f;
        }
    }
}

// crop_resize_normalize_kernel with each rectangle's page taken from the page table: boxes int32 [B,5] = (table index, x, y, w, h)
__global__ void crop_resize_normalize_pages_kernel(const int64_t* __restrict__ table, int n_pages, const int32_t* __restrict__ boxes, int B,
                                                   int oh, int ow, float* __restrict__ out) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const size_t total = (size_t)B * oh * ow;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % ow);
        const size_t t = i / ow;
        const int y = (int)(t % oh), b = (int)(t / oh);
        const int32_t* bx = boxes + (size_t)b * 5;
        const int img = bx[0];
        float* o = out + ((size_t)b * 3 * oh + y) * ow + x;
        const size_t plane = (size_t)oh * ow;
        const PageRef pr = (img >= 0 && img < n_pages) ? load_page(table, img) : PageRef{nullptr, 0, 0};
        const int H = pr.h, W = pr.w;
        // clamping exactly as crop_resize_normalize_kernel (crop_image, src/det/test.py:126-129)
        const int cx = max(bx[1], 0), cy = max(bx[2], 0);
        const int cw = min(bx[3], W - cx), ch = min(bx[4], H - cy);
        if (cw <= 0 || ch <= 0 || H == 0) {  // empty crop, index out of range or invalid entry -> zeros tensor (pipeline2.py:154-156)
            o[0] = o[plane] = o[2 * plane] = 0.f;
            continue;
        }
        int new_w = (int)((double)cw * ((double)oh / (double)ch));
        if (new_w > ow) new_w = ow;   // squash (pipeline2.py:104-105)
        if (new_w < 1) new_w = 1;
        int v[3] = {255, 255, 255};
        if (x < new_w) {
            const uint8_t* src = pr.p + ((size_t)cy * W) * 3 + (size_t)cx * 3;
            const size_t rs = (size_t)W * 3;
            if (cw == 2 * new_w && ch == 2 * oh) {
                const uint8_t* p0 = src + (size_t)(2 * y) * rs + (size_t)(2 * x) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = (p0[c] + p0[3 + c] + p0[rs + c] + p0[rs + 3 + c] + 2) >> 2;
            } else {
                const AxisCoef ax = axis_coef(x, cw, new_w), ay = axis_coef(y, ch, oh);
                const uint8_t *r0 = src + (size_t)ay.s0 * rs, *r1 = src + (size_t)ay.s1 * rs;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int h0 = r0[ax.s0 * 3 + c] * ax.a0 + r0[ax.s1 * 3 + c] * ax.a1;
                    const int h1 = r1[ax.s0 * 3 + c] * ax.a0 + r1[ax.s1 * 3 + c] * ax.a1;
                    v[c] = (((ay.a0 * (h0 >> 4)) >> 16) + ((ay.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane] = ((float)v[c] / 255.0f - mean[c]) / stdv[c];
    }
}

// ---------------------------------------------------------------- four-point rectification (src/preprocess/scanner.py:29-53)
// The perspective warp behind four_point_transform's cv2.warpPerspective call (scanner.py:51), as include/ocrvi.h states it: the inverse
// map in IEEE double without fused multiply-adds, source coordinates quantised to 1/32 pixel, 15-bit bilinear weights, constant border 0.
// OpenCV's own code differs between versions and block sizes and cv2 is absent from the build container: parity with cv2 is UNPINNED,
// as for the resize above; tests/warp_ref.py restates the same definition in numpy and the kernel is bit-equal to it.
struct WarpMat { double m[9]; };

// one source coordinate in 1/32 pixel: rint(clamp(v0 * s)) as int32 (a NaN product counts as the lower bound)
__device__ __forceinline__ int warp_coord(double v0, double s) {
#pragma clang fp contract(off)
    double v = v0 * s;
    if (!(v >= -2147483648.0)) v = -2147483648.0;
    if (v > 2147483647.0) v = 2147483647.0;
    return (int)rint(v);     // round half to even; exact after the clamp
}

// destination pixel (x, y) of the warp of a valid sh x sw page: the three channel values
__device__ __forceinline__ void warp_px(const uint8_t* __restrict__ src, int sh, int sw, const WarpMat& M, int x, int y, int v[3]) {
#pragma clang fp contract(off)
    const double dx = (double)x, dy = (double)y;
    const double X0 = (M.m[0] * dx + M.m[1] * dy) + M.m[2];
    const double Y0 = (M.m[3] * dx + M.m[4] * dy) + M.m[5];
    const double W0 = (M.m[6] * dx + M.m[7] * dy) + M.m[8];
    const double s = (W0 != 0.0) ? 32.0 / W0 : 0.0;
    const int X = warp_coord(X0, s), Y = warp_coord(Y0, s);
    const int sx = X >> 5, sy = Y >> 5, ax = X & 31, ay = Y & 31;
    // the range is decided on the integers (sx is up to +-2^26) before any address is formed; sx + 1 and sy + 1 cannot overflow
    const bool x0in = (unsigned)sx < (unsigned)sw, x1in = (unsigned)(sx + 1) < (unsigned)sw;
    const bool y0in = (unsigned)sy < (unsigned)sh, y1in = (unsigned)(sy + 1) < (unsigned)sh;
    v[0] = v[1] = v[2] = 0;
    if (!((x0in || x1in) && (y0in || y1in))) return;
    const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
    const size_t rs = (size_t)sw * 3;
    int acc[3] = {16384, 16384, 16384};
    if (y0in) {
        const uint8_t* r = src + (size_t)sy * rs;
        if (x0in) { const uint8_t* p = r + (size_t)sx * 3; acc[0] += w00 * p[0]; acc[1] += w00 * p[1]; acc[2] += w00 * p[2]; }
        if (x1in) { const uint8_t* p = r + (size_t)(sx + 1) * 3; acc[0] += w01 * p[0]; acc[1] += w01 * p[1]; acc[2] += w01 * p[2]; }
    }
    if (y1in) {
        const uint8_t* r = src + (size_t)(sy + 1) * rs;
        if (x0in) { const uint8_t* p = r + (size_t)sx * 3; acc[0] += w10 * p[0]; acc[1] += w10 * p[1]; acc[2] += w10 * p[2]; }
        if (x1in) { const uint8_t* p = r + (size_t)(sx + 1) * 3; acc[0] += w11 * p[0]; acc[1] += w11 * p[1]; acc[2] += w11 * p[2]; }
    }
    v[0] = acc[0] >> 15; v[1] = acc[1] >> 15; v[2] = acc[2] >> 15;
}

// One page: groups first, first + stride, ... of 4 consecutive pixels of the destination taken as one flat run of dh * dw pixels (a
// group may cross a row end).  A group is 12 bytes at dst + 12 g, so whether it can go out as three 4-byte words depends on the page's
// base address alone, whatever the row length: a wave then writes 768 contiguous bytes.  A base that is no multiple of 4, and the
// last, partial group, are written byte by byte.  sh == 0 (an invalid source) writes zeros.
__device__ __forceinline__ void warp_page(const uint8_t* __restrict__ src, int sh, int sw, const WarpMat& M, uint8_t* __restrict__ dst, int dh,
                                          int dw, size_t first, size_t stride) {
    const size_t npx = (size_t)dh * dw, groups = (npx + 3) >> 2;
    const bool words = (((uintptr_t)dst) & 3) == 0;
    for (size_t g = first; g < groups; g += stride) {
        const size_t i0 = g * 4;
        int y = (int)(i0 / (size_t)dw), x = (int)(i0 - (size_t)y * dw);
        const int cnt = (int)min((size_t)4, npx - i0);
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int v[3] = {0, 0, 0};
            if (k < cnt && sh != 0) warp_px(src, sh, sw, M, x, y, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) w[(3 * k + c) >> 2] |= (uint32_t)v[c] << (8 * ((3 * k + c) & 3));
            if (++x == dw) { x = 0; ++y; }
        }
        uint8_t* o = dst + i0 * 3;
        if (words && cnt == 4) {
            ((uint32_t*)o)[0] = w[0]; ((uint32_t*)o)[1] = w[1]; ((uint32_t*)o)[2] = w[2];
        } else {
            for (int j = 0; j < cnt * 3; ++j) o[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

__global__ void warp_perspective_u8_kernel(const uint8_t* __restrict__ src, int sh, int sw, WarpMat M, uint8_t* __restrict__ dst, int dh, int dw) {
    warp_page(src, sh, sw, M, dst, dh, dw, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// blockIdx.y = page: both tables and the page's matrix are read here, when the kernel runs
__global__ void warp_perspective_pages_kernel(const int64_t* __restrict__ src_table, const int64_t* __restrict__ dst_table,
                                              const double* __restrict__ m_inv) {
    const int pg = blockIdx.y;
    const PageRef d = load_page(dst_table, pg);
    if (d.h == 0) return;                          // an invalid destination entry is skipped, never dereferenced
    const PageRef s = load_page(src_table, pg);    // invalid source: h = 0 -> the destination is filled with 0
    WarpMat M;
#pragma unroll
    for (int k = 0; k < 9; ++k) M.m[k] = m_inv[(size_t)pg * 9 + k];
    warp_page(s.p, s.h, s.w, M, (uint8_t*)d.p, d.h, d.w, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

}  // namespace ocrvi

using namespace ocrvi;

extern "C" int ocrvi_resize_u8(int device, const uint8_t* src, int src_h, int src_w, uint8_t* dst, int dst_h, int dst_w, void* stream) {
    OCRVI_CHECK(src && dst && src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0, OCRVI_EINVAL, "resize_u8: bad argument");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t total = (size_t)dst_h * dst_w;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(resize_u8_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, src_h, src_w, dst, dst_h, dst_w);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

extern "C" int ocrvi_normalize_u8(int device, const uint8_t* images, int N, int H, int W, float* out, void* stream) {
    OCRVI_CHECK(images && out && N > 0 && H > 0 && W > 0, OCRVI_EINVAL, "normalize_u8: bad argument");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t total = (size_t)N * H * W;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(normalize_u8_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, images, out, N, H, W);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

extern "C" int ocrvi_crop_resize_normalize(int device, const uint8_t* images, int n_img, int H, int W, const int32_t* boxes, int B, int out_h,
                                           int out_w, float* out, void* stream) {
    OCRVI_CHECK(images && boxes && out && n_img > 0 && B > 0 && out_h > 0 && out_w > 0, OCRVI_EINVAL, "crop_resize_normalize: bad argument");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t total = (size_t)B * out_h * out_w;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(crop_resize_normalize_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, images, n_img, H, W, boxes, B, out_h, out_w, out);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

extern "C" int ocrvi_resize_normalize_pages(int device, const int64_t* pages, int n, int H, int W, float* out, void* stream) {
    OCRVI_CHECK(pages && out && n > 0 && H > 0 && W > 0 && W % 4 == 0 && (((uintptr_t)out) & 15) == 0, OCRVI_EINVAL,
                "resize_normalize_pages: bad argument (W must be a multiple of 4, out 16-byte aligned)");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t total = (size_t)n * H * (W / 4);
    const int grid = (int)std::min<size_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(resize_normalize_pages_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, pages, n, H, W, out);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

extern "C" int ocrvi_crop_resize_normalize_pages(int device, const int64_t* pages, int n_pages, const int32_t* boxes, int B, int out_h, int out_w,
                                                 float* out, void* stream) {
    OCRVI_CHECK(pages && boxes && out && n_pages > 0 && B > 0 && out_h > 0 && out_w > 0, OCRVI_EINVAL, "crop_resize_normalize_pages: bad argument");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t total = (size_t)B * out_h * out_w;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(crop_resize_normalize_pages_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, pages, n_pages, boxes, B, out_h, out_w, out);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

// ---------------------------------------------------------------- four-point rectification: host geometry and the two warp entries
// src/preprocess/scanner.py:13-53 restated: order_points (:13-27), the output size from the float32 side lengths (:36-42), the destination
// corners (:44-48) and cv2.getPerspectiveTransform (:50) as the 8 x 8 system of the four correspondences with h22 = 1.
static bool three_collinear(const double (*p)[2]) {
    for (int a = 0; a < 4; ++a) {          // the triple that leaves corner a out
        const double* q[3];
        for (int i = 0, k = 0; i < 4; ++i) if (i != a) q[k++] = p[i];
        const double ux = q[1][0] - q[0][0], uy = q[1][1] - q[0][1], vx = q[2][0] - q[0][0], vy = q[2][1] - q[0][1];
        const double cross = ux * vy - uy * vx;
        if (!(fabs(cross) > 1e-12 * sqrt((ux * ux + uy * uy) * (vx * vx + vy * vy)))) return true;
    }
    return false;
}

extern "C" int ocrvi_four_point_transform(const double* pts, double* m_fwd, double* m_inv, int32_t* out_w, int32_t* out_h) {
#pragma clang fp contract(off)
    OCRVI_CHECK(pts && m_inv && out_w && out_h, OCRVI_EINVAL, "four_point_transform: null argument");
    for (int i = 0; i < 8; ++i) OCRVI_CHECK(std::isfinite(pts[i]), OCRVI_EINVAL, "four_point_transform: corner %d is not finite", i / 2);
    // order_points: sums and differences in float64, first index wins ties (numpy argmin / argmax), corners kept as float32
    int tl = 0, br = 0, tr = 0, bl = 0;
    for (int i = 1; i < 4; ++i) {
        const double s = pts[2 * i] + pts[2 * i + 1], d = pts[2 * i + 1] - pts[2 * i];
        if (s < pts[2 * tl] + pts[2 * tl + 1]) tl = i;
        if (s > pts[2 * br] + pts[2 * br + 1]) br = i;
        if (d < pts[2 * tr + 1] - pts[2 * tr]) tr = i;
        if (d > pts[2 * bl + 1] - pts[2 * bl]) bl = i;
    }
    const int order[4] = {tl, tr, br, bl};
    float rect[4][2];
    for (int i = 0; i < 4; ++i) {
        rect[i][0] = (float)pts[2 * order[i]];
        rect[i][1] = (float)pts[2 * order[i] + 1];
        OCRVI_CHECK(std::isfinite(rect[i][0]) && std::isfinite(rect[i][1]), OCRVI_EINVAL, "four_point_transform: corner %d overflows float32", order[i]);
    }
    // side lengths entirely in float32 (numpy on the float32 rect), truncated by int()
    auto side = [&](int a, int b) -> float {
        const float dx = rect[a][0] - rect[b][0], dy = rect[a][1] - rect[b][1];
        const float xx = dx * dx, yy = dy * dy;
        return sqrtf(xx + yy);
    };
    const float top = side(1, 0), bottom = side(2, 3), left = side(0, 3), right = side(1, 2);
    OCRVI_CHECK(top < 2147483648.f && bottom < 2147483648.f && left < 2147483648.f && right < 2147483648.f, OCRVI_EINVAL,
                "four_point_transform: a side of the quad is longer than an int32");
    const int w = std::max((int)top, (int)bottom), h = std::max((int)left, (int)right);
    OCRVI_CHECK(w >= 1 && h >= 1, OCRVI_EINVAL, "four_point_transform: the quad rectifies to %d x %d pixels (a side shorter than one pixel)", w, h);
    const float dstf[4][2] = {{0.f, 0.f}, {(float)(w - 1), 0.f}, {(float)(w - 1), (float)(h - 1)}, {0.f, (float)(h - 1)}};
    double sp[4][2], dp[4][2];
    for (int i = 0; i < 4; ++i) { sp[i][0] = rect[i][0]; sp[i][1] = rect[i][1]; dp[i][0] = dstf[i][0]; dp[i][1] = dstf[i][1]; }
    // (the ordering can pick one point twice -- a diamond does --; the reference hands cv2 the degenerate system, the library refuses)
    OCRVI_CHECK(!three_collinear(sp), OCRVI_EINVAL, "four_point_transform: singular system: three of the ordered corners (%g,%g) (%g,%g) (%g,%g) (%g,%g) "
                "lie on one line or coincide", sp[0][0], sp[0][1], sp[1][0], sp[1][1], sp[2][0], sp[2][1], sp[3][0], sp[3][1]);
    OCRVI_CHECK(!three_collinear(dp), OCRVI_EINVAL, "four_point_transform: singular system: a %d x %d output has coinciding corners", w, h);
    // rows i / i + 4:  x h0 + y h1 + h2 - x u h6 - y u h7 = u,   x h3 + y h4 + h5 - x v h6 - y v h7 = v
    double A[8][9];
    for (int i = 0; i < 4; ++i) {
        const double x = sp[i][0], y = sp[i][1], u = dp[i][0], v = dp[i][1];
        const double r0[9] = {x, y, 1, 0, 0, 0, -x * u, -y * u, u}, r1[9] = {0, 0, 0, x, y, 1, -x * v, -y * v, v};
        for (int j = 0; j < 9; ++j) { A[i][j] = r0[j]; A[i + 4][j] = r1[j]; }
    }
    for (int c = 0; c < 8; ++c) {          // Gaussian elimination with partial pivoting
        int piv = c;
        for (int r = c + 1; r < 8; ++r) if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
        OCRVI_CHECK(A[piv][c] != 0.0 && std::isfinite(A[piv][c]), OCRVI_EINVAL, "four_point_transform: singular system (no pivot in column %d)", c);
        if (piv != c) for (int j = 0; j < 9; ++j) std::swap(A[c][j], A[piv][j]);
        for (int r = c + 1; r < 8; ++r) {
            const double f = A[r][c] / A[c][c];
            if (f == 0.0) continue;
            for (int j = c; j < 9; ++j) A[r][j] -= f * A[c][j];
        }
    }
    double hv[9];
    for (int r = 7; r >= 0; --r) {
        double acc = A[r][8];
        for (int j = r + 1; j < 8; ++j) acc -= A[r][j] * hv[j];
        hv[r] = acc / A[r][r];
        OCRVI_CHECK(std::isfinite(hv[r]), OCRVI_EINVAL, "four_point_transform: singular system (unknown %d is not finite)", r);
    }
    hv[8] = 1.0;
    // inverse: adjugate over determinant
    const double *m = hv;
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    OCRVI_CHECK(det != 0.0 && std::isfinite(det), OCRVI_EINVAL, "four_point_transform: the forward matrix has determinant %g", det);
    const double adj[9] = {c00, m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                           c01, m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                           c02, m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
    for (int i = 0; i < 9; ++i) {
        const double q = adj[i] / det;
        OCRVI_CHECK(std::isfinite(q), OCRVI_EINVAL, "four_point_transform: the inverse matrix is not finite (determinant %g)", det);
        m_inv[i] = q;
    }
    if (m_fwd) for (int i = 0; i < 9; ++i) m_fwd[i] = hv[i];
    *out_w = w;
    *out_h = h;
    return OCRVI_OK;
}

extern "C" int ocrvi_warp_perspective_u8(int device, const uint8_t* src, int src_h, int src_w, const double* m_inv_host, uint8_t* dst, int dst_h,
                                         int dst_w, void* stream) {
    OCRVI_CHECK(src && dst && m_inv_host && src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0, OCRVI_EINVAL, "warp_perspective_u8: bad argument");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    WarpMat M;               // passed by value: the host matrix is free again when the call returns
    for (int i = 0; i < 9; ++i) M.m[i] = m_inv_host[i];
    const size_t groups = ((size_t)dst_h * dst_w + 3) / 4;
    const int grid = (int)std::min<size_t>((groups + 255) / 256, 16384);
    hipLaunchKernelGGL(warp_perspective_u8_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, src_h, src_w, M, dst, dst_h, dst_w);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

extern "C" int ocrvi_warp_perspective_pages(int device, const int64_t* src_pages, const int64_t* dst_pages, const double* m_inv, int n, void* stream) {
    OCRVI_CHECK(src_pages && dst_pages && m_inv && n > 0 && n <= 65535, OCRVI_EINVAL, "warp_perspective_pages: bad argument (1 <= n <= 65535)");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    // the page sizes live in device memory: a fixed 1024 blocks per page stride over whatever size the table holds when the kernel runs
    hipLaunchKernelGGL(warp_perspective_pages_kernel, dim3(1024, n), dim3(256), 0, (hipStream_t)stream, src_pages, dst_pages, m_inv);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
