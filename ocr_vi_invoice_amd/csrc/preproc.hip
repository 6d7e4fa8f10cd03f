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

// DetectionDataset._resize_pad's image half (src/det/dataloader.py:240-261): page i resized to its own new_h x new_w (rows int32 [n][4] =
// (h, w, new_h, new_w), the row ocrvi_db_target_maps reads) with resize_u8_kernel's arithmetic -- a resize to the page's own size is the
// identity there, which is the reference's scale == 1.0 branch --, normalised in FLOAT32 ((v / 255 - mean) / std, every step rounded), then
// zero-padded to S x S.  One thread per output pixel: the pad and an invalid page are stores without a read.
__global__ void resize_normalize_pad_pages_kernel(const int64_t* __restrict__ table, const int32_t* __restrict__ rows, int n, int S,
                                                  float* __restrict__ out) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const size_t plane = (size_t)S * S, total = (size_t)n * plane;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int pg = (int)(i / plane);
        const size_t r = i - (size_t)pg * plane;
        const int y = (int)(r / S), x = (int)(r - (size_t)y * S);
        const PageRef src = load_page(table, pg);
        const int nh = min(rows[4 * pg + 2], S), nw = min(rows[4 * pg + 3], S);
        float f[3] = {0.f, 0.f, 0.f};
        if (src.h != 0 && x < nw && y < nh) {
            int v[3];
            resized_px(src.p, src.h, src.w, nh, nw, x, axis_coef(y, src.h, nh), y, src.w == 2 * nw && src.h == 2 * nh, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = ((float)v[c] / 255.0f - mean[c]) / stdv[c];
        }
        float* o = out + (size_t)pg * 3 * plane + r;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(size_t)c * plane] = f[c];
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

// ---------------------------------------------------------------- oriented text crops (include/ocrvi.h, "Oriented text crops")
// Pixel (x, y) of the intermediate crop C_b: warp_px under the crop's matrix with a replicate border -- a tap's row and column are clamped
// to the page instead of contributing 0, so a crop that overhangs the page edge gains no black rim.  Same coordinates, weights and rounding.
__device__ __forceinline__ void warp_px_replicate(const uint8_t* __restrict__ src, int sh, int sw, const double* __restrict__ m, int x, int y, int v[3]) {
#pragma clang fp contract(off)
    const double dx = (double)x, dy = (double)y;
    const double X0 = (m[0] * dx + m[1] * dy) + m[2];
    const double Y0 = (m[3] * dx + m[4] * dy) + m[5];
    const double W0 = (m[6] * dx + m[7] * dy) + m[8];
    const double s = (W0 != 0.0) ? 32.0 / W0 : 0.0;
    const int X = warp_coord(X0, s), Y = warp_coord(Y0, s);
    const int sx = X >> 5, sy = Y >> 5, ax = X & 31, ay = Y & 31;
    // clamped on the integers before any address is formed (sx is up to +-2^26: sx + 1 cannot overflow)
    const int x0 = min(max(sx, 0), sw - 1), x1 = min(max(sx + 1, 0), sw - 1);
    const int y0 = min(max(sy, 0), sh - 1), y1 = min(max(sy + 1, 0), sh - 1);
    const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
    const uint8_t *r0 = src + (size_t)y0 * sw * 3, *r1 = src + (size_t)y1 * sw * 3;
    const uint8_t *p00 = r0 + (size_t)x0 * 3, *p01 = r0 + (size_t)x1 * 3, *p10 = r1 + (size_t)x0 * 3, *p11 = r1 + (size_t)x1 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (16384 + w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c]) >> 15;
}

// where a crop's page comes from: a page table read when the kernel runs, or one [n,H,W,3] array
struct TablePages {
    const int64_t* table; int n;
    __device__ __forceinline__ PageRef get(int i) const { return (i >= 0 && i < n) ? load_page(table, i) : PageRef{nullptr, 0, 0}; }
};
struct ArrayPages {
    const uint8_t* images; int n, H, W;
    __device__ __forceinline__ PageRef get(int i) const {
        return (i >= 0 && i < n) ? PageRef{images + (size_t)i * H * W * 3, H, W} : PageRef{nullptr, 0, 0};
    }
};

// The direct form: one thread per output pixel forms the (at most) 2 x 2 pixels of C_b its resize reads, each from 2 x 2 page pixels; C_b
// is never stored.  A resize tap of weight 0 (identity rows or columns, the clamped last row / column) is not formed: it contributes 0
// whatever its value.  crops int32 [B,4] = (page, w, h, 0), m_inv float64 [B,9]; the rest is crop_resize_normalize_kernel on all of C_b.
template <class Pages>
__global__ void crop_quad_resize_normalize_kernel(Pages pages, const int32_t* __restrict__ crops, const double* __restrict__ m_inv, int B, int oh,
                                                  int ow, float* __restrict__ out) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const size_t total = (size_t)B * oh * ow;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % ow);
        const size_t t = i / ow;
        const int y = (int)(t % oh), b = (int)(t / oh);
        const int32_t* cr = crops + (size_t)b * 4;
        const int cw = cr[1], ch = cr[2];
        float* o = out + ((size_t)b * 3 * oh + y) * ow + x;
        const size_t plane = (size_t)oh * ow;
        const PageRef pr = pages.get(cr[0]);
        if (cw <= 0 || ch <= 0 || pr.h == 0) {  // empty crop, index out of range or invalid entry -> zeros tensor (pipeline2.py:154-156)
            o[0] = o[plane] = o[2 * plane] = 0.f;
            continue;
        }
        int new_w = (int)((double)cw * ((double)oh / (double)ch));
        if (new_w > ow) new_w = ow;   // squash (pipeline2.py:104-105)
        if (new_w < 1) new_w = 1;
        int v[3] = {255, 255, 255};
        if (x < new_w) {
            const double* m = m_inv + (size_t)b * 9;
            int p00[3], p01[3], p10[3], p11[3];
            if (cw == 2 * new_w && ch == 2 * oh) {  // exact 2x decimation: the 2x2 area filter
                warp_px_replicate(pr.p, pr.h, pr.w, m, 2 * x, 2 * y, p00);
                warp_px_replicate(pr.p, pr.h, pr.w, m, 2 * x + 1, 2 * y, p01);
                warp_px_replicate(pr.p, pr.h, pr.w, m, 2 * x, 2 * y + 1, p10);
                warp_px_replicate(pr.p, pr.h, pr.w, m, 2 * x + 1, 2 * y + 1, p11);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = (p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2;
            } else {
                const AxisCoef ax = axis_coef(x, cw, new_w), ay = axis_coef(y, ch, oh);
#pragma unroll
                for (int c = 0; c < 3; ++c) p01[c] = p10[c] = p11[c] = 0;
                warp_px_replicate(pr.p, pr.h, pr.w, m, ax.s0, ay.s0, p00);
                if (ax.a1 != 0) warp_px_replicate(pr.p, pr.h, pr.w, m, ax.s1, ay.s0, p01);
                if (ay.a1 != 0) {
                    warp_px_replicate(pr.p, pr.h, pr.w, m, ax.s0, ay.s1, p10);
                    if (ax.a1 != 0) warp_px_replicate(pr.p, pr.h, pr.w, m, ax.s1, ay.s1, p11);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int h0 = p00[c] * ax.a0 + p01[c] * ax.a1;
                    const int h1 = p10[c] * ax.a0 + p11[c] * ax.a1;
                    v[c] = (((ay.a0 * (h0 >> 4)) >> 16) + ((ay.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c * plane] = ((float)v[c] / 255.0f - mean[c]) / stdv[c];
    }
}

// The tile form: a workgroup owns an oh x QT_TW tile of one crop's output.  It warps every pixel of C_b the tile's resize reads once into
// LDS -- the double-precision division included --, then resizes from LDS and writes 16-byte stores per plane.  Enlarged crops (text lines
// under oh pixels high: the common case) share those pixels between neighbouring output pixels, which the direct form forms again per
// thread.  Per axis the LDS slots are either dense (slot = source index - first index, when the tile's source range fits the 2 oh rows /
// 2 QT_TW columns) or compact (slot = 2 * output index + tap, for a crop that is shrunk).  Pixels are packed r | g << 8 | b << 16; rows are
// QT_CS = 2 QT_TW + 1 words apart so that consecutive rows start on consecutive banks.
constexpr int QT_TW = 64;
constexpr int QT_CS = 2 * QT_TW + 1;
static inline size_t quad_tile_lds_bytes(int oh) { return ((size_t)2 * oh * QT_CS + 2 * oh + 2 * QT_TW) * 4; }

template <class Pages>
__global__ __launch_bounds__(256) void crop_quad_tile_kernel(Pages pages, const int32_t* __restrict__ crops, const double* __restrict__ m_inv, int oh,
                                                             int ow, float* __restrict__ out) {
    extern __shared__ uint32_t qt_lds[];
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    uint32_t* pix = qt_lds;                               // [2 oh][QT_CS]
    int* rowsrc = (int*)(qt_lds + (size_t)2 * oh * QT_CS);   // [2 oh]    row of C_b held by each row slot
    int* colsrc = rowsrc + 2 * oh;                        // [2 QT_TW] column of C_b held by each column slot
    const int tid = threadIdx.x, b = blockIdx.y, x0 = blockIdx.x * QT_TW;
    const int tw = min(QT_TW, ow - x0), tw4 = tw >> 2;    // ow % 4 == 0
    const int32_t* cr = crops + (size_t)b * 4;
    const int cw = cr[1], ch = cr[2];
    const size_t plane = (size_t)oh * ow;
    float* ob = out + (size_t)b * 3 * plane + x0;
    const PageRef pr = pages.get(cr[0]);
    const bool zero = cw <= 0 || ch <= 0 || pr.h == 0;    // empty crop, index out of range or invalid entry -> zeros tensor
    int new_w = 1;
    if (!zero) {
        new_w = (int)((double)cw * ((double)oh / (double)ch));
        if (new_w > ow) new_w = ow;   // squash (pipeline2.py:104-105)
        if (new_w < 1) new_w = 1;
    }
    const int nx = min(tw, new_w - x0);                   // the tile's columns left of the padding
    if (zero || nx <= 0) {                                // one value per plane: zeros, or the normalised 255 of the padding
        for (int q = tid; q < oh * tw4; q += 256) {
            const int y = q / tw4, xq = (q - y * tw4) * 4;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float f = zero ? 0.f : (255.0f / 255.0f - mean[c]) / stdv[c];
                *(float4*)(ob + (size_t)c * plane + (size_t)y * ow + xq) = make_float4(f, f, f, f);
            }
        }
        return;
    }
    const bool box = (cw == 2 * new_w && ch == 2 * oh);   // exact 2x decimation: the 2x2 area filter reads rows 2y, 2y+1, columns 2x, 2x+1
    bool rdense, cdense;
    int nrs, ncs, cmin;
    if (box) {
        rdense = cdense = true;
        nrs = ch; cmin = 2 * x0; ncs = 2 * nx;
    } else {
        rdense = ch <= 2 * oh;
        nrs = rdense ? ch : 2 * oh;
        const int c_lo = axis_coef(x0, cw, new_w).s0, c_hi = axis_coef(x0 + nx - 1, cw, new_w).s1;   // s0 and s1 never decrease with x
        cdense = c_hi - c_lo + 1 <= 2 * QT_TW;
        cmin = cdense ? c_lo : 0;
        ncs = cdense ? c_hi - c_lo + 1 : 2 * nx;
    }
    for (int i = tid; i < nrs; i += 256) {
        int r = i;
        if (!rdense) { const AxisCoef a = axis_coef(i >> 1, ch, oh); r = (i & 1) ? a.s1 : a.s0; }
        rowsrc[i] = r;
    }
    for (int j = tid; j < ncs; j += 256) {
        int c = cmin + j;
        if (!cdense) { const AxisCoef a = axis_coef(x0 + (j >> 1), cw, new_w); c = (j & 1) ? a.s1 : a.s0; }
        colsrc[j] = c;
    }
    __syncthreads();
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = m_inv[(size_t)b * 9 + k];
    for (int s = tid; s < nrs * ncs; s += 256) {
        const int i = s / ncs, j = s - i * ncs;
        int v[3];
        warp_px_replicate(pr.p, pr.h, pr.w, m, colsrc[j], rowsrc[i], v);
        pix[i * QT_CS + j] = (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16);
    }
    __syncthreads();
    for (int q = tid; q < oh * tw4; q += 256) {
        const int y = q / tw4, xq = (q - y * tw4) * 4;
        const AxisCoef ay = axis_coef(y, ch, oh);
        const int i0 = box ? 2 * y : (rdense ? ay.s0 : 2 * y), i1 = box ? 2 * y + 1 : (rdense ? ay.s1 : 2 * y + 1);
        const uint32_t *r0 = pix + i0 * QT_CS, *r1 = pix + i1 * QT_CS;
        float f[3][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xl = xq + k, x = x0 + xl;
            int v[3] = {255, 255, 255};
            if (x < new_w) {
                if (box) {
                    const uint32_t a = r0[2 * xl], bb = r0[2 * xl + 1], c2 = r1[2 * xl], d = r1[2 * xl + 1];
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        v[c] = (int)(((a >> (8 * c)) & 255) + ((bb >> (8 * c)) & 255) + ((c2 >> (8 * c)) & 255) + ((d >> (8 * c)) & 255) + 2) >> 2;
                } else {
                    const AxisCoef ax = axis_coef(x, cw, new_w);
                    const int j0 = cdense ? ax.s0 - cmin : 2 * xl, j1 = cdense ? ax.s1 - cmin : 2 * xl + 1;
                    const uint32_t p00 = r0[j0], p01 = r0[j1], p10 = r1[j0], p11 = r1[j1];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int h0 = (int)((p00 >> (8 * c)) & 255) * ax.a0 + (int)((p01 >> (8 * c)) & 255) * ax.a1;
                        const int h1 = (int)((p10 >> (8 * c)) & 255) * ax.a0 + (int)((p11 >> (8 * c)) & 255) * ax.a1;
                        v[c] = (((ay.a0 * (h0 >> 4)) >> 16) + ((ay.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c][k] = ((float)v[c] / 255.0f - mean[c]) / stdv[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) *(float4*)(ob + (size_t)c * plane + (size_t)y * ow + xq) = make_float4(f[c][0], f[c][1], f[c][2], f[c][3]);
    }
}

// the tile form needs 16-byte stores (out_w % 4 == 0, out 16-byte aligned), one grid row per crop and its LDS; anything else takes the direct form
template <class Pages>
static int launch_crop_quad(Pages pages, const int32_t* crops, const double* m_inv, int B, int oh, int ow, float* out, hipStream_t stream) {
    const size_t lds = quad_tile_lds_bytes(oh);
    if (ow % 4 == 0 && (((uintptr_t)out) & 15) == 0 && B <= 65535 && lds <= 65536) {
        hipLaunchKernelGGL(crop_quad_tile_kernel<Pages>, dim3((ow + QT_TW - 1) / QT_TW, B), dim3(256), lds, stream, pages, crops, m_inv, oh, ow, out);
    } else {
        const size_t total = (size_t)B * oh * ow;
        const int grid = (int)std::min<size_t>((total + 255) / 256, 16384);
        hipLaunchKernelGGL(crop_quad_resize_normalize_kernel<Pages>, dim3(grid), dim3(256), 0, stream, pages, crops, m_inv, B, oh, ow, out);
    }
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
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

extern "C" int ocrvi_resize_normalize_pad_pages(int device, const int64_t* pages, const int32_t* rows, int n, int S, float* out, void* stream) {
    OCRVI_CHECK(pages && rows && out && n > 0 && S > 0, OCRVI_EINVAL, "resize_normalize_pad_pages: bad argument");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    const size_t total = (size_t)n * S * S;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 16384);
    ProfScope ps("resize_normalize_pad", 0.0, 12.0 * total, (hipStream_t)stream);
    hipLaunchKernelGGL(resize_normalize_pad_pages_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, pages, rows, n, S, out);
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

// ---------------------------------------------------------------- oriented text crops: the two device entries (the host half is quads.hip)
extern "C" int ocrvi_crop_quad_resize_normalize_pages(int device, const int64_t* pages, int n_pages, const int32_t* crops, const double* m_inv, int B,
                                                      int out_h, int out_w, float* out, void* stream) {
    OCRVI_CHECK(pages && crops && m_inv && out && n_pages > 0 && B > 0 && out_h > 0 && out_w > 0, OCRVI_EINVAL,
                "crop_quad_resize_normalize_pages: bad argument");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    return launch_crop_quad(TablePages{pages, n_pages}, crops, m_inv, B, out_h, out_w, out, (hipStream_t)stream);
}

extern "C" int ocrvi_crop_quad_resize_normalize(int device, const uint8_t* images, int n_img, int H, int W, const int32_t* crops, const double* m_inv,
                                                int B, int out_h, int out_w, float* out, void* stream) {
    OCRVI_CHECK(images && crops && m_inv && out && n_img > 0 && H > 0 && W > 0 && B > 0 && out_h > 0 && out_w > 0, OCRVI_EINVAL,
                "crop_quad_resize_normalize: bad argument");
    DeviceGuard dg(device);  // the caller's current device is restored on return
    OCRVI_HIP(dg.err);
    return launch_crop_quad(ArrayPages{images, n_img, H, W}, crops, m_inv, B, out_h, out_w, out, (hipStream_t)stream);
}
