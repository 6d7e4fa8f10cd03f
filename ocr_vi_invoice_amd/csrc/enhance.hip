// enhance_document on the device (src/preprocess/scanner.py:55-76): COLOR_BGR2LAB -> CLAHE(2.0, 8x8) on L -> COLOR_LAB2BGR ->
// fastNlMeansDenoisingColored(10, 10, 7, 21) -> filter2D with the 3x3 sharpen kernel.  Everything is integer arithmetic on tables that
// the host builds once in double (include/ocrvi.h states every formula): the kernels below and tests/enhance_ref.py are two statements of
// the same definition and agree bit for bit.  The definition is modelled on OpenCV's 8-bit paths; cv2 is absent from the build container
// and its Lab, CLAHE and NLM code differ between versions: parity with cv2 itself is UNPINNED, as for the resize and the warp.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>

#include "common.h"

namespace ocrvi {

// ---------------------------------------------------------------- tables (int32 each, in this order: what ocrvi_enhance_tables returns)
constexpr int T_LIN = 0;               // [256]  rint(2040 g(v / 255))
constexpr int T_F = T_LIN + 256;       // [2041] rint(32768 f(t / 2040))
constexpr int T_ENC = T_F + 2041;      // [2041] rint(255 g^-1(t / 2040))
constexpr int T_FY = T_ENC + 2041;     // [256]  rint((L 100 / 255 + 16) / 116 * 32768)
constexpr int T_DA = T_FY + 256;       // [256]  rint((a - 128) 32768 / 500)
constexpr int T_DB = T_DA + 256;       // [256]  rint((b - 128) 32768 / 200)
constexpr int T_W1 = T_DB + 256;       // [1024] rint(255 exp(-(k 64 / 49) / 100))
constexpr int T_W2 = T_W1 + 1024;      // [1024] rint(255 exp(-(k 64 / 49) / 200))
constexpr int T_CF = T_W2 + 1024;      // [9]    RGB (linear) -> XYZ / white, 12 fractional bits, rows sum to 4096
constexpr int T_CI = T_CF + 9;         // [9]    XYZ / white -> RGB (linear), likewise
constexpr int T_TOTAL = T_CI + 9;      // 7172

static void fix_row(int32_t* r) {      // the entry of largest magnitude takes the rounding residue: the row sums to exactly 4096
    int j = 0;
    for (int k = 1; k < 3; ++k) if (std::abs(r[k]) > std::abs(r[j])) j = k;
    r[j] += 4096 - (r[0] + r[1] + r[2]);
}

static const int32_t* host_tables() {
    static int32_t t[T_TOTAL];
    static std::once_flag once;
    std::call_once(once, [] {
#pragma clang fp contract(off)
        for (int v = 0; v < 256; ++v) {
            const double c = (double)v / 255.0;
            const double g = c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4);
            t[T_LIN + v] = (int32_t)rint(2040.0 * g);
            t[T_FY + v] = (int32_t)rint(((double)v * 100.0 / 255.0 + 16.0) / 116.0 * 32768.0);
            t[T_DA + v] = (int32_t)rint((double)(v - 128) * 32768.0 / 500.0);
            t[T_DB + v] = (int32_t)rint((double)(v - 128) * 32768.0 / 200.0);
        }
        for (int i = 0; i <= 2040; ++i) {
            const double x = (double)i / 2040.0;
            const double f = x > 216.0 / 24389.0 ? cbrt(x) : (841.0 / 108.0) * x + 4.0 / 29.0;
            t[T_F + i] = (int32_t)rint(32768.0 * f);
            const double e = x <= 0.0031308 ? 12.92 * x : 1.055 * pow(x, 1.0 / 2.4) - 0.055;
            t[T_ENC + i] = (int32_t)rint(255.0 * e);
        }
        for (int k = 0; k < 1024; ++k) {
            const double d = (double)k * 64.0 / 49.0;
            t[T_W1 + k] = (int32_t)rint(255.0 * exp(-d / 100.0));
            t[T_W2 + k] = (int32_t)rint(255.0 * exp(-d / 200.0));
        }
        const double M[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
        double white[3], inv[3][3];
        for (int i = 0; i < 3; ++i) white[i] = M[i][0] + M[i][1] + M[i][2];
        const double c00 = M[1][1] * M[2][2] - M[1][2] * M[2][1], c01 = M[1][2] * M[2][0] - M[1][0] * M[2][2], c02 = M[1][0] * M[2][1] - M[1][1] * M[2][0];
        const double det = M[0][0] * c00 + M[0][1] * c01 + M[0][2] * c02;
        const double adj[3][3] = {{c00, M[0][2] * M[2][1] - M[0][1] * M[2][2], M[0][1] * M[1][2] - M[0][2] * M[1][1]},
                                  {c01, M[0][0] * M[2][2] - M[0][2] * M[2][0], M[0][2] * M[1][0] - M[0][0] * M[1][2]},
                                  {c02, M[0][1] * M[2][0] - M[0][0] * M[2][1], M[0][0] * M[1][1] - M[0][1] * M[1][0]}};
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) {
                inv[i][j] = adj[i][j] / det;
                t[T_CF + 3 * i + j] = (int32_t)rint(4096.0 * M[i][j] / white[i]);
                t[T_CI + 3 * i + j] = (int32_t)rint(4096.0 * inv[i][j] * white[j]);
            }
            fix_row(t + T_CF + 3 * i);
            fix_row(t + T_CI + 3 * i);
        }
    });
    return t;
}

constexpr int MAX_DEVICES = 64;
static int32_t* g_tables[MAX_DEVICES];
static std::mutex g_tables_mu;

// ---------------------------------------------------------------- colour
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// T: the table block (LDS or global).  v: R, G, B -> L, a, b
__device__ __forceinline__ void rgb_to_lab_px(const int32_t* T, int v[3]) {
    const int l0 = T[T_LIN + v[0]], l1 = T[T_LIN + v[1]], l2 = T[T_LIN + v[2]];
    int f[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int xyz = (T[T_CF + 3 * i] * l0 + T[T_CF + 3 * i + 1] * l1 + T[T_CF + 3 * i + 2] * l2 + 2048) >> 12;   // <= 2040: the row sums to 4096
        f[i] = T[T_F + xyz];
    }
    const int n = 2958 * f[1] - 13369344 + 163840;
    const int L = n >= 0 ? n / 327680 : -((327679 - n) / 327680);      // floor division
    v[0] = clampi(L, 0, 255);
    v[1] = clampi(((500 * (f[0] - f[1]) + 16384) >> 15) + 128, 0, 255);
    v[2] = clampi(((200 * (f[1] - f[2]) + 16384) >> 15) + 128, 0, 255);
}

__device__ __forceinline__ int lab_t(int f) {
    if (f > 6781) return (int)(((long long)f * f * f * 2040 + (1LL << 44)) >> 45);
    const int t = ((f - 4520) * 8383 + (1 << 19)) >> 20;
    return t > 0 ? t : 0;
}

// v: L, a, b -> R, G, B
__device__ __forceinline__ void lab_to_rgb_px(const int32_t* T, int v[3]) {
    const int fy = T[T_FY + v[0]];
    const int t0 = lab_t(clampi(fy + T[T_DA + v[1]], 0, 49151)), t1 = lab_t(clampi(fy, 0, 49151)), t2 = lab_t(clampi(fy - T[T_DB + v[2]], 0, 49151));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int r = (T[T_CI + 3 * i] * t0 + T[T_CI + 3 * i + 1] * t1 + T[T_CI + 3 * i + 2] * t2 + 2048) >> 12;
        v[i] = T[T_ENC + clampi(r, 0, 2040)];
    }
}

// ---------------------------------------------------------------- CLAHE
// One workgroup per tile of the 8 x 8 grid over the plane padded (reflect-101, right and down) to multiples of 8: histogram of channel 0
// with LDS atomics, clip at max(2 th tw / 256, 1), the excess spread evenly plus a residue on every step-th bin, inclusive scan, LUT.
__global__ void __launch_bounds__(256) clahe_lut_kernel(const uint8_t* __restrict__ lab, int h, int w, int th, int tw, uint8_t* __restrict__ lut) {
    __shared__ int hist[256];
    __shared__ int scan[2][256];
    __shared__ int s_excess;
    const int tid = threadIdx.x, ty = blockIdx.x >> 3, tx = blockIdx.x & 7;
    hist[tid] = 0;
    if (tid == 0) s_excess = 0;
    __syncthreads();
    const int area = th * tw;
    for (int i = tid; i < area; i += 256) {
        const int py = ty * th + i / tw, px = tx * tw + i % tw;
        const int sy = py < h ? py : 2 * (h - 1) - py, sx = px < w ? px : 2 * (w - 1) - px;     // at most 7 past the edge, h, w >= 16
        atomicAdd(&hist[lab[((size_t)sy * w + sx) * 3]], 1);
    }
    __syncthreads();
    const int clip = max((int)(2LL * area / 256), 1);
    int c = hist[tid];
    if (c > clip) { atomicAdd(&s_excess, c - clip); c = clip; }
    __syncthreads();
    const int excess = s_excess, r = excess & 255;
    c += excess >> 8;
    if (r > 0) {
        const int step = max(256 / r, 1);
        if (tid % step == 0 && tid / step < r) ++c;
    }
    int cur = 0;
    scan[0][tid] = c;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < 256; d <<= 1) {
        scan[cur ^ 1][tid] = scan[cur][tid] + (tid >= d ? scan[cur][tid - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    lut[(size_t)blockIdx.x * 256 + tid] = (uint8_t)((255LL * scan[cur][tid] + area / 2) / area);
}

struct ClaheGeom { int th, tw; };

// bilinear interpolation between the four surrounding tile LUTs (tile centres; the outer half tiles take the nearest)
__device__ __forceinline__ int clahe_px(const uint8_t* __restrict__ lut, int v, int x, int y, ClaheGeom g) {
    const int nx = 2 * x + 1 - g.tw, ny = 2 * y + 1 - g.th;                 // nx > -2 tw: the floor quotient is -1 or nx / 2tw
    int tx1 = nx < 0 ? -1 : nx / (2 * g.tw), ty1 = ny < 0 ? -1 : ny / (2 * g.th);
    const long long ax = nx - tx1 * 2 * g.tw, ay = ny - ty1 * 2 * g.th;
    int tx2 = min(tx1 + 1, 7), ty2 = min(ty1 + 1, 7);
    tx1 = clampi(tx1, 0, 7); ty1 = clampi(ty1, 0, 7);
    const long long bx = 2 * g.tw - ax, by = 2 * g.th - ay;
    const long long s = bx * by * lut[(ty1 * 8 + tx1) * 256 + v] + ax * by * lut[(ty1 * 8 + tx2) * 256 + v] +
                        bx * ay * lut[(ty2 * 8 + tx1) * 256 + v] + ax * ay * lut[(ty2 * 8 + tx2) * 256 + v];
    const long long q = 2LL * g.tw * g.th;
    return (int)((s + q) / (2 * q));
}

// ---------------------------------------------------------------- the per-pixel stages
// Groups of 4 consecutive pixels of the page taken as one flat run (12 bytes at 12 g, as the warp writes them): three 4-byte words when
// the base address is a multiple of 4, bytes otherwise and for the last, partial group.
enum { PX_RGB2LAB = 0, PX_LAB2RGB = 1, PX_CLAHE = 2, PX_CLAHE_RGB_LAB = 3 };

__device__ __forceinline__ void load_group(const uint8_t* __restrict__ p, bool words, int cnt, uint32_t w[3]) {
    if (words && cnt == 4) {
        w[0] = ((const uint32_t*)p)[0]; w[1] = ((const uint32_t*)p)[1]; w[2] = ((const uint32_t*)p)[2];
    } else {
        w[0] = w[1] = w[2] = 0u;
        for (int j = 0; j < cnt * 3; ++j) w[j >> 2] |= (uint32_t)p[j] << (8 * (j & 3));
    }
}
__device__ __forceinline__ void store_group(uint8_t* __restrict__ o, bool words, int cnt, const uint32_t w[3]) {
    if (words && cnt == 4) {
        ((uint32_t*)o)[0] = w[0]; ((uint32_t*)o)[1] = w[1]; ((uint32_t*)o)[2] = w[2];
    } else {
        for (int j = 0; j < cnt * 3; ++j) o[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
}

template <int MODE>
__global__ void __launch_bounds__(256) px_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w,
                                                 const int32_t* __restrict__ tables, const uint8_t* __restrict__ lut, ClaheGeom geom) {
    __shared__ int32_t T[MODE == PX_CLAHE ? 1 : T_TOTAL];
    if (MODE != PX_CLAHE) {
        for (int i = threadIdx.x; i < T_TOTAL; i += 256) T[i] = tables[i];
        __syncthreads();
    }
    const size_t npx = (size_t)h * w, groups = (npx + 3) >> 2;
    const bool rwords = (((uintptr_t)src) & 3) == 0, wwords = (((uintptr_t)dst) & 3) == 0;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        const size_t i0 = g * 4;
        const int cnt = (int)min((size_t)4, npx - i0);
        int y = (int)(i0 / (size_t)w), x = (int)(i0 - (size_t)y * w);
        uint32_t in[3], out[3] = {0u, 0u, 0u};
        load_group(src + i0 * 3, rwords, cnt, in);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = (in[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3))) & 255;
            if (k < cnt) {
                if (MODE == PX_RGB2LAB) rgb_to_lab_px(T, v);
                if (MODE == PX_LAB2RGB) lab_to_rgb_px(T, v);
                if (MODE == PX_CLAHE || MODE == PX_CLAHE_RGB_LAB) v[0] = clahe_px(lut, v[0], x, y, geom);
                if (MODE == PX_CLAHE_RGB_LAB) { lab_to_rgb_px(T, v); rgb_to_lab_px(T, v); }     // the uint8 RGB page between them stays in registers
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) out[(3 * k + c) >> 2] |= (uint32_t)v[c] << (8 * ((3 * k + c) & 3));
            if (++x == w) { x = 0; ++y; }
        }
        store_group(dst + i0 * 3, wwords, cnt, out);
    }
}

// ---------------------------------------------------------------- sharpen: clamp(9 c - the eight neighbours), reflect-101
__global__ void __launch_bounds__(256) sharpen_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w) {
    const size_t npx = (size_t)h * w, groups = (npx + 3) >> 2;
    const bool wwords = (((uintptr_t)dst) & 3) == 0;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        const size_t i0 = g * 4;
        const int cnt = (int)min((size_t)4, npx - i0);
        int y = (int)(i0 / (size_t)w), x = (int)(i0 - (size_t)y * w);
        uint32_t out[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < cnt) {
                const int ys[3] = {y == 0 ? 1 : y - 1, y, y == h - 1 ? h - 2 : y + 1};
                const int xs[3] = {x == 0 ? 1 : x - 1, x, x == w - 1 ? w - 2 : x + 1};
                int s[3] = {0, 0, 0};
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const uint8_t* p = src + ((size_t)ys[j] * w + xs[i]) * 3;
                        s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
                    }
                const uint8_t* cp = src + ((size_t)y * w + x) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) out[(3 * k + c) >> 2] |= (uint32_t)clampi(10 * cp[c] - s[c], 0, 255) << (8 * ((3 * k + c) & 3));
            }
            if (++x == w) { x = 0; ++y; }
        }
        store_group(dst + i0 * 3, wwords, cnt, out);
    }
}

// ---------------------------------------------------------------- non-local means (template 7, search 21) on C planes of the Lab page
// One workgroup per 32 x 64 tile of the output: the tile and its 13-pixel halo (reflect-101) of the C planes lie in LDS as bytes (rows
// of 60), beside them S2, the horizontal 7-sum of squares over the C planes at every window start, and the 1024-entry weight table.
// A thread owns column `tx` of an 8-row strip.  A row's horizontal 7-sum of squared differences between the template at p and the one at
// p + q is  sum a^2 + sum b^2 - 2 sum a b  =  S2(p) + S2(p + q) - 2 dot(a, b): the thread keeps its 14 template rows packed in registers
// for all 441 offsets (seven bytes in two words per row and plane), fetches the other template's seven bytes as three aligned words,
// shifts them into place (v_alignbyte) and forms the products with two v_dot4_u32_u8.  It walks down the strip's 14 rows with the last
// seven row sums as a running vertical sum and from the seventh row on has the 7 x 7 distance of one output pixel: no barrier in the
// offset loop, all sums exact in uint32 / int32 (a distance is at most 98 * 255^2, an accumulator at most 441 * 255 * 255).
constexpr int NLM_TW = 32, NLM_TH = 64, NLM_STRIP = 8, NLM_HALO = 13, NLM_LW = NLM_TW + 2 * NLM_HALO, NLM_LH = NLM_TH + 2 * NLM_HALO;
constexpr int NLM_PITCH = (NLM_LW + 3) & ~3;          // bytes per LDS row: a multiple of 4, so a lane's byte shift is the same on every row
constexpr int NLM_SW = NLM_LW - 6;                    // window starts per row

__device__ __forceinline__ int reflect_clamp(int v, int n) {      // reflect-101, then (a partial tile's unused columns) into range
    if (v < 0) v = -v;
    if (v >= n) v = 2 * (n - 1) - v;
    return clampi(v, 0, n - 1);
}

template <int C, int C0>
__global__ void __launch_bounds__(256) nlm_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w,
                                                  const int32_t* __restrict__ wtab) {
    __shared__ __attribute__((aligned(16))) uint8_t sI[C][NLM_LH * NLM_PITCH + 16];     // (+16: slack; a three-word fetch ends inside its row)
    __shared__ uint32_t sS2[NLM_LH * NLM_SW];
    __shared__ uint8_t sW[1024];
    const int tid = threadIdx.x, x0 = blockIdx.x * NLM_TW, y0 = blockIdx.y * NLM_TH;
    for (int i = tid; i < NLM_LH * NLM_PITCH + 16; i += 256) {
        const int ly = i / NLM_PITCH, lx = i - ly * NLM_PITCH;
        const bool in = ly < NLM_LH && lx < NLM_LW;               // the padding bytes are fetched but never enter a product
        const int gy = reflect_clamp(y0 - NLM_HALO + ly, h), gx = reflect_clamp(x0 - NLM_HALO + lx, w);
        const uint8_t* p = src + ((size_t)gy * w + gx) * 3 + C0;
#pragma unroll
        for (int c = 0; c < C; ++c) sI[c][i] = in ? p[c] : (uint8_t)0;
    }
    for (int i = tid; i < 1024; i += 256) sW[i] = (uint8_t)wtab[i];
    __syncthreads();
    for (int i = tid; i < NLM_LH * NLM_SW; i += 256) {
        const int ly = i / NLM_SW, lx = i - ly * NLM_SW;
        uint32_t s = 0;
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) {
                const uint32_t v = sI[c][ly * NLM_PITCH + lx + dx];
                s += v * v;
            }
        sS2[i] = s;
    }
    __syncthreads();
    const int tx = tid & (NLM_TW - 1), ry0 = (tid / NLM_TW) * NLM_STRIP;
    const int arow = ry0 + NLM_HALO - 3, acol = tx + NLM_HALO - 3;              // template row 0, column 0 of output row ry0
    uint32_t alo[NLM_STRIP + 6][C], ahi[NLM_STRIP + 6][C], a2[NLM_STRIP + 6];
#pragma unroll
    for (int j = 0; j < NLM_STRIP + 6; ++j) {
        a2[j] = sS2[(arow + j) * NLM_SW + acol];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint8_t* a = &sI[c][(arow + j) * NLM_PITCH + acol];
            alo[j][c] = (uint32_t)a[0] | ((uint32_t)a[1] << 8) | ((uint32_t)a[2] << 16) | ((uint32_t)a[3] << 24);
            ahi[j][c] = (uint32_t)a[4] | ((uint32_t)a[5] << 8) | ((uint32_t)a[6] << 16);      // the fourth byte is 0: seven products
        }
    }
    int sw[NLM_STRIP], acc[NLM_STRIP][C];
#pragma unroll
    for (int o = 0; o < NLM_STRIP; ++o) {
        sw[o] = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[o][c] = 0;
    }
    for (int q = 0; q < 441; ++q) {
        const int qy = q / 21 - 10, qx = q - (q / 21) * 21 - 10;
        const int bcol = acol + qx, brow = arow + qy;                            // 0 <= bcol <= NLM_SW - 1, 0 <= brow
        const uint32_t sh = (uint32_t)bcol & 3u;
        const int bword = brow * NLM_PITCH + (bcol & ~3);
        const int bs2 = brow * NLM_SW + bcol;
        uint32_t hs[7], vsum = 0;
#pragma unroll
        for (int j = 0; j < NLM_STRIP + 6; ++j) {
            uint32_t dot = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const uint32_t* bw = (const uint32_t*)&sI[c][bword + j * NLM_PITCH];
                const uint32_t w0 = bw[0], w1 = bw[1], w2 = bw[2];
                dot = __builtin_amdgcn_udot4(alo[j][c], __builtin_amdgcn_alignbyte(w1, w0, sh), dot, false);
                dot = __builtin_amdgcn_udot4(ahi[j][c], __builtin_amdgcn_alignbyte(w2, w1, sh), dot, false);
            }
            const uint32_t hsum = a2[j] + sS2[bs2 + j * NLM_SW] - 2u * dot;
            if (j >= 7) vsum -= hs[j % 7];
            hs[j % 7] = hsum;
            vsum += hsum;
            if (j >= 6) {
                const int o = j - 6;
                const int wt = sW[min(vsum >> 6, 1023u)];
                sw[o] += wt;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[o][c] += wt * (int)sI[c][(brow + o + 3) * NLM_PITCH + bcol + 3];
            }
        }
    }
    const int gx = x0 + tx;
    if (gx >= w) return;
#pragma unroll
    for (int o = 0; o < NLM_STRIP; ++o) {
        const int gy = y0 + ry0 + o;
        if (gy >= h) break;
        uint8_t* p = dst + ((size_t)gy * w + gx) * 3 + C0;
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = (uint8_t)((acc[o][c] + (sw[o] >> 1)) / sw[o]);     // sw >= 255: the offset (0, 0) has distance 0
    }
}

// ---------------------------------------------------------------- host side
constexpr size_t LUT_BYTES = 64 * 256;
constexpr int MIN_SIDE = 16;
constexpr size_t MAX_PIXELS = (size_t)1 << 29;

static int check_page(const char* what, int device, const void* src, int h, int w, const void* dst, const int32_t** tables) {
    OCRVI_CHECK(src && dst, OCRVI_EINVAL, "%s: null pointer", what);
    OCRVI_CHECK(h >= MIN_SIDE && w >= MIN_SIDE, OCRVI_EINVAL, "%s: a %d x %d page is smaller than %d x %d", what, h, w, MIN_SIDE, MIN_SIDE);
    OCRVI_CHECK((size_t)h * (size_t)w <= MAX_PIXELS, OCRVI_EINVAL, "%s: a %d x %d page has more than 2^29 pixels", what, h, w);
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst, n = (uintptr_t)h * w * 3;
    OCRVI_CHECK(s + n <= d || d + n <= s, OCRVI_EINVAL, "%s: dst overlaps src", what);
    OCRVI_CHECK(device >= 0 && device < MAX_DEVICES, OCRVI_EINVAL, "%s: device %d", what, device);
    const int32_t* t;
    {
        std::lock_guard<std::mutex> lk(g_tables_mu);
        t = g_tables[device];
    }
    OCRVI_CHECK(t, OCRVI_EINVAL, "%s: ocrvi_enhance_init(%d) has not been called", what, device);
    *tables = t;
    return OCRVI_OK;
}

static inline int px_grid(int h, int w) { return (int)std::min<size_t>((((size_t)h * w + 3) / 4 + 255) / 256, 1024); }
static inline ClaheGeom clahe_geom(int h, int w) { return ClaheGeom{(h + 7) / 8, (w + 7) / 8}; }
static inline size_t page_bytes(int h, int w) { return ((size_t)h * w * 3 + 255) & ~(size_t)255; }

template <int MODE>
static int launch_px(const uint8_t* src, uint8_t* dst, int h, int w, const int32_t* t, const uint8_t* lut, hipStream_t st) {
    hipLaunchKernelGGL(px_kernel<MODE>, dim3(px_grid(h, w)), dim3(256), 0, st, src, dst, h, w, t, lut, clahe_geom(h, w));
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
static int launch_lut(const uint8_t* lab, int h, int w, uint8_t* lut, hipStream_t st) {
    const ClaheGeom g = clahe_geom(h, w);
    hipLaunchKernelGGL(clahe_lut_kernel, dim3(64), dim3(256), 0, st, lab, h, w, g.th, g.tw, lut);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
static int launch_nlm(const uint8_t* src, uint8_t* dst, int h, int w, const int32_t* t, hipStream_t st) {
    const dim3 grid((w + NLM_TW - 1) / NLM_TW, (h + NLM_TH - 1) / NLM_TH);
    hipLaunchKernelGGL((nlm_kernel<1, 0>), grid, dim3(256), 0, st, src, dst, h, w, t + T_W1);
    OCRVI_HIP(hipGetLastError());
    hipLaunchKernelGGL((nlm_kernel<2, 1>), grid, dim3(256), 0, st, src, dst, h, w, t + T_W2);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}
static int launch_sharpen(const uint8_t* src, uint8_t* dst, int h, int w, hipStream_t st) {
    hipLaunchKernelGGL(sharpen_kernel, dim3(px_grid(h, w)), dim3(256), 0, st, src, dst, h, w);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

}  // namespace ocrvi

using namespace ocrvi;

extern "C" int ocrvi_enhance_tables(void* out, size_t cap, size_t* bytes) {
    OCRVI_CHECK(bytes, OCRVI_EINVAL, "enhance_tables: null pointer");
    *bytes = sizeof(int32_t) * T_TOTAL;
    if (!out) return OCRVI_OK;
    OCRVI_CHECK(cap >= *bytes, OCRVI_ENOMEM, "enhance_tables: %zu bytes given, %zu needed", cap, *bytes);
    memcpy(out, host_tables(), *bytes);
    return OCRVI_OK;
}

extern "C" int ocrvi_enhance_init(int device) {
    OCRVI_CHECK(device >= 0 && device < MAX_DEVICES, OCRVI_EINVAL, "enhance_init: device %d", device);
    std::lock_guard<std::mutex> lk(g_tables_mu);
    if (g_tables[device]) return OCRVI_OK;
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    int32_t* d = nullptr;
    OCRVI_HIP(hipMalloc((void**)&d, sizeof(int32_t) * T_TOTAL));
    const hipError_t e = hipMemcpy(d, host_tables(), sizeof(int32_t) * T_TOTAL, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        OCRVI_HIP(e);
    }
    g_tables[device] = d;
    return OCRVI_OK;
}

extern "C" int ocrvi_enhance_workspace_bytes(int h, int w, size_t* bytes) {
    OCRVI_CHECK(bytes, OCRVI_EINVAL, "enhance_workspace_bytes: null pointer");
    OCRVI_CHECK(h >= MIN_SIDE && w >= MIN_SIDE && (size_t)h * (size_t)w <= MAX_PIXELS, OCRVI_EINVAL,
                "enhance_workspace_bytes: %d x %d (16 <= h, w and h w <= 2^29)", h, w);
    *bytes = LUT_BYTES + 2 * page_bytes(h, w);
    return OCRVI_OK;
}

extern "C" int ocrvi_rgb_to_lab_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* stream) {
    const int32_t* t;
    OCRVI_TRY(check_page("rgb_to_lab_u8", device, src, h, w, dst, &t));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_px<PX_RGB2LAB>(src, dst, h, w, t, nullptr, (hipStream_t)stream);
}

extern "C" int ocrvi_lab_to_rgb_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* stream) {
    const int32_t* t;
    OCRVI_TRY(check_page("lab_to_rgb_u8", device, src, h, w, dst, &t));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_px<PX_LAB2RGB>(src, dst, h, w, t, nullptr, (hipStream_t)stream);
}

extern "C" int ocrvi_clahe_lab_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* workspace, size_t workspace_bytes, void* stream) {
    const int32_t* t;
    OCRVI_TRY(check_page("clahe_lab_u8", device, src, h, w, dst, &t));
    OCRVI_CHECK(workspace, OCRVI_EINVAL, "clahe_lab_u8: null workspace");
    OCRVI_CHECK(workspace_bytes >= LUT_BYTES, OCRVI_ENOMEM, "clahe_lab_u8: workspace of %zu bytes, %zu needed", workspace_bytes, LUT_BYTES);
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    OCRVI_TRY(launch_lut(src, h, w, (uint8_t*)workspace, (hipStream_t)stream));
    return launch_px<PX_CLAHE>(src, dst, h, w, t, (const uint8_t*)workspace, (hipStream_t)stream);
}

extern "C" int ocrvi_nlm_lab_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* stream) {
    const int32_t* t;
    OCRVI_TRY(check_page("nlm_lab_u8", device, src, h, w, dst, &t));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_nlm(src, dst, h, w, t, (hipStream_t)stream);
}

extern "C" int ocrvi_sharpen_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* stream) {
    const int32_t* t;
    OCRVI_TRY(check_page("sharpen_u8", device, src, h, w, dst, &t));
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    return launch_sharpen(src, dst, h, w, (hipStream_t)stream);
}

extern "C" int ocrvi_enhance_u8(int device, const uint8_t* src, int h, int w, uint8_t* dst, void* workspace, size_t workspace_bytes, void* stream) {
    const int32_t* t;
    OCRVI_TRY(check_page("enhance_u8", device, src, h, w, dst, &t));
    OCRVI_CHECK(workspace, OCRVI_EINVAL, "enhance_u8: null workspace");
    const size_t need = LUT_BYTES + 2 * page_bytes(h, w);
    OCRVI_CHECK(workspace_bytes >= need, OCRVI_ENOMEM, "enhance_u8: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    DeviceGuard dg(device);
    OCRVI_HIP(dg.err);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* lut = (uint8_t*)workspace;
    uint8_t* A = lut + LUT_BYTES;
    uint8_t* B = A + page_bytes(h, w);
    OCRVI_TRY(launch_px<PX_RGB2LAB>(src, A, h, w, t, nullptr, st));               // scanner.py:60
    OCRVI_TRY(launch_lut(A, h, w, lut, st));                                      // :63-64
    OCRVI_TRY(launch_px<PX_CLAHE_RGB_LAB>(A, B, h, w, t, lut, st));               // :64-67, and the Lab conversion inside :70
    OCRVI_TRY(launch_nlm(B, A, h, w, t, st));                                     // :70
    OCRVI_TRY(launch_px<PX_LAB2RGB>(A, B, h, w, t, nullptr, st));                 // :70, back to RGB
    return launch_sharpen(B, dst, h, w, st);                                      // :73-74
}
