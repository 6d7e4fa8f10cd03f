// Direct grouped 3x3 convolution with 32 channels per group (stride 1, pad 1) for the f16x2 mode: SVTRv2's LocalMixing pair
// (svtrv2.py:47-63).  gconv32.h's structure at 4 bytes per element, on a tile that spans the whole height of the recogniser's maps.
//
// As an implicit GEMM (conv_gemm 128 x 32) the layer gathers every pixel's 128-byte group slice nine times from L2 for a GEMM of 32
// columns.  Here a persistent workgroup of 4 waves owns ONE group: it stages the group's 9 x 32 x 32 weights in LDS once (36 KiB, already
// regrouped into (hi, lo) quartets: a weight fragment is two ds_read_b128 and no register moves), and per tile the zero-padded halo
// patch of the group's pixel slices, from which all nine taps' MFMA operands are read: fragment rows are 16 consecutive pixels of an
// image row shifted by the tap, K = the group's 32 input channels = one 128-byte K-step.
//   * Tile: bh rows x 16 nbx columns with bh = the image height up to 12 rows (taller images: bands of 12) and bh * nbx <= 12 MFMA blocks,
//     three per wave: 12 x 16 at H = 12, 6 x 32 at H = 6.  A tile that spans the image has no halo rows to load: the rows above and
//     below are the zero border (gconv32's 4-row tile loads 6 rows for 4).  Halo (at most 288 pixels, 36 KiB) + weights = 72 KiB: two
//     workgroups per CU.
//   * The next tile's patch is loaded into registers (plain clamped loads; the zero mask is applied at the LDS store) and written to LDS
//     behind the barrier that ends the current tile's MFMAs.  conv1 requests it ahead of those MFMAs, as gconv32 does; conv2 refills the
//     registers with the tile after next as soon as they are stored, so patch loads are in flight under its epilogue too.  The fp32
//     residual of a tile is requested ahead of its MFMAs.
//   * Pixel and weight rows are 128 bytes, XOR-swizzled by swz_halo: fragment reads that start at any pixel are conflict-free.
//   * f16x2 arithmetic: Mma::regroup / three (the lo lo product is dropped, as in conv3_halo), K in ascending (tap, channel) order, fp32
//     accumulation.  A lane's four accumulator values of an N-block are four consecutive channels of one pixel: every store is 16 bytes.
//   * Epilogues (the two the model has): act(acc wscale + bias) -> f16x2 with the range check; act(acc wscale + bias) + fp32 residual ->
//     fp32, each element read and then written by the same lane, so the residual may be the output buffer.
// Workgroup id = slot * groups + group: the groups of one tile are neighbours in launch order and read the 4 / 8 / 12 parts of a pixel
// row at about the same time (the other order, group-major, measures the same: profiles/r31_gconv_x2.md).  Neither the tiling nor the K order depends on n_img: an image alone and inside a batch give the same bits.
#include <stdlib.h>

#include "gconv32.h"
#include "kernels.h"

namespace ocrvi {
OCRVI_RANGE_FLAG_TU()

constexpr int GX_MAX_BH = 12;        // rows per tile
constexpr int GX_MAX_BLK = 12;       // 16-pixel MFMA blocks per tile (three per wave)
constexpr int GX_MAX_NBX = 4;
constexpr int GX_HALO_PIX = 288;     // halo pixels per tile at most (36 KiB)
constexpr int GX_W_BYTES = 9 * 32 * 128;

// 16-pixel blocks per tile row for a band of bh rows of an image W wide
static inline int gx_nbx(int bh, int W) {
    int nbx = std::min(std::min(GX_MAX_BLK / bh, GX_MAX_NBX), cdiv(W, 16));
    while (nbx > 1 && (bh + 2) * (16 * nbx + 2) > GX_HALO_PIX) --nbx;
    return nbx;
}
// halo pixel index -> (row, column) by gconv32's multiplication, exact for every pixel of every tile gx_nbx can choose
constexpr bool gx_hw_magic_exact() {
    for (int nbx = 1; nbx <= GX_MAX_NBX; ++nbx) {
        const int hw = 16 * nbx + 2;
        for (int pix = 0; pix < GX_HALO_PIX; ++pix)
            if ((int)(((unsigned)pix * gc_hw_magic(hw)) >> 16) != pix / hw) return false;
    }
    return true;
}
static_assert(gx_hw_magic_exact(), "gconv_x2: the halo-index multiplication is not exact for every pixel of a tile");
static_assert((GX_MAX_BH + 2) * 18 <= GX_HALO_PIX, "gconv_x2: a 12-row tile of one block does not fit the halo");

template <bool F32O>
__global__ __launch_bounds__(256, 2) void gconv_x2_kernel(const ConvParams p, int bh, int nbx, int bands_y, int bands_x, unsigned hw_magic) {
    typedef f16x2_t T;
    typedef Mma<T>::u4v U;
    constexpr int MB = GX_MAX_BLK / 4;                       // M-blocks per wave
    constexpr int HPASS = GX_HALO_PIX * 8 / 256, WPASS = (32 * 36 + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, g4 = lane >> 4;
    const int TW = 16 * nbx, HW = TW + 2, HH = bh + 2;
    char* const halo = smem;
    char* const wl = smem + HH * HW * 128;
    const int gp = (int)blockIdx.x % p.groups, G = (int)gridDim.x / p.groups;
    const int ntile = p.n_img * bands_y * bands_x;
    const char* const Xg = (const char*)p.x + (size_t)(p.cin_off + gp * 32) * 4;
    const size_t pix_b = (size_t)p.Cin * 4;
    uint4 hv[HPASS];
    const int htotal = HH * HW * 8;                          // 16-byte chunks of the halo patch
    auto tile_origin = [&](int t, int& img, int& y0, int& x0) {
        const int bx = t % bands_x;
        t /= bands_x;
        const int by = t % bands_y;
        img = t / bands_y;
        y0 = by * bh;
        x0 = bx * TW;
    };
    // All loads are unconditional (clamped addresses, value masked at the LDS store); whole passes past the patch are skipped (uniform).
    auto fetch = [&](int t) {
        int img, y0, x0;
        tile_origin(t, img, y0, x0);
        const char* X = Xg + (size_t)img * p.H * p.W * pix_b;
#pragma unroll
        for (int k = 0; k < HPASS; ++k) {
            if (256 * k < htotal) {
                const int i = min(tid + 256 * k, htotal - 1);
                const int pix = i >> 3, c = i & 7;
                const int hy = (int)(((unsigned)pix * hw_magic) >> 16), hx = pix - hy * HW;
                const int iy = min(max(y0 + hy - 1, 0), p.H - 1), ix = min(max(x0 + hx - 1, 0), p.W - 1);
                hv[k] = *(const uint4*)(X + ((size_t)iy * p.W + ix) * pix_b + c * 16);
            }
        }
    };
    auto stage = [&](int t) {  // registers -> LDS, zeros outside the image
        int img, y0, x0;
        tile_origin(t, img, y0, x0);
#pragma unroll
        for (int k = 0; k < HPASS; ++k) {
            const int i = tid + 256 * k;
            if (i < htotal) {
                const int pix = i >> 3, c = i & 7;
                const int hy = (int)(((unsigned)pix * hw_magic) >> 16), hx = pix - hy * HW;
                const int iy = y0 + hy - 1, ix = x0 + hx - 1;
                const bool in = (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                *(uint4*)(halo + pix * 128 + ((c ^ swz_halo(pix)) << 4)) = in ? hv[k] : make_uint4(0, 0, 0, 0);
            }
        }
    };
    int tile = (int)blockIdx.x / p.groups;
    if (tile >= ntile) return;
    fetch(tile);
    {   // the group's 9 x 32 x 32 weights, once: row tap * 32 + n, the 8 k-slots of lane group q as quartets (hi at 2 q, lo at 2 q + 1)
        const char* Wg = (const char*)p.w + (size_t)gp * p.Np * p.Kp * 4;   // [n][tap * 32 + c], chunk form
        uint4 wv[WPASS][2];
#pragma unroll
        for (int k = 0; k < WPASS; ++k) {
            const int i = min(tid + 256 * k, 32 * 36 - 1);
            const int n = i / 36, rem = i - n * 36, tap = rem >> 2, q = rem & 3;
            const char* s = Wg + (size_t)n * p.Kp * 4 + tap * 128 + q * 32;
            wv[k][0] = *(const uint4*)s;
            wv[k][1] = *(const uint4*)(s + 16);
        }
#pragma unroll
        for (int k = 0; k < WPASS; ++k) {
            const int i = tid + 256 * k;
            if (i < 32 * 36) {
                const int n = i / 36, rem = i - n * 36, tap = rem >> 2, q = rem & 3;
                const int row = tap * 32 + n, sw = swz_halo(row);
                *(uint4*)(wl + row * 128 + (((2 * q) ^ sw) << 4)) = make_uint4(wv[k][0].x, wv[k][0].y, wv[k][1].x, wv[k][1].y);
                *(uint4*)(wl + row * 128 + (((2 * q + 1) ^ sw) << 4)) = make_uint4(wv[k][0].z, wv[k][0].w, wv[k][1].z, wv[k][1].w);
            }
        }
    }
    stage(tile);
    __syncthreads();
    const int nblk = bh * nbx;
    // wave w owns M-blocks w, w + 4, w + 8: block mb = tile row mb / nbx, 16 pixels from column 16 (mb % nbx).  A block past the tile
    // (small images) repeats the last one and stores nothing: the MFMA loop has no branch.
    int pbase[MB], bty[MB], btb[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int mb = min(wave + 4 * m, nblk - 1);
        bty[m] = mb / nbx;
        btb[m] = mb - bty[m] * nbx;
        pbase[m] = bty[m] * HW + btb[m] * 16 + lr;           // tap (0, 0) = halo pixel (ty, 16 tb + lr)
    }
    // weight row of MFMA row lr: tap * 32 + 16 nb + lr, swz_halo(row) = swz_halo(lr)
    const int wo = lr * 128 + (((2 * g4) ^ swz_halo(lr)) << 4);
    float4 bias_r[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) bias_r[nb] = p.bias ? *(const float4*)(p.bias + gp * 32 + nb * 16 + 4 * g4) : make_float4(0.f, 0.f, 0.f, 0.f);
    auto activate = [&](float (&v)[4]) {
        if (p.act == ACT_RELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        } else if (p.act == ACT_GELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
        }
    };
    unsigned long long bad = 0;
    // The next tile's patch is requested ahead of the current tile's MFMAs (conv1), or (conv2, EARLY) the patch registers are refilled as
    // soon as they have been written to LDS, so that the loads of the tile after next are in flight under this tile's longer epilogue,
    // the barrier and the next tile's MFMAs.  conv1 measured slower that way (profiles/r31_gconv_x2.md, which has conv2's figures too).
    constexpr bool EARLY = F32O;
    int next = tile + G;
    if (EARLY && next < ntile) fetch(next);
    for (;;) {
        if (!EARLY && next < ntile) fetch(next);
        int img, y0, x0;
        tile_origin(tile, img, y0, x0);
        bool ok[MB];
        size_t opix[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            const int y = y0 + bty[m], x = x0 + btb[m] * 16 + lr;
            ok[m] = wave + 4 * m < nblk && y < p.H && x < p.W;
            opix[m] = ok[m] ? ((size_t)img * p.H + y) * p.W + x : 0;
        }
        float4 rres[MB][2];                                  // fp32 residual of this tile, requested ahead of the MFMAs
        if constexpr (F32O) {
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)   // (a lane without a pixel reads nothing: in place another workgroup may be writing what it would read)
                    rres[m][nb] = ok[m] ? *(const float4*)((const float*)p.res + opix[m] * p.ldr + gp * 32 + nb * 16 + 4 * g4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // ---- MFMA: K in ascending (tap, channel) order
        f32x4 acc[MB][2];
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[m][0] = acc[m][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - r * 3;
            U wH[2], wL[2];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const char* wr = wl + (tap * 32 + nb * 16) * 128 + wo;
                wH[nb] = Mma<T>::as_u4v(*(const uint4*)wr);
                wL[nb] = Mma<T>::as_u4v(*(const uint4*)(wl + (tap * 32 + nb * 16) * 128 + (wo ^ 16)));
            }
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const int pp = pbase[m] + r * HW + s;
                const int o = pp * 128 + (((2 * g4) ^ swz_halo(pp)) << 4);
                U xH, xL;
                Mma<T>::regroup(*(const uint4*)(halo + o), *(const uint4*)(halo + (o ^ 16)), xH, xL);
                Mma<T>::three(wH[0], wL[0], xH, xL, acc[m][0]);
                Mma<T>::three(wH[1], wL[1], xH, xL, acc[m][1]);
            }
        }
        __syncthreads();  // every wave is done reading the halo tile
        const int after = next + G;
        if (next < ntile) {
            stage(next);
            if (EARLY && after < ntile) fetch(after);
        }
        // ---- epilogue of the current tile (registers only; overlaps the other waves' LDS stores)
#pragma unroll
        for (int m = 0; m < MB; ++m) {
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const int ch = gp * 32 + nb * 16 + 4 * g4;
                float v[4] = {unscale<T>(acc[m][nb][0], p.wscale) + bias_r[nb].x, unscale<T>(acc[m][nb][1], p.wscale) + bias_r[nb].y,
                              unscale<T>(acc[m][nb][2], p.wscale) + bias_r[nb].z, unscale<T>(acc[m][nb][3], p.wscale) + bias_r[nb].w};
                activate(v);
                if constexpr (F32O) {
                    const float4 rv = rres[m][nb];
                    if (ok[m])
                        *(float4*)((float*)p.out + opix[m] * p.ldo + p.out_coff + ch) = make_float4(v[0] + rv.x, v[1] + rv.y, v[2] + rv.z, v[3] + rv.w);
                } else {
                    bad |= f16x2_out_of_range(v) & __builtin_amdgcn_ballot_w64(ok[m]);
                    if (ok[m]) *(uint4*)((char*)p.out + (opix[m] * p.ldo + p.out_coff + ch) * 4) = Chunk<T>::pack(v);
                }
            }
        }
        if (next >= ntile) break;
        tile = next;
        next = after;
        __syncthreads();  // the next tile's halo is in LDS
    }
    if constexpr (!F32O) f16x2_raise(bad);
}

// ---------------------------------------------------------------- host
GconvX2Plan gconv_x2_plan(int n_img, int H, int W, int groups, int n_cu, int max_workgroups) {
    GconvX2Plan r;
    r.bh = std::min(H, GX_MAX_BH);                           // the whole image up to 12 rows, bands of 12 above
    r.nbx = gx_nbx(r.bh, W);
    r.bands_y = cdiv(H, r.bh);
    r.bands_x = cdiv(W, 16 * r.nbx);
    r.ntile = n_img * r.bands_y * r.bands_x;
    int slots = std::max(1, 2 * n_cu / groups);              // two persistent workgroups per CU over all groups
    if (max_workgroups > 0) slots = std::min(slots, max_workgroups);
    r.grid_x = persistent_grid(r.ntile, slots);
    r.tiles_min = r.ntile / r.grid_x;
    r.tiles_max = cdiv(r.ntile, r.grid_x);
    r.smem = (r.bh + 2) * (16 * r.nbx + 2) * 128 + GX_W_BYTES;
    return r;
}

// a LocalMixing-shaped f16x2 call with one of the kernel's two epilogues
static bool gconv_x2_takes(const ConvParams& p, int dtype) {
    if (dtype != OCRVI_F16X2 || p.groups < 2 || p.Cin_g != 32 || p.N_g != 32 || p.Np != 32 || p.KH != 3 || p.w_quartets) return false;
    if (p.SH != 1 || p.SW != 1 || p.PH != 1 || p.PW != 1 || p.H != p.OH || p.W != p.OW || p.H < 1 || p.W < 1 || p.store_mode != ST_NHWC) return false;
    if (p.Kp < 288 || p.Kp % 4 != 0 || p.Cin % 4 != 0 || p.cin_off % 4 != 0 || p.cin_off + p.groups * 32 > p.Cin) return false;
    if (!p.x || !p.w || !p.out || ((uintptr_t)p.x & 15) != 0 || ((uintptr_t)p.w & 15) != 0 || ((uintptr_t)p.out & 15) != 0) return false;
    if (p.bias && ((uintptr_t)p.bias & 15) != 0) return false;
    if (p.ldo % 4 != 0 || p.out_coff % 4 != 0 || p.out_coff + p.groups * 32 > p.ldo) return false;
    if (p.act != ACT_NONE && p.act != ACT_RELU && p.act != ACT_GELU) return false;
    if ((size_t)p.n_img * p.H * p.W >= ((size_t)1 << 23)) return false;
    if (p.out_f32)   // act(..) + fp32 residual -> fp32
        return p.res_mode == RES_SAME && p.res && p.res_f32 && p.res_post && p.ldr % 4 == 0 && p.groups * 32 <= p.ldr && ((uintptr_t)p.res & 15) == 0;
    return p.res_mode == RES_NONE;   // act(..) -> f16x2
}
bool gconv_x2_eligible(const ConvParams& p, int dtype) { return gconv32_on() && gconv_x2_takes(p, dtype); }

int k_gconv_x2(const ConvParams& p, hipStream_t stream, int max_workgroups) {
    OCRVI_CHECK(gconv_x2_takes(p, OCRVI_F16X2), OCRVI_EINVAL, "gconv_x2: not a grouped 3x3 call this kernel takes (Cin_g %d, N_g %d, out_f32 %d, res %d)",
                p.Cin_g, p.N_g, p.out_f32, p.res_mode);
    int n_cu = 0;
    OCRVI_TRY(device_cus(&n_cu));
    const GconvX2Plan pl = gconv_x2_plan(p.n_img, p.H, p.W, p.groups, n_cu, max_workgroups);
    const double px = (double)p.n_img * p.H * p.W, ch = 32.0 * p.groups;
    char tag[64];
    snprintf(tag, sizeof(tag), "gconv_x2_f16x2 M%d g%d %s", p.n_img * p.H * p.W, p.groups, p.out_f32 ? "res_f32" : "f16x2");
    // algorithmic bytes: input read once, weights once, output written once (+ the residual read once)
    ProfScope ps(tag, 2.0 * px * ch * 288.0, px * ch * 4.0 + ch * 288.0 * 4.0 + px * ch * 4.0 + (p.out_f32 ? px * ch * 4.0 : 0.0), stream);
    const dim3 grid(pl.grid_x * p.groups);
    if (p.out_f32) {
        auto k = gconv_x2_kernel<true>;
        OCRVI_TRY(ensure_max_smem((const void*)k, 80 * 1024));
        hipLaunchKernelGGL(k, grid, dim3(256), pl.smem, stream, p, pl.bh, pl.nbx, pl.bands_y, pl.bands_x, gc_hw_magic(16 * pl.nbx + 2));
    } else {
        auto k = gconv_x2_kernel<false>;
        OCRVI_TRY(ensure_max_smem((const void*)k, 80 * 1024));
        hipLaunchKernelGGL(k, grid, dim3(256), pl.smem, stream, p, pl.bh, pl.nbx, pl.bands_y, pl.bands_x, gc_hw_magic(16 * pl.nbx + 2));
    }
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

}  // namespace ocrvi
