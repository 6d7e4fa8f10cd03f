// Direct (halo-resident) 3x3 / stride 1 / pad 1 convolution for f16x2 with 64, 128 or 256 output channels: the detector's dense 3x3 layers
// (FPN smoothing convs, head_conv, ResNet layer1 conv2).  As an implicit GEMM (conv_gemm_kernel, 128x128 tile) every tap of every
// 128-pixel tile re-reads its input rows from L2 / HBM: about 7x the algorithmic input per launch, and at 4 bytes per element the operand
// feed, not the matrix pipe, capped those layers at ~0.35 of the f16x2 roof.
//
// Here a persistent workgroup of 8 waves (two per SIMD) owns a 16 x 16 tile of output pixels and NC = 64 or 128 output channels (256-column
// layers run as two column tiles of 128: a 256-column tile, 128 accumulator registers per wave, spills at two waves per SIMD).  Per 128-byte
// channel block (32 channels) the tile's 18 x 18 input patch is DMA'd (global_load_lds_dwordx4) into one of two LDS stages ONCE, one channel
// block ahead; the nine taps' MFMA pixel operands are all read from it (the fragment of tap (dy, dx) for output row y is the 16 patch
// pixels (y + dy) * 18 + dx + 0..15).  The weights stream per (channel block, tap) unit -- Np rows x 128 B, `sc1` (a layer's weights stay
// resident in L2) -- through a ring of NWS units (64 KiB in all: 4 / 8 units for 128 / 64 columns), NWS - 1 units ahead.  One counted
// vmcnt wait + barrier per unit.  The waves split the tile as WP pixel groups x WC column groups of 64 channels (RW output rows x four
// 16-channel blocks each: 4 x 4 or 2 x 4 accumulator blocks), in two passes of two blocks (16 weight registers).
//
// Patch (and weight) rows are XOR-swizzled by bits 1 and 2 of the pixel (row) index (swz_halo): fragment reads that start at ANY pixel are
// conflict-free under the gfx950 ds_read_b128 lane groups (each group reads chunks {c, c ^ 2} of 8 consecutive pixels mod 8; the swizzle
// maps those 16 reads onto 16 distinct 16-byte bank slots), where offs_conv's swz128 (bits 1 and 3) is 2-way conflicted.
//
// f16x2 arithmetic as everywhere: Mma<f16x2_t>::regroup / three, fp32 accumulation.  The K order is (channel block, tap, channel) instead
// of the implicit GEMM's (tap, channel): results differ from conv_gemm by fp32 rounding only.  Neither the kernel choice nor the K order
// depends on n_img or M (a page alone and inside a batch give the same bits).  OCRVI_CONV3_HALO=0 falls back to conv_gemm.
//
// vmcnt protocol (per wave, VMEM ops retire in issue order): at step s the wait must cover weight unit s.  Younger than it are the NWS - 2
// later units (WPW pieces each), the patch of the next stage when it was issued at tap 0 of this stage after unit s (taps 1 .. NWS - 2:
// at least PPW_MIN pieces per wave), and the previous tile's epilogue stores when they came after unit s (STORES per wave, unconditional:
// out-of-range lanes store to the dump page).  Past the last step the stream keeps issuing (harmless units into free slots, a zero patch),
// so these counts never change; the range flag's store can only add younger operations (a longer wait, never a shorter one).
#pragma once
#include "gemm_ring.h"

namespace ocrvi {

__device__ __forceinline__ int swz_halo(int row) { return ((row >> 1) & 1) | (((row >> 2) & 1) << 2); }

template <int NC> struct HaloCfg {
    static constexpr int TH = 16, TW = 16, PH = TH + 2, PW = TW + 2, NPIX = PH * PW;   // 18 x 18 patch
    static constexpr int NI_P = (NPIX + 7) / 8;                    // 41 1-KiB patch pieces per stage (8 pixels x 128 B)
    static constexpr int PSLOTS = (NI_P + 7) / 8, PPW_MIN = NI_P / 8;   // pieces per wave: 6 for wave 0, 5 for the others
    static constexpr int PATCH = NI_P * 1024;
    static constexpr int WU = NC * 128, WPW = NC / 64;            // weight unit bytes; pieces per wave per unit
    static constexpr int NWS = 65536 / WU;                         // weight ring slots
    static constexpr int WC = NC / 64, WP = 8 / WC, RW = TH / WP;  // column groups, pixel groups, output rows per wave
    static constexpr int STORES = RW * 4;                          // epilogue stores per wave per tile
    static constexpr int BIAS = 2 * PATCH + NWS * WU;              // fp32 bias of the NC columns
    static constexpr int SMEM = BIAS + NC * 4;
    static_assert(NC == 64 || NC == 128 || NC == 256, "columns");
    static_assert(NWS >= 2 && NWS - 2 <= 8, "ring depth");
    static_assert((NWS - 2) * WPW + PPW_MIN + STORES < 64, "vmcnt is a 6-bit counter");
    static_assert(SMEM <= 160 * 1024, "LDS");
};

template <typename T, int NC, int ACT>
__global__ __launch_bounds__(512, 2) void conv3_halo_kernel(const ConvParams p, int tiles_x, int tiles_y) {
    using C = HaloCfg<NC>;
    constexpr int PW = C::PW, NI_P = C::NI_P, PSLOTS = C::PSLOTS, WPW = C::WPW, NWS = C::NWS, WC = C::WC, RW = C::RW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, g = lane >> 4;
    const int wc = wave % WC, wp = wave / WC;
    const int ncb = p.Cin_g / 32;
    const int ntile = p.n_img * tiles_y * tiles_x;
    // workgroup = (row lane, column tile nt): it keeps its NC columns; the column tiles of one row lane are consecutive ids (one XCD),
    // so they walk the same pixel tiles side by side and the second patch read is an L2 hit
    const int nct = p.Np / NC, G = gridDim.x / nct;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int nt = wg % nct, first = wg / nct;
    const int my_tiles = first < ntile ? (ntile - first + G - 1) / G : 0;
    const int col0 = nt * NC;
    const char* const X = (const char*)p.x + (size_t)p.cin_off * 4;
    const char* const zero = (const char*)p.zero_page + (lane & 7) * 16;
    const int pix_b = p.Cin * 4, wrow_b = p.Kp * 4;

    {   // bias of the NC columns into LDS (0 past N_g / without bias)
        float* bl = (float*)(smem + C::BIAS);
        for (int n = tid; n < NC; n += 512) bl[n] = (p.bias && col0 + n < p.N_g) ? p.bias[col0 + n] : 0.f;
        __syncthreads();
    }

    // ---- weight stream: unit u = (cb, tap) of the cyclic sequence cb-major; piece j of this wave = rows (wave + 8 j) * 8 + lane / 8
    unsigned wvoff[WPW];
#pragma unroll
    for (int j = 0; j < WPW; ++j) {
        const int n = (wave + 8 * j) * 8 + (lane >> 3), cq = lane & 7;
        wvoff[j] = (unsigned)(n * wrow_b + ((cq ^ swz_halo(n)) << 4));
    }
    int wi_cb = 0, wi_tap = 0, wi_s = 0;   // next unit to issue, and its step index (-> ring slot)
    auto issue_w = [&]() {
        const char* base = uniform_ptr((const char*)p.w + (size_t)col0 * wrow_b + (size_t)(wi_tap * p.Cin_g + wi_cb * 32) * 4);
        const unsigned dst = lds0 + 2 * C::PATCH + (wi_s & (NWS - 1)) * C::WU;
#pragma unroll
        for (int j = 0; j < WPW; ++j) glds16_sc1(base, wvoff[j], __builtin_amdgcn_readfirstlane(dst + (wave + 8 * j) * 1024));
        ++wi_s;
        if (++wi_tap == 9) { wi_tap = 0; if (++wi_cb == ncb) wi_cb = 0; }
    };

    // ---- patch stream: stage k = (my tile k / ncb, channel block k % ncb); per-lane sources of channel block 0 rebuilt per tile
    const char* src[PSLOTS];
    int pi_tile = 0, pi_cb = 0, pi_k = 0;
    auto setup_tile = [&](int t) {
        const bool live = t < my_tiles;
        const int tile = first + t * G;
        const int tx = tile % tiles_x, r = tile / tiles_x, ty = r % tiles_y, img = r / tiles_y;
        const int y0 = ty * C::TH - 1, x0 = tx * C::TW - 1;
#pragma unroll
        for (int j = 0; j < PSLOTS; ++j) {
            const int pp = (wave + 8 * j) * 8 + (lane >> 3), cq = lane & 7;
            const int py = pp / PW, px = pp - py * PW;
            const int iy = y0 + py, ix = x0 + px;
            const char* s = zero;
            if (live && pp < C::NPIX && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W)
                s = X + ((size_t)(img * p.H + iy) * p.W + ix) * pix_b + ((cq ^ swz_halo(pp)) << 4);
            src[j] = s;
        }
    };
    auto issue_patch = [&]() {
        if (pi_cb == 0) setup_tile(pi_tile);
        const unsigned base = lds0 + (pi_k & 1) * C::PATCH;
#pragma unroll
        for (int j = 0; j < PSLOTS; ++j) {
            const int i = wave + 8 * j;
            if (i < NI_P) {                                        // (wave-uniform)
                const bool is_zero = src[j] == zero;
                glds16v(is_zero ? src[j] : src[j] + (size_t)pi_cb * 128, __builtin_amdgcn_readfirstlane(base + i * 1024));
            }
        }
        ++pi_k;
        if (++pi_cb == ncb) { pi_cb = 0; ++pi_tile; }
    };

    if (my_tiles == 0) return;
    issue_patch();
#pragma unroll
    for (int u = 0; u < NWS - 1; ++u) issue_w();

    typedef typename Mma<T>::u4v U;
    f32x4 acc[RW][4];
    const int row0 = wp * RW;                                          // first output row of this wave in the tile
    const int ncol0 = wc * 64;
    // Per-lane fragment offsets.  Pixel fragment of patch pixel pp = 18 row0 + lr + k: byte pp * 128 + (chunk ^ swz_halo(pp)) * 16, and
    // swz_halo only sees pp mod 8, so xoff[k mod 8][h] + k * 128 (k compile-time: an immediate) addresses it
    // (xoff also carries the byte offset of the current patch buffer).  Weight row n = ncol0 + 16 a + lr:
    // swz_halo(n) = swz_halo(lr).
    int xoff[8][2], woff[2];
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int pp = row0 * PW + lr;
            xoff[m][h] = pp * 128 + (((2 * g + h) ^ swz_halo(pp + m)) << 4);
        }
#pragma unroll
    for (int h = 0; h < 2; ++h) woff[h] = (ncol0 + lr) * 128 + (((2 * g + h) ^ swz_halo(lr)) << 4);
    int s = 0;                                                         // step (= weight unit) index
    int pcur = 0;                                                      // patch buffer offset xoff holds
    for (int t = 0; t < my_tiles; ++t) {
        for (int cb = 0; cb < ncb; ++cb) {
            const bool after_epi = cb == 0 && t > 0;
            {   // this stage's patch buffer, folded into the per-lane offsets (in place: no second set of 16 registers)
                const int want = ((t * ncb + cb) & 1) * C::PATCH, d = want - pcur;
                pcur = want;
#pragma unroll
                for (int m = 0; m < 8; ++m) { xoff[m][0] += d; xoff[m][1] += d; }
            }
            auto step = [&](auto tc) {
                constexpr int TAP = decltype(tc)::value, DY = TAP / 3, DX = TAP % 3;
                constexpr int NB = (NWS - 2) * WPW + ((TAP >= 1 && TAP <= NWS - 2) ? C::PPW_MIN : 0);
                constexpr int NA = NB + (TAP <= NWS - 2 ? C::STORES : 0);
                if (after_epi) wait_vm_barrier<NA>(); else wait_vm_barrier<NB>();
                if constexpr (TAP == 0) issue_patch();   // next stage into the patch buffer every wave is done reading
                issue_w();                            // unit s + NWS - 1 into the slot of unit s - 1
                if (TAP == 0 && cb == 0) {   // (first unit of a tile)
#pragma unroll
                    for (int r = 0; r < RW; ++r)
#pragma unroll
                        for (int a = 0; a < 4; ++a) acc[r][a] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
                const char* const Ws = smem + 2 * C::PATCH + (s & (NWS - 1)) * C::WU;
                // two passes over the wave's rows, one per pair of 16-channel blocks: 16 weight registers instead of 32 (the pixel fragments
                // are read twice; LDS bandwidth has room for it, the register file does not)
#pragma unroll
                for (int ap = 0; ap < 2; ++ap) {
                    if (ap) asm volatile("" ::: "memory");   // (re-read: left alone hipcc keeps the first pass's fragments live)
                    U wH[2], wL[2];
#pragma unroll
                    for (int a = 0; a < 2; ++a)
                        Mma<T>::regroup(lds16(Ws + woff[0] + (2 * ap + a) * 16 * 128), lds16(Ws + woff[1] + (2 * ap + a) * 16 * 128), wH[a], wL[a]);
                    uint4 xf[2][2];
                    auto rdx = [&](int r, int set) {   // (r, DY, DX compile-time: the pixel offset is the ds_read's immediate)
                        const int k = (r + DY) * PW + DX;
                        xf[set][0] = lds16(smem + xoff[k & 7][0] + k * 128);
                        xf[set][1] = lds16(smem + xoff[k & 7][1] + k * 128);
                    };
                    rdx(0, 0);
                    // (fenced: hipcc otherwise sinks each fragment read to its first MFMA behind an lgkmcnt(0))
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < RW; ++r) {
                        if (r + 1 < RW) rdx(r + 1, (r + 1) & 1);
                        __builtin_amdgcn_sched_barrier(0);
                        U xH, xL;
                        Mma<T>::regroup(xf[r & 1][0], xf[r & 1][1], xH, xL);
#pragma unroll
                        for (int a = 0; a < 2; ++a) Mma<T>::three(wH[a], wL[a], xH, xL, acc[r][2 * ap + a]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                ++s;
            };
            step(IC<0>()); step(IC<1>()); step(IC<2>()); step(IC<3>()); step(IC<4>());
            step(IC<5>()); step(IC<6>()); step(IC<7>()); step(IC<8>());
        }
        // ---- epilogue: + bias, activation, range check, f16x2 chunks of 4 channels; every lane stores (dump page when out of range)
        const int tile = first + t * G;
        const int tx = tile % tiles_x, r_ = tile / tiles_x, ty = r_ % tiles_y, img = r_ / tiles_y;
        const int ox = tx * C::TW + lr;
        const float* bl = (const float*)(smem + C::BIAS);
        unsigned long long bad = 0;
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int oy = ty * C::TH + row0 + r;
            const bool pix_ok = oy < p.OH && ox < p.OW;
            char* const orow = (char*)p.out + (((size_t)(img * p.OH + oy) * p.OW + ox) * p.ldo + p.out_coff) * 4;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int n = ncol0 + a * 16 + 4 * g;
                const float4 bv = *(const float4*)(bl + n);
                float v[4] = {unscale<T>(acc[r][a][0], p.wscale) + bv.x, unscale<T>(acc[r][a][1], p.wscale) + bv.y,
                              unscale<T>(acc[r][a][2], p.wscale) + bv.z, unscale<T>(acc[r][a][3], p.wscale) + bv.w};
                if constexpr (ACT == ACT_RELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                const bool ok = pix_ok && col0 + n < p.N_g;
                bad |= f16x2_out_of_range(v) & __builtin_amdgcn_ballot_w64(ok);
                char* dst = ok ? orow + (size_t)(col0 + n) * 4 : (char*)p.dump_page + lane * 16;
                *(uint4*)dst = Chunk<T>::pack(v);
            }
        }
        f16x2_raise(bad);
    }
    wait_vm_only<0>();
}

bool conv3_halo_eligible(const ConvParams& p, int amode, int dtype);   // host_util.hip

template <typename T, int NC, int ACT>
static int launch_conv3_halo_t(const ConvParams& p_in, int n_cu, hipStream_t stream) {
    using C = HaloCfg<NC>;
    ConvParams p = p_in;
    OCRVI_TRY(ring_pages(&p.zero_page, &p.dump_page));
    const int tiles_x = cdiv(p.OW, C::TW), tiles_y = cdiv(p.OH, C::TH);
    const int ntile = p.n_img * tiles_y * tiles_x, nct = p.Np / NC;
    int gm = std::min(ntile, std::max(1, n_cu / nct));
    gm = cdiv(ntile, cdiv(ntile, gm));   // equal tile counts
    const int grid = gm * nct;
    auto kern = conv3_halo_kernel<T, NC, ACT>;
    OCRVI_TRY(ensure_max_smem((const void*)kern, C::SMEM));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), C::SMEM, stream, p, tiles_x, tiles_y);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

template <typename T, int NC>
static int launch_conv3_halo_n(const ConvParams& p, int n_cu, hipStream_t stream) {
    if (p.act == ACT_RELU) return launch_conv3_halo_t<T, NC, ACT_RELU>(p, n_cu, stream);
    return launch_conv3_halo_t<T, NC, ACT_NONE>(p, n_cu, stream);
}

template <typename T>
static int launch_conv3_halo(const ConvParams& p, hipStream_t stream) {
    if constexpr (IsSplit<T>::value) {
        int n_cu = 0;
        OCRVI_TRY(device_cus(&n_cu));
        // (256 columns: two column tiles of 128.  A 256-column tile -- 128 accumulator registers per wave -- spills at two waves per SIMD)
        if (p.Np == 256 || p.Np == 128) return launch_conv3_halo_n<T, 128>(p, n_cu, stream);
        if (p.Np == 64) return launch_conv3_halo_n<T, 64>(p, n_cu, stream);
    }
    set_error("conv3_halo: unsupported call (Np=%d)", p.Np);
    return OCRVI_EINVAL;
}

}  // namespace ocrvi
