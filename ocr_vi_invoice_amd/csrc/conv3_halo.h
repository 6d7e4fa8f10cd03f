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
// 16-channel blocks each: 4 x 4 or 2 x 4 accumulator blocks), in ONE pass per unit with the four blocks' weight fragments in registers.
//
// Fragment reads run one stage ahead of the MFMAs that use them: a row's pixel fragment goes out under the MFMAs of the row before, and a
// unit's four weight fragments and first pixel row go out under the LAST row of the unit before -- across the unit's barrier, the
// patch-stage switch behind tap 8 and the tile boundary (ahead of the epilogue's stores).  Both waves of a SIMD pass a unit's barrier
// together, so an LDS round trip left between the barrier and the first MFMA stalls the matrix pipe outright.  The weights are packed on
// the host as (hi, lo) quartets (pack_conv / conv3_halo_packing: the layer's loader asks for it), so a weight fragment is two
// ds_read_b128 and no register regrouping; the pixel fragments (activations, chunk form) are regrouped once per unit and row.
//
// Patch (and weight) rows are XOR-swizzled by bits 1 and 2 of the pixel (row) index (swz_halo): fragment reads that start at ANY pixel are
// conflict-free under the gfx950 ds_read_b128 lane groups (each group reads chunks {c, c ^ 2} of 8 consecutive pixels mod 8; the swizzle
// maps those 16 reads onto 16 distinct 16-byte bank slots), where offs_conv's swz128 (bits 1 and 3) is 2-way conflicted.
//
// f16x2 arithmetic as everywhere: Mma<f16x2_t>::regroup / three, fp32 accumulation.  The K order is (channel block, tap, channel) instead
// of the implicit GEMM's (tap, channel): results differ from conv_gemm by fp32 rounding only.  Neither the kernel choice nor the K order
// depends on n_img or M (a page alone and inside a batch give the same bits).  OCRVI_CONV3_HALO=0 falls back to conv_gemm (read by the
// weight packer, which then keeps the chunk form that conv_gemm reads).
//
// vmcnt protocol (per wave, VMEM ops retire in issue order): at step s the wait must cover weight unit s + 1, not only unit s -- each wave
// waits for its own pieces of unit s + 1 BEFORE barrier s, so behind barrier s unit s + 1 is readable by every wave and the last row of
// step s may request its fragments.  (A prologue wait + barrier does the same for unit 0 and the first patch.)  issue_w at step s still
// refills the slot of unit s - 1, which nobody reads any more: its last readers were the MFMAs of step s - 1, in front of barrier s.
// Younger than unit s + 1 at the wait of step s are
//   * the NWS - 3 later units, WPW pieces each (one unit at 128 columns, five at 64);
//   * the patch of the next stage, issued at tap 0 of this stage between units s0 + NWS - 2 and s0 + NWS - 1 (s0 = the stage's first step):
//     younger than unit s + 1 at taps 1 .. NWS - 3 (at least PPW_MIN pieces per wave), older -- hence covered -- from tap NWS - 2 on.
//     Tap 8 >= NWS - 2 for every ring depth, so the patch has landed for every wave behind barrier (tap 8), where the look-ahead of the
//     next stage's tap 0 first reads it; with one channel block per tile (Cin = 32) that is the next TILE's patch, same count;
//   * the previous tile's epilogue stores, issued between the last step of a tile and step s0 of the next, i.e. behind unit s0 + NWS - 2:
//     younger than unit s + 1 at taps 0 .. NWS - 3 of the tile's first stage (STORES per wave, unconditional: out-of-range lanes store to
//     the dump page), older from tap NWS - 2 on.
// Past the last step the stream keeps issuing (harmless units into free slots, a zero patch), so these counts never change and the
// look-ahead behind the last unit of the last tile reads a landed, harmless unit; the range flag's store can only add younger operations
// (a longer wait, never a shorter one).
#pragma once
#include "gemm_ring.h"

namespace ocrvi {

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
    static_assert(NWS >= 4, "the wait of step s covers unit s + 1 and leaves NWS - 3 units in flight");
    static_assert(RW >= 2, "a unit's last row fetches the next unit's fragments, the rows before it the next row");
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
    int pbuf = 0;                                                      // patch buffer (0 / 1) whose offset xoff holds
    // The unit's four weight fragments and its first pixel row, requested one unit ahead (by `ahead`, under the last row of MFMAs of the
    // unit before) so that no LDS round trip stands between a unit's barrier and its first MFMA.
    U wH[4], wL[4];
    uint4 x0[2];
    auto ahead = [&](auto tn) {   // fragments of the unit with tap TN in ring slot (s + 1): legal once barrier s is passed (see the protocol)
        constexpr int TN = decltype(tn)::value, k = (TN / 3) * PW + TN % 3;
        const char* const Wn = smem + 2 * C::PATCH + ((s + 1) & (NWS - 1)) * C::WU;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            wH[a] = Mma<T>::as_u4v(lds16(Wn + woff[0] + a * 16 * 128));   // (hi, lo) quartets: packed that way (pack_conv)
            wL[a] = Mma<T>::as_u4v(lds16(Wn + woff[1] + a * 16 * 128));
        }
        x0[0] = lds16(smem + xoff[k & 7][0] + k * 128);
        x0[1] = lds16(smem + xoff[k & 7][1] + k * 128);
    };
    // unit 0 and the first patch have landed (younger: units 1 .. NWS - 2), for every wave: its fragments
    wait_vm_barrier<(NWS - 2) * WPW>();
    --s;
    ahead(IC<0>());
    ++s;
    for (int t = 0; t < my_tiles; ++t) {
        for (int cb = 0; cb < ncb; ++cb) {
            const bool after_epi = cb == 0 && t > 0;
            auto step = [&](auto tc) {
                constexpr int TAP = decltype(tc)::value, DY = TAP / 3, DX = TAP % 3;
                constexpr int NB = (NWS - 3) * WPW + ((TAP >= 1 && TAP <= NWS - 3) ? C::PPW_MIN : 0);
                constexpr int NA = NB + (TAP <= NWS - 3 ? C::STORES : 0);
                if (after_epi) wait_vm_barrier<NA>(); else wait_vm_barrier<NB>();
                if constexpr (TAP == 0) issue_patch();   // next stage into the patch buffer every wave is done reading
                issue_w();                            // unit s + NWS - 1 into the slot of unit s - 1
                if (TAP == 0 && cb == 0) {   // (first unit of a tile)
#pragma unroll
                    for (int r = 0; r < RW; ++r)
#pragma unroll
                        for (int a = 0; a < 4; ++a) acc[r][a] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
                // one pass over the wave's rows with all four 16-channel blocks' weights in registers; pixel rows one row ahead
                U cH[4], cL[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    cH[a] = wH[a]; cL[a] = wL[a];
                    asm volatile("" : "+v"(cH[a]), "+v"(cL[a]));   // (waited for here, ahead of the row reads below, not at the first MFMA behind them)
                }
                uint4 xf[RW][2];                   // (one name per row: each dies with its row's MFMAs, so two rows are live at a time)
                xf[0][0] = x0[0]; xf[0][1] = x0[1];
                auto rdx = [&](int r) {   // (r, DY, DX compile-time: the pixel offset is the ds_read's immediate)
                    const int k = (r + DY) * PW + DX;
                    xf[r][0] = lds16(smem + xoff[k & 7][0] + k * 128);
                    xf[r][1] = lds16(smem + xoff[k & 7][1] + k * 128);
                };
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    // This row's fragment (requested a row of MFMAs ago: it has landed) is regrouped first, then the next row's reads go out,
                    // then the MFMAs -- each part fenced: left alone hipcc sinks every read to its first use behind an lgkmcnt(0), and a read
                    // issued ahead of the regrouping gets a full wait directly behind it.
                    U xH, xL;
                    Mma<T>::regroup(xf[r][0], xf[r][1], xH, xL);
                    asm volatile("" : "+v"(xH), "+v"(xL));   // (the regrouping's moves are made here, not behind the reads below)
                    __builtin_amdgcn_sched_barrier(0);
                    if (r + 1 < RW) {
                        rdx(r + 1);
                    } else {   // the next unit's fragments; behind tap 8 they come from the other patch buffer, folded into the per-lane offsets
                        if constexpr (TAP == 8) {
                            const int d = pbuf ? -C::PATCH : C::PATCH;
                            pbuf ^= 1;
#pragma unroll
                            for (int m = 0; m < 8; ++m) { xoff[m][0] += d; xoff[m][1] += d; }
                        }
                        ahead(IC<(TAP + 1) % 9>());
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int a = 0; a < 4; ++a) Mma<T>::three(cH[a], cL[a], xH, xL, acc[r][a]);
                    __builtin_amdgcn_sched_barrier(0);
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

// The launch of conv3_halo_kernel (and of bneck_tail_kernel, whose phase A is the NC = 64 tile: Np = 64) as a pure function of the shape and
// the CU count: launch_conv3_halo / launch_bneck_tail_t launch on it and ocrvi_test_halo_plan reports it.
struct HaloPlan {
    int nc, nct;                 // columns of a column tile (256-column layers: two column tiles of 128), column tiles
    int tiles_x, tiles_y, ntile; // 16 x 16 pixel tiles across / down an image, in all
    int gm, grid;                // row lanes, workgroups = gm * nct
    int tiles_min, tiles_max;    // pixel tiles the workgroups walk
};
inline HaloPlan conv3_halo_plan(int n_img, int OH, int OW, int Np, int n_cu) {
    HaloPlan r;
    // (256 columns: two column tiles of 128.  A 256-column tile -- 128 accumulator registers per wave -- spills at two waves per SIMD)
    r.nc = Np == 64 ? 64 : 128;
    r.nct = Np / r.nc;
    r.tiles_x = cdiv(OW, HaloCfg<64>::TW); r.tiles_y = cdiv(OH, HaloCfg<64>::TH);
    r.ntile = n_img * r.tiles_y * r.tiles_x;
    r.gm = persistent_grid(r.ntile, n_cu / r.nct);
    r.grid = r.gm * r.nct;
    r.tiles_min = r.ntile / r.gm;
    r.tiles_max = cdiv(r.ntile, r.gm);
    return r;
}

template <typename T, int NC, int ACT>
static int launch_conv3_halo_t(const ConvParams& p_in, const HaloPlan& pl, hipStream_t stream) {
    using C = HaloCfg<NC>;
    static_assert(C::TW == HaloCfg<64>::TW && C::TH == HaloCfg<64>::TH, "one pixel tile for every column width");
    ConvParams p = p_in;
    OCRVI_TRY(ring_pages(&p.zero_page, &p.dump_page));
    auto kern = conv3_halo_kernel<T, NC, ACT>;
    OCRVI_TRY(ensure_max_smem((const void*)kern, C::SMEM));
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(512), C::SMEM, stream, p, pl.tiles_x, pl.tiles_y);
    OCRVI_HIP(hipGetLastError());
    return OCRVI_OK;
}

template <typename T, int NC>
static int launch_conv3_halo_n(const ConvParams& p, const HaloPlan& pl, hipStream_t stream) {
    if (p.act == ACT_RELU) return launch_conv3_halo_t<T, NC, ACT_RELU>(p, pl, stream);
    return launch_conv3_halo_t<T, NC, ACT_NONE>(p, pl, stream);
}

template <typename T>
static int launch_conv3_halo(const ConvParams& p, hipStream_t stream) {
    if constexpr (IsSplit<T>::value) {
        if (p.Np == 256 || p.Np == 128 || p.Np == 64) {
            int n_cu = 0;
            OCRVI_TRY(device_cus(&n_cu));
            const HaloPlan pl = conv3_halo_plan(p.n_img, p.OH, p.OW, p.Np, n_cu);
            if (pl.nc == 128) return launch_conv3_halo_n<T, 128>(p, pl, stream);
            return launch_conv3_halo_n<T, 64>(p, pl, stream);
        }
    }
    set_error("conv3_halo: unsupported call (Np=%d)", p.Np);
    return OCRVI_EINVAL;
}

}  // namespace ocrvi
